"""-m gpu: every warp entry point (csrc/warp.hip, csrc/warp_tile.hip) against the fp64 oracle on the lattice cases of
tests/warp_exact.py, bit for bit.

src and d_out hold small integers and every flow component is a multiple of 1/4 (1/2 for the nearest mode), so nothing is left to
rounding (tests/test_cpu_warp_exact.py proves it on the host): every comparison below is torch.equal.  What that pins and the
tolerance tests cannot: which of the eight corners is inside the volume at positions exactly on -1, 0, dim - 1 and dim; floor at
an integer coordinate; ties to even in the nearest mode; every contribution handed over by the x, y and z merges of the scatter
kernels, the tile a base corner belongs to, the 217 high-face cells of a tile window, the overflow list, the tiles of the
bounded gather -- each arriving once, in the right cell.

The entry points are called raw through _lib.load(); output buffers and workspaces are filled with NaN first."""
import pytest
import torch

from tests import warp_exact as wx

pytestmark = pytest.mark.gpu

NAN = float("nan")
BWD_C = (3, 8, 12, 16, 64)
FWD_CASES = wx.select(families=[f for f in wx.FAMILIES if f != "half"])
NEAR_CASES = wx.select(families=["half"])
BWD_CASES = [c for c in FWD_CASES if c[1] in BWD_C]
TILE_CASES = [c for c in BWD_CASES if c[1] in (3, 8, 16)]
BOUND_CASES = wx.select(Cs=[3], families=["white1", "zero"])


def same(entry, case, what, got, want):
    """got == want in every element, or a failure naming the entry point, the case, how many differ and the first index"""
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, (entry, case, what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g, w = got.detach().cpu(), want.cpu()
    bad = (g != w).nonzero()
    first = tuple(bad[0].tolist())
    raise AssertionError(f"{entry} [{wx.case_id(case)}] {what}: {bad.shape[0]} of {g.numel()} elements differ, first at {first}: "
                         f"got {g[first].item()!r}, want {w[first].item()!r}")


def nan_like(t, dtype=None):
    return torch.full(t.shape, NAN, dtype=dtype or t.dtype, device="cuda")


def nan_ws(nbytes):
    return torch.full((nbytes // 4 + 8,), NAN, dtype=torch.float32, device="cuda")


class Case:
    def __init__(self, case):
        from smilecode_amd import _lib
        self.case, self.lib, self.L = case, _lib, _lib.load()
        self.shape = wx.SHAPES[case[0]]
        self.C = case[1]
        x = wx.inputs(case)
        self.src, self.flow, self.dout, self.add = (x[k].cuda() for k in ("src", "flow", "dout", "add"))
        self.dims = self.shape + (self.C,)
        self.st = torch.cuda.current_stream().cuda_stream

    def ok(self, code, what):
        self.lib.check(code, what)


def p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", FWD_CASES, ids=wx.case_id)
def test_forward_trilinear(case):
    """modet_warp_fwd mode 0: C = 1, 5 (one channel per thread), 3, 6 (three), 8, 12, 16, 64 (four); C = 3 also with add_flow"""
    k = Case(case)
    out = nan_like(k.src)
    k.ok(k.L.modet_warp_fwd(p(k.src), p(k.flow), p(out), *k.dims, 0, 0, k.st), "warp_fwd")
    same("modet_warp_fwd", case, "out", out, wx.reference(case)["out"])
    if k.C == 3:
        out = nan_like(k.src)
        k.ok(k.L.modet_warp_fwd(p(k.src), p(k.flow), p(out), *k.dims, 0, 1, k.st), "warp_fwd add_flow")
        same("modet_warp_fwd add_flow", case, "out", out, wx.expected_out(case, True))


@pytest.mark.parametrize("case", [c for c in FWD_CASES if c[1] == 8], ids=wx.case_id)
def test_forward_bf16_forms(case):
    """modet_warp_fwd_t with the three bf16 combinations and modet_warp_fwd_o16: the integer src is a bf16 number, and a bf16
    output is the exact result rounded once"""
    k = Case(case)
    want = wx.reference(case)["out"]
    s16 = k.src.bfloat16()
    for src_bf16, out_bf16 in ((1, 0), (0, 1), (1, 1)):
        out = nan_like(k.src, torch.bfloat16 if out_bf16 else torch.float32)
        k.ok(k.L.modet_warp_fwd_t(p(s16 if src_bf16 else k.src), src_bf16, p(k.flow), p(out), out_bf16, *k.dims, k.st), "warp_fwd_t")
        same(f"modet_warp_fwd_t src_bf16={src_bf16} out_bf16={out_bf16}", case, "out", out, want.bfloat16() if out_bf16 else want)
    out = nan_like(k.src, torch.bfloat16)
    k.ok(k.L.modet_warp_fwd_o16(p(k.src), p(k.flow), p(out), *k.dims, k.st), "warp_fwd_o16")
    same("modet_warp_fwd_o16", case, "out", out, want.bfloat16())


@pytest.mark.parametrize("case", NEAR_CASES, ids=wx.case_id)
def test_forward_nearest_rounds_ties_to_even(case):
    """modet_warp_fwd mode 1 on the half lattice (more than 80 % of the voxels have a coordinate at an exact tie)"""
    k = Case(case)
    out = nan_like(k.src)
    k.ok(k.L.modet_warp_fwd(p(k.src), p(k.flow), p(out), *k.dims, 1, 0, k.st), "warp_fwd nearest")
    same("modet_warp_fwd mode 1", case, "out", out, wx.reference(case)["near"])


# ------------------------------------------------------------------------------------------------ backward, scatter kernels
@pytest.mark.parametrize("case", BWD_CASES, ids=wx.case_id)
def test_backward_float_atomics(case):
    """modet_warp_bwd_acc: warp_bwd_kernel below the patch threshold, warp_bwd2_kernel from it (tests/warp_exact.py SHAPES).
    C = 3 (G = 4: one dead lane), 8, 12 (G = 16: four dead lanes), 16, 64 (G = 64: no x neighbour inside the wave)"""
    k = Case(case)
    r = wx.reference(case)
    kern = "warp_bwd2_kernel" if wx.runs_patch_kernel(k.shape, k.C) else "warp_bwd_kernel"
    for add in (False, True):
        ds, df = nan_like(k.src), nan_like(k.flow)
        k.ok(k.L.modet_warp_bwd_acc(p(k.src), 0, p(k.flow), p(k.dout), p(ds), p(df), p(k.add if add else None), *k.dims, 0, 0, k.st), "bwd_acc")
        same(f"modet_warp_bwd_acc ({kern}) add={add}", case, "d_src", ds, r["dsrc"])
        same(f"modet_warp_bwd_acc ({kern}) add={add}", case, "d_flow", df, wx.expected_dflow(case, False, add))
    ds = nan_like(k.src)
    k.ok(k.L.modet_warp_bwd_acc(p(k.src), 0, p(k.flow), p(k.dout), p(ds), None, None, *k.dims, 0, 0, k.st), "bwd_acc d_src alone")
    same(f"modet_warp_bwd_acc ({kern}) d_src alone", case, "d_src", ds, r["dsrc"])
    df = nan_like(k.flow)
    k.ok(k.L.modet_warp_bwd_acc(p(k.src), 0, p(k.flow), p(k.dout), None, p(df), p(k.add), *k.dims, 0, 0, k.st), "bwd_acc d_flow alone")
    same("modet_warp_bwd_acc (warp_bwd_kernel) d_flow alone", case, "d_flow", df, wx.expected_dflow(case, False, True))
    s16 = k.src.bfloat16()
    ds, df = nan_like(k.src), nan_like(k.flow)
    k.ok(k.L.modet_warp_bwd_acc(p(s16), 1, p(k.flow), p(k.dout), p(ds), p(df), p(k.add), *k.dims, 0, 0, k.st), "bwd_acc src_bf16")
    same(f"modet_warp_bwd_acc ({kern}) src_bf16", case, "d_src", ds, r["dsrc"])
    same(f"modet_warp_bwd_acc ({kern}) src_bf16", case, "d_flow", df, wx.expected_dflow(case, False, True))
    if k.C == 3:
        ds, df = nan_like(k.src), nan_like(k.flow)
        k.ok(k.L.modet_warp_bwd_acc(p(k.src), 0, p(k.flow), p(k.dout), p(ds), p(df), p(k.add), *k.dims, 1, 0, k.st), "bwd_acc add_flow")
        same(f"modet_warp_bwd_acc ({kern}) add_flow", case, "d_src", ds, r["dsrc"])
        same(f"modet_warp_bwd_acc ({kern}) add_flow", case, "d_flow", df, wx.expected_dflow(case, True, True))


@pytest.mark.parametrize("case", BWD_CASES, ids=wx.case_id)
def test_backward_deterministic_atomics(case):
    """modet_warp_bwd_det: the same two kernels with 64-bit fixed-point integer atomics"""
    k = Case(case)
    r = wx.reference(case)
    kern = "warp_bwd2_kernel" if wx.runs_patch_kernel(k.shape, k.C) else "warp_bwd_kernel"
    nb = k.L.modet_warp_bwd_det_ws_bytes(*k.dims)
    for add, af, s16 in ((False, 0, 0), (True, 0, 0), (True, 0, 1)) + (((True, 1, 0),) if k.C == 3 else ()):
        ds, df, ws = nan_like(k.src), nan_like(k.flow), nan_ws(nb)
        src = k.src.bfloat16() if s16 else k.src
        k.ok(k.L.modet_warp_bwd_det(p(src), s16, p(k.flow), p(k.dout), p(ds), p(df), p(k.add if add else None), p(ws), nb, *k.dims, af, k.st), "bwd_det")
        what = f"modet_warp_bwd_det ({kern}) add={add} add_flow={af} src_bf16={s16}"
        same(what, case, "d_src", ds, r["dsrc"])
        same(what, case, "d_flow", df, wx.expected_dflow(case, bool(af), add))
    ds, ws = nan_like(k.src), nan_ws(nb)
    k.ok(k.L.modet_warp_bwd_det(p(k.src), 0, p(k.flow), p(k.dout), p(ds), None, None, p(ws), nb, *k.dims, 0, k.st), "bwd_det d_src alone")
    same(f"modet_warp_bwd_det ({kern}) d_src alone", case, "d_src", ds, r["dsrc"])


@pytest.mark.parametrize("case", BOUND_CASES, ids=wx.case_id)
def test_backward_bounded_flow_gather(case):
    """modet_warp_bwd with flow_bound = 1 (warp_bwd_gather3_tiled_kernel, 4 x 4 x 16 tiles with a one-voxel halo): flows in
    [-1, 1] including exactly +-1, where a hat weight is exactly 0 or 1"""
    k = Case(case)
    r = wx.reference(case)
    for af in (0, 1):
        ds, df = nan_like(k.src), nan_like(k.flow)
        k.ok(k.L.modet_warp_bwd(p(k.src), p(k.flow), p(k.dout), p(ds), p(df), *k.dims, af, 1, k.st), "warp_bwd flow_bound")
        same(f"modet_warp_bwd flow_bound=1 add_flow={af}", case, "d_src", ds, r["dsrc"])
        same(f"modet_warp_bwd flow_bound=1 add_flow={af}", case, "d_flow", df, wx.expected_dflow(case, bool(af), False))
    ds = nan_like(k.src)
    k.ok(k.L.modet_warp_bwd(p(k.src), p(k.flow), p(k.dout), p(ds), None, *k.dims, 0, 1, k.st), "warp_bwd flow_bound d_src alone")
    same("modet_warp_bwd flow_bound=1 d_src alone", case, "d_src", ds, r["dsrc"])


# ------------------------------------------------------------------------------------------------ backward, destination tiles
@pytest.mark.parametrize("case", TILE_CASES, ids=wx.case_id)
def test_backward_destination_tiles(case):
    """modet_warp_bwd_tiles / modet_warp_bwd_dsrc_tiles: C = 8, 16 (fp32 and bf16 src), C = 3 with add_flow 0 and 1; SZ = 1 and
    (33x45x137) SZ = 4; `collapse` sends a sample's 30 720 voxels to the eight tiles around one tile corner -- the overflow list
    beyond the 1 536-entry segments and the border pass carry most of it"""
    k = Case(case)
    r = wx.reference(case)
    tag = f"SZ={wx.fill_sz(k.shape)}"
    nb = k.L.modet_warp_bwd_dsrc_tiles_ws_bytes(*k.dims)
    assert nb > 0
    for add, af, s16 in [(False, 0, 0), (True, 0, 0)] + ([(True, 1, 0), (False, 1, 0)] if k.C == 3 else [(True, 0, 1)]):
        ds, df, ws = nan_like(k.src), nan_like(k.flow), nan_ws(nb)
        src = k.src.bfloat16() if s16 else k.src
        k.ok(k.L.modet_warp_bwd_tiles(p(src), s16, p(k.flow), p(k.dout), p(ds), p(df), p(k.add if add else None), p(ws), nb, *k.dims, af, k.st), "tiles")
        what = f"modet_warp_bwd_tiles {tag} add={add} add_flow={af} src_bf16={s16}"
        same(what, case, "d_src", ds, r["dsrc"])
        same(what, case, "d_flow", df, wx.expected_dflow(case, bool(af), add))
    ds, ws = nan_like(k.src), nan_ws(nb)
    k.ok(k.L.modet_warp_bwd_dsrc_tiles(p(k.flow), p(k.dout), p(ds), p(ws), nb, *k.dims, k.st), "dsrc_tiles")
    same(f"modet_warp_bwd_dsrc_tiles {tag}", case, "d_src", ds, r["dsrc"])


# ------------------------------------------------------------------------------------------------ routed through autograd
def _routed(ops, k, tee, add_flow, flow_bound=0):
    s_, f_ = k.src.clone().requires_grad_(True), k.flow.clone().requires_grad_(True)
    if tee:
        o, fl = ops.warp_tee(s_, f_)
        ((o * k.dout).sum() + (fl * k.add).sum()).backward()        # the second consumer's gradient is exactly `add`
    else:
        o = ops.warp(s_, f_, 0, add_flow, flow_bound)
        (o * k.dout).sum().backward()
    return o.detach(), s_.grad, f_.grad


@pytest.mark.parametrize("case", [c for c in BWD_CASES if c[2] in ("shift", "contract", "faces", "collapse", "rewrap", "white1")], ids=wx.case_id)
def test_autograd_routes_agree_with_the_reference_and_each_other(case, monkeypatch):
    """ops.warp and ops.warp_tee with WARP_TILES on and off and ops.set_deterministic(True): whichever kernels the route picks
    (tiles, the 64-bit integer atomics, the float atomics, the bounded gather), the bits are the reference's"""
    from smilecode_amd import ops
    k = Case(case)
    r = wx.reference(case)
    prev = ops.set_deterministic(False)
    try:
        for tiles in (True, False):
            for det in (False, True):
                monkeypatch.setattr(ops, "WARP_TILES", tiles)
                ops.set_deterministic(det)
                route = f"WARP_TILES={tiles} deterministic={det}"
                for add_flow in ((False, True) if k.C == 3 else (False,)):
                    o, ds, df = _routed(ops, k, False, add_flow)
                    same(f"ops.warp add_flow={add_flow} {route}", case, "out", o, wx.expected_out(case, add_flow))
                    same(f"ops.warp add_flow={add_flow} {route}", case, "d_src", ds, r["dsrc"])
                    same(f"ops.warp add_flow={add_flow} {route}", case, "d_flow", df, wx.expected_dflow(case, add_flow, False))
                o, ds, df = _routed(ops, k, True, False)
                same(f"ops.warp_tee {route}", case, "out", o, r["out"])
                same(f"ops.warp_tee {route}", case, "d_src", ds, r["dsrc"])
                same(f"ops.warp_tee {route}", case, "d_flow", df, wx.expected_dflow(case, False, True))
                if case[2] == "white1":
                    for add_flow in (False, True):
                        o, ds, df = _routed(ops, k, False, add_flow, 1)
                        same(f"ops.warp flow_bound=1 add_flow={add_flow} {route}", case, "d_src", ds, r["dsrc"])
                        same(f"ops.warp flow_bound=1 add_flow={add_flow} {route}", case, "d_flow", df, wx.expected_dflow(case, add_flow, False))
    finally:
        ops.set_deterministic(prev)


# ------------------------------------------------------------------------------------------------ evaluation tail
@pytest.mark.parametrize("key", wx.LABEL_CASES, ids=wx.case_id)
def test_label_warp_counts(key):
    """ops.label_warp_counts / modet_label_warp_counts on `half` (ties everywhere), `faces` (positions exactly on -1, -0.5, 0,
    dim - 1, dim - 0.5, dim) and `ishift`: the warped labels are the reference's, the counts its bincount over 0..54 with
    labels 55 and 56 uncounted; want_warped=False gives the same counts"""
    from smilecode_amd import _lib, ops
    L = _lib.load()
    mov, fix, flow, warped, counts = wx.label_case(key)
    D, H, W = mov.shape
    lm, lf = torch.from_numpy(mov).cuda(), torch.from_numpy(fix).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for b in range(flow.shape[0]):
        fb = flow[b:b + 1].contiguous().cuda()
        want_w, want_c = torch.from_numpy(warped[b]), torch.from_numpy(counts[b])
        w, c = ops.label_warp_counts(lm, fb, lf, wx.NLABELS)
        same("ops.label_warp_counts", key + (b,), "warped", w, want_w)
        same("ops.label_warp_counts", key + (b,), "counts", c, want_c)
        w0, c0 = ops.label_warp_counts(lm, fb, lf, wx.NLABELS, want_warped=False)
        assert w0 is None
        same("ops.label_warp_counts want_warped=False", key + (b,), "counts", c0, want_c)
        wr = torch.full((D, H, W), -1, dtype=torch.int16, device="cuda")
        cr = torch.full((3, wx.NLABELS + 1), -1, dtype=torch.int64, device="cuda")
        _lib.check(L.modet_label_warp_counts(p(lm), p(fb), p(lf), p(wr), p(cr), D, H, W, wx.NLABELS, st), "label_warp_counts")
        same("modet_label_warp_counts", key + (b,), "warped", wr, want_w)
        same("modet_label_warp_counts", key + (b,), "counts", cr, want_c)
