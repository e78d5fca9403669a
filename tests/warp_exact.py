"""Lattice cases for the warp kernels (csrc/warp.hip, csrc/warp_tile.hip) and their fp64 reference.  Host only.

Method.  src and d_out hold small integers, every flow component is a multiple of 1/4.  A trilinear weight is then a multiple
of 1/64, and every product and partial sum the kernels form -- in any order -- is a dyadic rational of far fewer than 24 bits:
fp32 is exact, and so is the 2^-40 fixed point of the deterministic and the destination-tile paths.  A kernel's result must
therefore EQUAL the fp64 reference; a lost, doubled or misplaced contribution is an error of order 1.  tests/test_cpu_warp_exact.py
proves the premise on the host (fp64 == fp32 oracle, the 2^24 cap), tests/test_gpu_warp_exact.py holds the kernels to it.

Reference: oracle.modet_torch.warp in fp64 with autograd -- direct voxel coordinates with floor and round, which is the contract
of include/modet_hip.h: floor for the base corner (the right-hand derivative at an integer coordinate), zero padding, ties to
even in the nearest mode.  (Not grid_sample behind the reference's normalise round trip: at lattice positions that round trip is
not the identity and flips floor.)

All arrays are channels-last: src / d_out (B,D,H,W,C), flow / d_flow_add (B,D,H,W,3) float32; labels (D,H,W) int16."""
import zlib

import numpy as np
import torch

NLABELS = 54                  # counted range 0..54; the label maps hold 0..56, so 55 and 56 stay uncounted
LABEL_MAX = 56

# ---- shapes (B, D, H, W), each checked against the host conditions of modet_warp_bwd_acc (csrc/warp.hip) and tiles_launch
# (csrc/warp_tile.hip).  patch(C) = B * ceil(D/8) * ceil(H/4) * W * G, G = C rounded up to a power of two: warp_bwd2_kernel (x, y
# and z merges) runs from 65 536 = 256 * 256 items, warp_bwd_kernel (x and z merges, ZRUN = 8) below.  The other conditions of
# the patch form -- tensor below 2 GiB, (D+3)(H+3)(W+3) < 2^23, W * C * 4 < 2^23 -- hold for every shape here.  The fill pass of
# the tile path takes SZ = 1 below 400 000 voxels and SZ = 4 from there; its source block is SZ x 8 x 32 voxels, a destination
# tile 8^3, a tile of the bounded gather 4 x 4 x 16.
SHAPES = {
    # one partial tile, every voxel on a face.  patch: 1*1*2*7*G = 14 G <= 896: warp_bwd_kernel for every C.  210 voxels: SZ = 1
    "5x6x7": (1, 5, 6, 7),
    # a partial tile on every axis; W crosses the 32-wide fill block and the 16-wide gather tile; D = ZRUN + 1; two samples.
    # patch: 2*2*4*35*G = 560 G <= 35 840 (C = 64): warp_bwd_kernel for every C.  8 190 voxels: SZ = 1
    "9x13x35": (2, 9, 13, 35),
    # whole tiles, two samples; the only shape of `collapse` (the cap, tests/test_cpu_warp_exact.py).
    # patch: 2*3*8*40*G = 1 920 G = 30 720 at C = 16: warp_bwd_kernel (C <= 16 here).  61 440 voxels: SZ = 1
    "24x32x40": (2, 24, 32, 40),
    # patch: 1*3*11*250*G = 8 250 G: C = 3 (G = 4) 33 000 stays on warp_bwd_kernel; C = 8 gives 66 000 >= 65 536, C = 12 and 16
    # (G = 16) 132 000: warp_bwd2_kernel.  174 250 voxels: SZ = 1
    "17x41x250": (1, 17, 41, 250),
    # 406 890 voxels >= 400 000: SZ = 4.  patch: 2*5*12*137*G = 16 440 G: 65 760 already at C = 3 (G = 4): warp_bwd2_kernel for
    # every C.  No axis is a multiple of 4 or 8.  C <= 16 here (the fp64 reference stays at a second or two)
    "33x45x137": (2, 33, 45, 137),
}
PATCH_MIN = 256 * 256
FILL_SZ4_MIN = 400000


def pow2_at_least(C):
    G = 1
    while G < C:
        G <<= 1
    return G


def patch_items(shape, C):
    B, D, H, W = shape
    return B * ((D + 7) // 8) * ((H + 3) // 4) * W * pow2_at_least(C)


def runs_patch_kernel(shape, C):
    """True where modet_warp_bwd_acc / _det (with d_src) take warp_bwd2_kernel"""
    return patch_items(shape, C) >= PATCH_MIN


def fill_sz(shape):
    B, D, H, W = shape
    return 4 if B * D * H * W >= FILL_SZ4_MIN else 1


# ---- flow families.  Every component is a multiple of 1/4 (HALF_LATTICE: of 1/2, so nearest-mode ties are everywhere); every
# position is kept inside [-2, dim + 1].
SHIFTS = [(0.5, -1.25, 2.0), (-0.75, 0.25, -3.0)]                # one constant vector per sample: every x, y and z merge fires
# integer shifts: every fraction is 0, so four to seven corners have weight exactly 0.  Sample 0 puts the z = 0 face on position
# -1 and (no shift along y) the opposite y face on H - 1; sample 1 puts the z = D - 2 plane on D - 1 and the last one on D
ISHIFTS = [(-1.0, 0.0, 2.0), (1.0, -3.0, 0.0)]
COLLAPSE_TARGETS = [(8.0, 16.0, 24.0), (16.0, 8.0, 32.0)]        # tile corners (8a, 8b, 8c) inside 24x32x40
FACE_SWEEP = np.arange(-1.25, 0.26, 0.25)                         # -1.25 ... 0.25; the high faces use dim + the same
FAMILIES = ("zero", "shift", "ishift", "contract", "expand", "white", "white1", "faces", "collapse", "rewrap", "half")
HALF_LATTICE = ("zero", "ishift", "half")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _index_grids(D, H, W):
    return np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")


def make_flow(family, shape):
    B, D, H, W = shape
    dims = (D, H, W)
    idx = np.stack(_index_grids(D, H, W), -1).astype(np.float64)               # (D,H,W,3)
    rng = _rng("flow", family, shape)
    f = np.zeros((B, D, H, W, 3))
    if family == "zero":
        pass
    elif family in ("shift", "ishift"):
        for b in range(B):
            f[b] = (SHIFTS if family == "shift" else ISHIFTS)[b]
    elif family in ("contract", "expand"):
        c = (np.array(dims, dtype=np.float64) - 1.0) / 2.0
        q = np.round(-(idx - c) / 4.0 * 4.0) / 4.0                             # smooth; cells collide; merge runs break regularly
        f[:] = q if family == "contract" else -q
    elif family == "white":
        f = rng.integers(-12, 13, f.shape) / 4.0
    elif family == "white1":
        f = rng.integers(-4, 5, f.shape) / 4.0                                 # includes exactly +-1 (flow_bound = 1)
    elif family == "half":
        f = rng.integers(-6, 7, f.shape) / 2.0
    elif family == "faces":
        f = rng.integers(-12, 13, f.shape) / 4.0
        g = _index_grids(D, H, W)
        for a in range(3):
            u, v = [g[o] for o in range(3) if o != a]
            k = (u + 3 * v) % len(FACE_SWEEP)
            lo, hi = g[a] == 0, g[a] == dims[a] - 1
            for b in range(B):
                kb = (k + b) % len(FACE_SWEEP)
                f[b, ..., a] = np.where(lo, FACE_SWEEP[kb] - 0.0, f[b, ..., a])
                f[b, ..., a] = np.where(hi, dims[a] + FACE_SWEEP[kb] - (dims[a] - 1), f[b, ..., a])
    elif family == "rewrap":
        # smooth along the LINEAR voxel order instead of along x: voxel n = y * W + x of a plane lands on x = n mod (W - 1) + 1/4,
        # y = n div (W - 1) + 1/2, so the first voxel of a row continues the footprint sequence of the previous row's last one --
        # the one place where "the lane G up is this footprint shifted by +1 in x" holds and the x merge must still not fire
        n = idx[..., 1] * W + idx[..., 2]
        f[..., 0] = 0.25
        f[..., 1] = np.floor(n / (W - 1)) + 0.5 - idx[..., 1]
        f[..., 2] = np.mod(n, W - 1) + 0.25 - idx[..., 2]
    elif family == "collapse":
        for b in range(B):
            f[b] = np.array(COLLAPSE_TARGETS[b]) - idx + rng.integers(-2, 3, idx.shape) / 4.0
    else:
        raise KeyError(family)
    pos = np.clip(idx[None] + f, -2.0, np.array(dims, dtype=np.float64) + 1.0)
    f = pos - idx[None]
    assert np.array_equal(f * 4.0, np.round(f * 4.0))
    return np.ascontiguousarray(f.astype(np.float32))


def make_src(shape, C):
    B, D, H, W = shape
    return _rng("src", shape, C).integers(-8, 9, (B, D, H, W, C)).astype(np.float32)         # bf16-exact as well


def make_dout(shape, C):
    B, D, H, W = shape
    g = _rng("dout", shape, C).integers(-4, 5, (B, D, H, W, C)).astype(np.float32)
    g[:, : max(1, D // 3), H // 2:] = 0.0                                      # a block of exact zeros (the tile path drops those voxels)
    return g


def make_dflow_add(shape):
    B, D, H, W = shape
    return (_rng("add", shape).integers(-8, 9, (B, D, H, W, 3)) / 4.0).astype(np.float32)


def make_labels(shape):
    """(moving, fixed) int16 (D,H,W) maps with labels 0..56; about half of the fixed voxels repeat the moving map"""
    _, D, H, W = shape
    rng = _rng("labels", shape)
    mov = rng.integers(0, LABEL_MAX + 1, (D, H, W)).astype(np.int16)
    fix = np.where(rng.random((D, H, W)) < 0.5, mov, rng.integers(0, LABEL_MAX + 1, (D, H, W))).astype(np.int16)
    return mov, fix


# ---- the case table: (shape, C, family).  tests/test_cpu_warp_exact.py checks the premise on every one of them.
def _table():
    t = []
    small = ("5x6x7", "9x13x35")
    for s in small:
        for C in (3, 8, 16):
            t += [(s, C, f) for f in ("zero", "shift", "ishift", "contract", "expand", "white", "faces")]
        for C in (12, 64):                       # dead channel lanes (G = 16) / no x neighbour inside the wave (G = 64)
            t += [(s, C, f) for f in ("shift", "contract", "faces")]
        for C in (1, 5, 6):                      # forward only: one and three channels per thread
            t += [(s, C, f) for f in ("shift", "white", "faces")]
        t += [(s, 3, "white1"), (s, 8, "rewrap"), (s, 1, "half"), (s, 4, "half")]
    s = "24x32x40"
    for C in (3, 8, 16):
        t += [(s, C, f) for f in ("shift", "contract", "white", "faces", "collapse")]
    t += [(s, 3, "white1"), (s, 3, "zero"), (s, 8, "rewrap"), (s, 1, "half"), (s, 4, "half")]
    s = "17x41x250"
    t += [(s, 8, f) for f in ("shift", "ishift", "contract", "expand", "white", "faces", "rewrap")]
    t += [(s, 3, f) for f in ("shift", "faces", "white1")]
    t += [(s, 12, f) for f in ("shift", "faces")]
    t += [(s, 16, f) for f in ("contract", "white")]
    s = "33x45x137"
    t += [(s, 3, f) for f in ("shift", "contract", "expand", "white", "faces")]
    t += [(s, 8, f) for f in ("shift", "faces")]
    t += [(s, 16, f) for f in ("contract", "white")]
    return t


CASES = _table()
LABEL_CASES = [(s, f) for s in ("5x6x7", "9x13x35", "24x32x40", "33x45x137") for f in ("half", "faces", "ishift")]


def case_id(case):
    return "-".join(str(v) for v in case)


def select(shapes=None, Cs=None, families=None):
    return [c for c in CASES if (shapes is None or c[0] in shapes) and (Cs is None or c[1] in Cs)
            and (families is None or c[2] in families)]


_IN, _REF, _LAB = {}, {}, {}


def inputs(case):
    """{'src', 'flow', 'dout', 'add'}: read-only float32 tensors, made once per case"""
    if case not in _IN:
        s, C, fam = case
        shape = SHAPES[s]
        _IN[case] = {"src": torch.from_numpy(make_src(shape, C)), "flow": torch.from_numpy(make_flow(fam, shape)),
                     "dout": torch.from_numpy(make_dout(shape, C)), "add": torch.from_numpy(make_dflow_add(shape))}
    return _IN[case]


def _nc(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def oracle(case, dtype=torch.float64, abs_dout=False):
    """oracle.modet_torch.warp with autograd in ``dtype`` -> (out, d_src, d_flow, out_nearest), channels-last, in ``dtype``.
    abs_dout: the gradient of |d_out| -- per d_src cell the sum of |w * d_out| (the weights are non-negative)"""
    from oracle import modet_torch as orc
    x = inputs(case)
    src = _nc(x["src"]).to(dtype).requires_grad_(True)
    flow = _nc(x["flow"]).to(dtype).requires_grad_(True)
    go = _nc(x["dout"]).to(dtype)
    out = orc.warp(src, flow)
    ds, df = torch.autograd.grad(out, [src, flow], go.abs() if abs_dout else go)
    with torch.no_grad():
        near = orc.warp(src.detach(), flow.detach(), "nearest")
    return _cl(out.detach()), _cl(ds), _cl(df), _cl(near)


def reference(case):
    """the fp64 oracle's answer as float32 tensors (exact: test_cpu_warp_exact), computed once per case and shared read-only:
    out, dsrc, dflow, near; the derived forms add exactly representable terms: out + flow (add_flow), d_flow + d_out (add_flow's
    identity term, C == 3), + d_flow_add"""
    if case not in _REF:
        out, ds, df, near = oracle(case)
        r = {"out": out.float(), "dsrc": ds.float(), "dflow": df.float(), "near": near.float()}
        for k, v in zip(("out", "dsrc", "dflow", "near"), (out, ds, df, near)):
            assert torch.equal(r[k].double(), v), (case, k)
        _REF[case] = r
    return _REF[case]


def expected_out(case, add_flow=False):
    r, x = reference(case), inputs(case)
    return (r["out"].double() + x["flow"].double()).float() if add_flow else r["out"]


def expected_dflow(case, add_flow=False, add=False):
    r, x = reference(case), inputs(case)
    g = r["dflow"].double()
    if add_flow:
        g = g + x["dout"].double()
    if add:
        g = g + x["add"].double()
    return g.float()


def label_case(key):
    """(moving, fixed, flow (B,D,H,W,3), warped (B,D,H,W) int16, counts (B,3,NLABELS+1) int64): the reference's nearest warp of
    the moving map per sample of the flow, and np.bincount over the counted range"""
    if key not in _LAB:
        from oracle import modet_torch as orc
        s, fam = key
        shape = SHAPES[s]
        mov, fix = make_labels(shape)
        flow = torch.from_numpy(make_flow(fam, shape))
        B = shape[0]
        m = torch.from_numpy(mov.astype(np.float64))[None, None].expand(B, 1, *mov.shape)
        w = orc.warp(m, _nc(flow).double(), "nearest")[:, 0].numpy()
        assert np.array_equal(w, np.round(w))
        warped = w.astype(np.int16)
        counts = np.zeros((B, 3, NLABELS + 1), dtype=np.int64)
        n1 = NLABELS + 1
        for b in range(B):
            wb = warped[b].reshape(-1).astype(np.int64)
            fb = fix.reshape(-1).astype(np.int64)
            counts[b, 0] = np.bincount(wb[wb < n1], minlength=n1)
            counts[b, 1] = np.bincount(fb[fb < n1], minlength=n1)
            hit = wb[(wb == fb) & (wb < n1)]
            counts[b, 2] = np.bincount(hit, minlength=n1)
        _LAB[key] = (mov, fix, flow, warped, counts)
    return _LAB[key]


def tie_fraction(flow):
    """fraction of voxels with at least one coordinate at an exact .5 (the identity grid is integer: the flow decides)"""
    f = flow.numpy() if torch.is_tensor(flow) else flow
    return float((np.abs(f - np.floor(f)) == 0.5).any(-1).mean())


def positions(flow):
    f = flow.numpy() if torch.is_tensor(flow) else flow
    B, D, H, W, _ = f.shape
    return f.astype(np.float64) + np.stack(_index_grids(D, H, W), -1)[None]
