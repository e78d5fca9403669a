"""-m gpu: WHERE the PR++ family's kernels read and write -- tests/test_gpu_pcnet_guard.py's assertions over the family's own table
(_lib.FAMILIES["prpp"], include/modet_hip_prpp.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py), every
workspace is exactly modet_prpp_*_ws_bytes bytes, outputs and workspaces are poisoned, and the library is reached through a
recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an unguarded run bit
for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.

The shapes are those of tests/test_gpu_prpp_ops.py: the decoder input at one voxel, with a batch, on the scalar path (3 + 5
channels) and over several workgroups; ReLU over 1, 3, 4 and 1027 floats (tails of 1, 3, 0 and 3); the stack at 1 x 1 x 3, at
9 x 10 x 33 with a batch (strips of 32 voxels that cross rows, planes and samples; 3 lanes per dot product) and at C = 32; the
composition with a batch, with a row crossing a workgroup, on one coarse plane, on equal grids and on the exactness lattice.  Each
optional pointer is seen present and absent."""
import pytest
import torch

from tests import guard
from tests import prpp_oracle as orc
from tests.guard_family import DIM, NULL, UNSUP, WS, Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("prpp")
px = H.fixture()


def _p(t):
    return None if t is None else t.data_ptr()


def upcat_abi(n, want_x=True, want_skip=True):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, (d, h, w), C1, C2 = orc.UPCAT_CASES[n]
        x, skip, gy = (g(t) for t in orc.upcat_tensors(n))
        out = g.empty(gy.shape)
        dx = g.empty(x.shape) if want_x else None
        ds = g.empty(skip.shape) if want_skip else None
        _lib.check(L.modet_prpp_upcat_fwd(_p(x), _p(skip), _p(out), B, d, h, w, C1, C2, stream()), "upcat fwd")
        _lib.check(L.modet_prpp_upcat_bwd(_p(gy), _p(dx), _p(ds), B, d, h, w, C1, C2, stream()), "upcat bwd")
        named = {"out": out}
        named.update({k: v for k, v in (("d_x", dx), ("d_skip", ds)) if v is not None})
        return named
    return case


def relu_abi(n):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        x, t, gy = (g(v) for v in orc.relu_tensors(n))
        y, s, dt = g.empty((n,)), g.empty((n,)), g.empty((n,))
        _lib.check(L.modet_prpp_relu_fwd(_p(t), _p(y), n, stream()), "relu fwd")
        _lib.check(L.modet_prpp_relu_add_fwd(_p(x), _p(t), _p(s), n, stream()), "relu add")
        _lib.check(L.modet_prpp_relu_bwd(_p(gy), _p(y), _p(dt), n, stream()), "relu bwd")
        return {"y": y, "s": s, "d_t": dt}
    return case


def stack_abi(n, want_mov=True, want_fix=True):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, (D, Hh, W), C = orc.STACK_CASES[n]
        mov, fix, gy = (g(t) for t in orc.stack_tensors(n))
        nb = L.modet_prpp_stack_ws_bytes(B, D, Hh, W, C)
        assert nb > 0
        ws1, ws2 = g.ws(nb), g.ws(nb)
        out = g.empty(gy.shape)
        dm = g.empty(mov.shape) if want_mov else None
        df = g.empty(fix.shape) if want_fix else None
        _lib.check(L.modet_prpp_stack_fwd(_p(mov), _p(fix), _p(out), _p(ws1), nb, B, D, Hh, W, C, stream()), "stack fwd")
        _lib.check(L.modet_prpp_stack_bwd(_p(mov), _p(fix), _p(gy), _p(dm), _p(df), _p(ws2), nb, B, D, Hh, W, C, stream()), "stack bwd")
        named = {"out": out}
        named.update({k: v for k, v in (("d_mov", dm), ("d_fix", df)) if v is not None})
        return named
    return case


def compose_abi(n, want_src=True, want_w=True):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        src, w, gy = orc.compose_exact_tensors() if n == "exact" else orc.compose_tensors(n)
        dims = (src.shape[0],) + tuple(src.shape[1:4]) + tuple(w.shape[1:4])
        src, w, gy = g(src), g(w), g(gy)
        out = g.empty(w.shape)
        ds = g.empty(src.shape) if want_src else None
        dw = g.empty(w.shape) if want_w else None
        nb = L.modet_prpp_compose_ws_bytes(*dims[:4]) if want_src else 0
        ws = g.ws(nb) if want_src else None
        _lib.check(L.modet_prpp_compose_fwd(_p(src), _p(w), _p(out), *dims, stream()), "compose fwd")
        _lib.check(L.modet_prpp_compose_bwd(_p(src), _p(w), _p(gy), _p(ds), _p(dw), _p(ws), nb, *dims, stream()), "compose bwd")
        named = {"out": out}
        named.update({k: v for k, v in (("d_src", ds), ("d_w", dw)) if v is not None})
        return named
    return case


def ops_case(which, n):
    """the package's own wrappers under GuardedAlloc: outputs, gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import ops
        if which == "upcat":
            x, skip, gy = orc.upcat_tensors(n)
            leaves = [g(x).requires_grad_(True), g(skip).requires_grad_(True)]
            y = ops.upsample_nearest_cat(*leaves)
        elif which == "relu":
            x, t, gy = orc.relu_tensors(n)
            leaves = [g(x).requires_grad_(True), g(t).requires_grad_(True)]
            y = ops.relu_add(leaves[0], ops.relu(leaves[1]))
        elif which == "stack":
            mov, fix, gy = orc.stack_tensors(n)
            leaves = [g(mov).requires_grad_(True), g(fix).requires_grad_(True)]
            y = ops.corr_stack(*leaves)
        else:
            src, w, gy = orc.compose_tensors(n)
            leaves = [g(src).requires_grad_(True), g(w).requires_grad_(True)]
            y = ops.compose_cross(*leaves)
        grads = torch.autograd.grad(y, leaves, g(gy))
        out = {"y": y}
        out.update({"g%d" % i: v for i, v in enumerate(grads)})
        return out
    return case


CASES = {}
for _n in sorted(orc.UPCAT_CASES):
    CASES["abi[upcat case%d]" % _n] = upcat_abi(_n)
    CASES["ops[upcat case%d]" % _n] = ops_case("upcat", _n)
CASES["abi[upcat case3,d_skip only]"] = upcat_abi(3, want_x=False)
CASES["abi[upcat case2,d_x only]"] = upcat_abi(2, want_skip=False)
for _n in orc.RELU_SIZES:
    CASES["abi[relu %d]" % _n] = relu_abi(_n)
    CASES["ops[relu %d]" % _n] = ops_case("relu", _n)
for _n in sorted(orc.STACK_CASES):
    CASES["abi[stack case%d]" % _n] = stack_abi(_n)
    CASES["ops[stack case%d]" % _n] = ops_case("stack", _n)
CASES["abi[stack case2,d_mov only]"] = stack_abi(2, want_fix=False)
CASES["abi[stack case3,d_fix only]"] = stack_abi(3, want_mov=False)
for _n in sorted(orc.COMPOSE_CASES):
    CASES["abi[compose case%d]" % _n] = compose_abi(_n)
    CASES["ops[compose case%d]" % _n] = ops_case("compose", _n)
CASES["abi[compose exact]"] = compose_abi("exact")
CASES["abi[compose case1,d_w only]"] = compose_abi(1, want_src=False)
CASES["abi[compose case2,d_src only]"] = compose_abi(2, want_w=False)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_prpp_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import ops
    px.refuse = True
    z = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    for bad in (lambda: ops.upsample_nearest_cat(z(1, 2, 2, 2, 4), z(1, 4, 4, 5, 4)), lambda: ops.upsample_nearest_cat(z(1, 2, 2, 2, 4).double(), z(1, 4, 4, 4, 4)),
                lambda: ops.upsample_nearest_cat(z(1, 2, 2, 2, 4).cpu(), z(1, 4, 4, 4, 4)), lambda: ops.relu(z(0)), lambda: ops.relu(z(4, 2).t()),
                lambda: ops.relu_add(z(4), z(5)), lambda: ops.corr_stack(z(1, 2, 2, 2, 6), z(1, 2, 2, 2, 6)),
                lambda: ops.corr_stack(z(1, 2, 2, 2, 8), z(1, 2, 2, 3, 8)), lambda: ops.corr_stack(z(2, 2, 2, 8), z(2, 2, 2, 8)),
                lambda: ops.compose_cross(z(1, 2, 2, 2, 3), z(1, 4, 1, 4, 3)), lambda: ops.compose_cross(z(1, 2, 2, 2, 3), z(2, 4, 4, 4, 3)),
                lambda: ops.compose_cross(z(1, 2, 2, 2, 4), z(1, 4, 4, 4, 3))):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, counts below 1, channel counts outside the kernels', misaligned tensors and a short or misaligned workspace
    are answered with the library's error codes before any launch: the outputs keep their fill"""
    from smilecode_amd import _lib
    L, s = _lib.load(), stream()
    f7 = lambda *shape: torch.full(shape, 7.0, device="cuda")          # noqa: E731
    z = lambda *shape: torch.zeros(shape, device="cuda")               # noqa: E731
    x, skip, out = z(1, 2, 2, 2, 4), z(1, 4, 4, 4, 4), f7(1, 4, 4, 4, 8)
    up = lambda **kw: L.modet_prpp_upcat_fwd(*({**dict(x=_p(x), skip=_p(skip), out=_p(out), B=1, d=2, h=2, w=2, C1=4, C2=4, s=s), **kw}.values()))  # noqa: E731
    assert up(x=None) == NULL and up(skip=None) == NULL and up(out=None) == NULL
    assert up(B=0) == DIM and up(d=0) == DIM and up(C1=0) == DIM and up(C2=-4) == DIM and up(out=_p(out) + 2) == UNSUP
    dx, ds = f7(1, 2, 2, 2, 4), f7(1, 4, 4, 4, 4)
    assert L.modet_prpp_upcat_bwd(_p(out), None, None, 1, 2, 2, 2, 4, 4, s) == NULL and L.modet_prpp_upcat_bwd(None, _p(dx), _p(ds), 1, 2, 2, 2, 4, 4, s) == NULL
    assert L.modet_prpp_upcat_bwd(_p(out), _p(dx), _p(ds), 1, 2, 0, 2, 4, 4, s) == DIM
    a, y = z(8), f7(8)
    assert L.modet_prpp_relu_fwd(None, _p(y), 8, s) == NULL and L.modet_prpp_relu_fwd(_p(a), None, 8, s) == NULL
    assert L.modet_prpp_relu_fwd(_p(a), _p(y), 0, s) == DIM and L.modet_prpp_relu_fwd(_p(a) + 4, _p(y), 4, s) == UNSUP
    assert L.modet_prpp_relu_add_fwd(None, _p(a), _p(y), 8, s) == NULL and L.modet_prpp_relu_add_fwd(_p(a), _p(a), _p(y) + 8, 4, s) == UNSUP
    assert L.modet_prpp_relu_bwd(_p(a), None, _p(y), 8, s) == NULL and L.modet_prpp_relu_bwd(_p(a), _p(a), _p(y), -1, s) == DIM
    B, D, Hh, W, C = 1, 2, 3, 4, 8
    mov, row = z(B, D, Hh, W, C), f7(B, D, Hh, W, 2 * C + 27)
    dm = f7(B, D, Hh, W, C)
    nb = L.modet_prpp_stack_ws_bytes(B, D, Hh, W, C)
    ws = torch.empty(nb + 32, dtype=torch.uint8, device="cuda")
    st = lambda **kw: L.modet_prpp_stack_fwd(*({**dict(mov=_p(mov), fix=_p(mov), out=_p(row), ws=_p(ws), nb=nb, B=B, D=D, H=Hh, W=W, C=C, s=s), **kw}.values()))  # noqa: E731
    assert st(mov=None) == NULL and st(fix=None) == NULL and st(out=None) == NULL and st(ws=None) == NULL
    assert st(nb=nb - 1) == WS and st(ws=_p(ws) + 4) == WS and st(C=6) == UNSUP and st(C=132) == UNSUP and st(C=0) == DIM and st(W=0) == DIM
    assert st(mov=_p(mov) + 4) == UNSUP and st(out=_p(row) + 2) == UNSUP
    sb = lambda **kw: L.modet_prpp_stack_bwd(*({**dict(mov=_p(mov), fix=_p(mov), g=_p(row), dm=_p(dm), df=_p(dm), ws=_p(ws), nb=nb, B=B, D=D, H=Hh, W=W, C=C,  # noqa: E731
                                                      s=s), **kw}.values()))
    assert sb(dm=None, df=None) == NULL and sb(g=None) == NULL and sb(nb=nb - 4) == WS and sb(dm=_p(dm) + 4) == UNSUP and sb(B=0) == DIM
    src, w, o3 = z(1, 2, 3, 5, 3), z(1, 4, 6, 10, 3), f7(1, 4, 6, 10, 3)
    dsrc = f7(1, 2, 3, 5, 3)
    nbc = L.modet_prpp_compose_ws_bytes(1, 2, 3, 5)
    wsc = torch.empty(nbc + 32, dtype=torch.uint8, device="cuda")
    cf = lambda **kw: L.modet_prpp_compose_fwd(*({**dict(src=_p(src), w=_p(w), out=_p(o3), B=1, Dc=2, Hc=3, Wc=5, Df=4, Hf=6, Wf=10, s=s), **kw}.values()))  # noqa: E731
    assert cf(src=None) == NULL and cf(w=None) == NULL and cf(out=None) == NULL and cf(B=0) == DIM and cf(Dc=0) == DIM and cf(Hf=1) == DIM
    assert cf(out=_p(o3) + 2) == UNSUP
    cb = lambda **kw: L.modet_prpp_compose_bwd(*({**dict(src=_p(src), w=_p(w), g=_p(w), ds=_p(dsrc), dw=_p(o3), ws=_p(wsc), nb=nbc, B=1, Dc=2, Hc=3, Wc=5,  # noqa: E731
                                                        Df=4, Hf=6, Wf=10, s=s), **kw}.values()))
    assert cb(ds=None, dw=None) == NULL and cb(g=None) == NULL and cb(ws=None) == NULL and cb(nb=nbc - 8) == WS and cb(ws=_p(wsc) + 8) == WS
    assert cb(Wf=1) == DIM and cb(B=65536) == DIM
    torch.cuda.synchronize()
    for v in (out, dx, ds, y, row, dm, o3, dsrc):
        assert bool((v == 7.0).all())                                       # nothing was launched


def test_every_launching_prpp_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- either gradient of the
    decoder input, of the stack and of the composition, and the composition's workspace -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_prpp_upcat_fwd": ((), (0, 1, 2)),                          # x skip out | stream
        "modet_prpp_upcat_bwd": ((1, 2), (0,)),                           # d_out d_x d_skip | stream
        "modet_prpp_relu_fwd": ((), (0, 1)),                              # t y | stream
        "modet_prpp_relu_add_fwd": ((), (0, 1, 2)),                       # x t out | stream
        "modet_prpp_relu_bwd": ((), (0, 1, 2)),                           # d_y y d_t | stream
        "modet_prpp_stack_fwd": ((), (0, 1, 2, 3)),                       # mov fix out ws | stream
        "modet_prpp_stack_bwd": ((3, 4), (0, 1, 2, 5)),                   # mov fix d_out d_mov d_fix ws | stream
        "modet_prpp_compose_fwd": ((), (0, 1, 2)),                        # src w out | stream
        "modet_prpp_compose_bwd": ((3, 4, 5), (0, 1, 2)),                   # src w d_out d_src d_w ws | stream
    })
