"""-m gpu: WHERE the stride-2 4x4x4 transposed-convolution kernels read and write -- tests/test_gpu_convs2_guard.py's assertions
over the family's own table (_lib.FAMILIES["deconv"], include/modet_hip_deconv.h).  Every caller-supplied tensor sits between guard
bands (tests/guard.py), every workspace is exactly modet_deconv4s2_ws_bytes(..., pass) bytes, outputs and workspaces are poisoned,
and the library is reached through a recording proxy over the new table.  Per case: no band is damaged, every result is finite,
the results equal an unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same
bits.  The shapes: cases 1, 3, 4 and 6 of tests/test_gpu_deconv.py (a single input voxel, 3 -> 3 channels with scalar tails on both
sides, the 259-channel tail of x / d_x beside 16-byte loads of y, several tiles with a partial one in every axis)."""
import pytest
import torch

from tests import guard
from tests import rcn_oracle as orc
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("deconv")
px = H.fixture()


def abi_case(n, bias=None):
    """the C ABI directly, exact workspaces: forward, data gradient, weight gradient"""
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, (D_, H_, W_), Cin, Cout, has_bias, slope = orc.OP_CASES[n]
        use_bias = has_bias if bias is None else bias
        x, w, b, gy = orc.case_tensors(n)
        x, w, gy = g(x), g(w), g(gy)
        b = g(b if b is not None else torch.full((Cout,), 0.25)) if use_bias else None
        act, sl = int(slope is not None), float(slope or 0.0)
        dims = (B, D_, H_, W_, Cin, Cout)
        y, dx, dw = g.empty(gy.shape), g.empty(x.shape), g.empty(w.shape)
        db = g.empty((Cout,)) if use_bias else None
        p = lambda v: None if v is None else v.data_ptr()      # noqa: E731
        nbs = [L.modet_deconv4s2_ws_bytes(*dims, k) for k in range(3)]
        assert min(nbs) > 0
        ws = [g.ws(nb) for nb in nbs]
        _lib.check(L.modet_deconv4s2_fwd(p(x), p(w), p(b), p(y), p(ws[0]), nbs[0], *dims, act, sl, stream()), "deconv fwd")
        ya = y if act else None
        _lib.check(L.modet_deconv4s2_bwd_data(p(gy), p(ya), p(w), p(dx), p(ws[1]), nbs[1], *dims, act, sl, stream()), "deconv bwd data")
        _lib.check(L.modet_deconv4s2_bwd_weight(p(x), p(gy), p(ya), p(dw), p(db), p(ws[2]), nbs[2], *dims, act, sl, stream()), "deconv bwd weight")
        out = {"y": y, "d_x": dx, "d_w": dw}
        if use_bias:
            out["d_b"] = db
        return out
    return case


def ops_case(n, bias=None):
    """the package's own wrapper under GuardedAlloc: outputs, gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import ops
        Cout, has_bias, slope = orc.OP_CASES[n][3], orc.OP_CASES[n][4], orc.OP_CASES[n][5]
        use_bias = has_bias if bias is None else bias
        x, w, b, gy = orc.case_tensors(n, seed=4000 + n)
        x, w, gy = g(x), g(w), g(gy)
        b = g(b if b is not None else torch.full((Cout,), 0.25)) if use_bias else None
        leaves = [t.requires_grad_(True) for t in ((x, w, b) if use_bias else (x, w))]
        y = ops.conv_transpose3d_k4s2(x, w, b, slope)
        grads = torch.autograd.grad(y, leaves, gy)
        out = {"y": y}
        out.update({"g%d" % i: v for i, v in enumerate(grads)})
        return out
    return case


CASES = {}
for _n in (1, 3, 4, 6):
    CASES["abi[case%d]" % _n] = abi_case(_n)
    CASES["ops[case%d]" % _n] = ops_case(_n)
CASES["abi[case6,no bias]"] = abi_case(6, bias=False)
CASES["abi[case3,bias]"] = abi_case(3, bias=True)
CASES["ops[case1,no bias]"] = ops_case(1, bias=False)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_deconv_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import ops
    px.refuse = True
    x, w, b = torch.rand(1, 2, 3, 4, 8, device="cuda"), torch.rand(8, 16, 4, 4, 4, device="cuda"), torch.rand(16, device="cuda")
    f = ops.conv_transpose3d_k4s2
    for bad in (lambda: f(x.double(), w, b), lambda: f(x[0], w, b), lambda: f(x.cpu(), w, b), lambda: f(x.permute(0, 3, 2, 1, 4), w, b),
                lambda: f(x, w[:4].contiguous(), b), lambda: f(x, w, b[:8].contiguous()), lambda: f(x, w[..., :3].contiguous(), b),
                lambda: f(x, w.permute(1, 0, 2, 3, 4).contiguous(), b), lambda: f(x, w, b, -1.0), lambda: f(x, w, b, "relu"),
                lambda: f(x[:0], w, b), lambda: f(x, w[0], b)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, channel counts outside the kernels', empty axes, a negative slope, a misaligned tensor and a short or misaligned
    workspace are answered with the library's error codes before any launch: the outputs keep their fill"""
    from smilecode_amd import _lib
    L = _lib.load()
    dims = (1, 2, 2, 2, 4, 8)
    x, w, b = torch.zeros(1, 2, 2, 2, 4, device="cuda"), torch.zeros(4, 8, 4, 4, 4, device="cuda"), torch.zeros(8, device="cuda")
    y, gy = torch.full((1, 4, 4, 4, 8), 7.0, device="cuda"), torch.ones(1, 4, 4, 4, 8, device="cuda")
    dx, dw, db = torch.full_like(x, 7.0), torch.full_like(w, 7.0), torch.full_like(b, 7.0)
    P, st = (lambda t: t.data_ptr()), stream()
    NULL, DIM, UNSUP, WS = -1, -2, -3, -4
    nb = [L.modet_deconv4s2_ws_bytes(*dims, k) for k in range(3)]
    assert nb[0] == nb[1] == 64 * 4 * 8 * 4 and nb[2] == 2 * (64 * 4 * 8 + 8) * 4
    assert L.modet_deconv4s2_ws_bytes(*dims, 3) == 0 and L.modet_deconv4s2_ws_bytes(1, 2, 2, 2, 0, 8, 0) == 0
    assert L.modet_deconv4s2_ws_bytes(1, 2, 2, 2, 4, 1025, 0) == 0 and L.modet_deconv4s2_ws_bytes(1, 0, 2, 2, 4, 8, 0) == 0
    assert L.modet_deconv4s2_ws_bytes(1, 512, 512, 512, 4, 8, 0) == 0                      # y of 2^33 elements
    assert L.modet_deconv4s2_ws_bytes(1, 2, 2, 2, 3, 3, 0) == 64 * 4 * 4 * 4               # the padded counts
    ws = torch.empty(max(nb) + 32, dtype=torch.uint8, device="cuda")
    tail = (1, 0.1, st)
    fwd, bd, bw = L.modet_deconv4s2_fwd, L.modet_deconv4s2_bwd_data, L.modet_deconv4s2_bwd_weight
    assert fwd(None, P(w), P(b), P(y), P(ws), nb[0], *dims, *tail) == NULL
    assert fwd(P(x), P(w), P(b), None, P(ws), nb[0], *dims, *tail) == NULL
    assert fwd(P(x), P(w), P(b), P(y), None, nb[0], *dims, *tail) == NULL
    assert fwd(P(x), P(w), P(b), P(y), P(ws), nb[0] - 1, *dims, *tail) == WS
    assert fwd(P(x), P(w), P(b), P(y), P(ws) + 4, nb[0], *dims, *tail) == WS
    assert fwd(P(x) + 4, P(w), P(b), P(y), P(ws), nb[0], *dims, *tail) == UNSUP
    assert fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], 1, 2, 2, 2, 1025, 8, *tail) == UNSUP
    assert fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], 1, 2, 2, 2, 4, 0, *tail) == DIM
    assert fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], 1, 2, 0, 2, 4, 8, *tail) == DIM
    assert fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], *dims, 1, -0.5, st) == UNSUP
    assert fwd(P(x), P(w), P(b), P(y), P(ws), nb[0], *dims, 2, 0.1, st) == UNSUP
    assert bd(P(gy), None, P(w), P(dx), P(ws), nb[1], *dims, *tail) == NULL      # act == 1 needs y
    assert bd(P(gy), P(y), P(w), None, P(ws), nb[1], *dims, *tail) == NULL
    assert bd(P(gy), P(y), P(w), P(dx), P(ws), nb[1] - 4, *dims, *tail) == WS
    assert bw(P(x), P(gy), None, P(dw), P(db), P(ws), nb[2], *dims, *tail) == NULL
    assert bw(P(x), P(gy), P(y), None, P(db), P(ws), nb[2], *dims, *tail) == NULL
    assert bw(P(x), P(gy), P(y), P(dw), P(db), P(ws), nb[2] - 4, *dims, *tail) == WS
    assert bw(P(x), P(gy), P(y), P(dw), P(db), P(ws) + 8, nb[2], *dims, *tail) == WS
    torch.cuda.synchronize()
    for t in (y, dx, dw, db):
        assert bool((t == 7.0).all())                                   # nothing was launched


def test_every_launching_deconv_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- the forward's bias, y
    of both backward entry points (absent without an activation) and the weight gradient's d_b -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_deconv4s2_fwd": ((2,), (0, 1, 3, 4)),                    # x w bias y ws | stream
        "modet_deconv4s2_bwd_data": ((1,), (0, 2, 3, 4)),               # d_y y w d_x ws | stream
        "modet_deconv4s2_bwd_weight": ((2, 4), (0, 1, 3, 5)),           # x d_y y d_w d_b ws | stream
    })
