"""-m gpu: WHERE the positional-encoding kernels read and write -- tests/test_gpu_vecint_guard.py's assertions over the family's own
table (_lib.FAMILIES["posenc"], include/modet_hip_posenc.h).  Every caller-supplied tensor sits between guard bands
(tests/guard.py), the workspace is exactly modet_posenc_ws_bytes(...) bytes, outputs and workspace are poisoned, and the library is
reached through a recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an
unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.  The shapes:
the five of the parity test (every lane-group width, odd sizes, one or several partial workgroups), axes of 2, and one volume
larger than a whole grid pass of both grid caps."""
import pytest
import torch

from tests import guard
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("posenc")
px = H.fixture()


def _inputs(B, shape, Cin, seed=71):
    gen = torch.Generator().manual_seed(seed + Cin)
    n = (B,) + tuple(shape)
    return {"x1": torch.randn(n + (Cin,), generator=gen), "x2": torch.randn(n + (Cin,), generator=gen),
            "gy1": torch.randn(n + (6,), generator=gen), "gy2": torch.randn(n + (6,), generator=gen),
            "Wt": torch.randn(6, Cin, generator=gen) / Cin ** 0.5, "b": torch.randn(6, generator=gen), "alpha": torch.tensor([0.7])}


def abi_case(B, shape, Cin, uses=2, want=(True, True)):
    """the C ABI directly, exact workspace: forward, data gradients (``want``: which of d_x1, d_x2), parameter gradients"""
    def case(g):
        from smilecode_amd import _lib, ops
        L, D_, H_, W_ = _lib.load(), *shape
        t = {k: g(v) for k, v in _inputs(B, shape, Cin).items()}
        tab = g(ops.posenc_table(D_, H_, W_))
        dims = (B, D_, H_, W_, Cin, 6)
        two = uses == 2
        y1, y2 = g.empty(t["gy1"].shape), (g.empty(t["gy1"].shape) if two else None)
        dx1 = g.empty(t["x1"].shape) if want[0] else None
        dx2 = g.empty(t["x1"].shape) if (two and want[1]) else None
        dW, db, da = g.empty((6, Cin)), g.empty((6,)), g.empty((1,))
        nb = L.modet_posenc_ws_bytes(*dims)
        assert nb > 0
        ws = g.ws(nb)
        p = lambda v: None if v is None else v.data_ptr()      # noqa: E731
        x2, gy2 = (t["x2"], t["gy2"]) if two else (None, None)
        _lib.check(L.modet_posenc_fwd_pair(p(t["x1"]), p(x2), p(t["Wt"]), p(t["b"]), p(t["alpha"]), p(tab), p(y1), p(y2), *dims, stream()),
                   "posenc fwd")
        _lib.check(L.modet_posenc_bwd_data_pair(p(t["gy1"]) if dx1 is not None else None, p(gy2) if dx2 is not None else None, p(t["Wt"]),
                                                p(dx1), p(dx2), *dims, stream()), "posenc bwd data")
        _lib.check(L.modet_posenc_bwd_params_pair(p(t["x1"]), p(t["gy1"]), p(x2), p(gy2), p(tab), p(dW), p(db), p(da), p(ws), nb, *dims,
                                                  stream()), "posenc bwd params")
        out = {"y1": y1, "d_W": dW, "d_b": db, "d_alpha": da}
        out.update({k: v for k, v in (("y2", y2), ("d_x1", dx1), ("d_x2", dx2)) if v is not None})
        return out
    return case


def ops_case(B, shape, Cin, pair=True):
    """the package's own wrappers under GuardedAlloc: outputs, gradients and the workspace are guarded allocations"""
    def case(g):
        from smilecode_amd import ops
        t = {k: g(v) for k, v in _inputs(B, shape, Cin, seed=72).items()}
        tab = g(ops.posenc_table(*shape))
        leaves = [t[n].requires_grad_(True) for n in (("x1", "x2") if pair else ("x1",)) + ("Wt", "b", "alpha")]
        if pair:
            ys = ops.posenc_pair(t["x1"], t["x2"], t["Wt"], t["b"], t["alpha"], tab)
            grads = torch.autograd.grad(list(ys), leaves, [t["gy1"], t["gy2"]])
        else:
            ys = (ops.posenc(t["x1"], t["Wt"], t["b"], t["alpha"], tab),)
            grads = torch.autograd.grad(list(ys), leaves, [t["gy1"]])
        out = {"y%d" % i: y for i, y in enumerate(ys)}
        out.update({"g%d" % i: v for i, v in enumerate(grads)})
        return out
    return case


SHAPES = ((2, (2, 3, 5), 8), (1, (7, 6, 19), 16), (1, (3, 5, 17), 32), (2, (4, 7, 9), 64), (1, (2, 3, 4), 128), (1, (2, 2, 2), 4),
          (3, (5, 2, 33), 20))
CASES = {}
for _B, _shape, _cin in SHAPES:
    _t = "%dx%dx%d,B%d,c%d" % (_shape + (_B, _cin))
    CASES["abi[%s]" % _t] = abi_case(_B, _shape, _cin)
    CASES["ops[%s,pair]" % _t] = ops_case(_B, _shape, _cin)
CASES["abi[7x6x19,c16,single]"] = abi_case(1, (7, 6, 19), 16, uses=1)
CASES["abi[4x7x9,c64,d_x1 only]"] = abi_case(2, (4, 7, 9), 64, want=(True, False))
CASES["abi[3x5x17,c32,d_x2 only]"] = abi_case(1, (3, 5, 17), 32, want=(False, True))
CASES["ops[3x5x17,c32,single]"] = ops_case(1, (3, 5, 17), 32, pair=False)
CASES["abi[64x96x96,c8,more than a grid pass]"] = abi_case(1, (64, 96, 96), 8)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_posenc_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import models, ops
    px.refuse = True
    x, W, b, al = torch.rand(1, 4, 5, 6, 8, device="cuda"), torch.rand(6, 8, device="cuda"), torch.rand(6, device="cuda"), torch.ones(1, device="cuda")
    tab = ops.posenc_table(4, 5, 6, device="cuda")
    for bad in (lambda: ops.posenc(x.double(), W, b, al, tab), lambda: ops.posenc(x.bfloat16(), W, b, al, tab), lambda: ops.posenc(x[0], W, b, al, tab),
                lambda: ops.posenc(x.cpu(), W, b, al, tab), lambda: ops.posenc(x.permute(0, 3, 2, 1, 4), W, b, al, tab),
                lambda: ops.posenc(x, W, b, al, tab[:-1]), lambda: ops.posenc(x, W, b, al.double(), tab), lambda: ops.posenc(x[:, :1].contiguous(), W, b, al, tab),
                lambda: ops.posenc_pair(x, x[:, :2].contiguous(), W, b, al, tab), lambda: ops.posenc(x, torch.rand(12, 8, device="cuda"), b, al, tab),
                lambda: ops.posenc(x[..., :6].contiguous(), W[:, :6].contiguous(), b, al, tab), lambda: ops.posenc(x[:0], W, b, al, tab),
                lambda: models.PositionalEncodingLayer(8, dim=3), lambda: models.Im2grid((32, 32, 24)),
                lambda: models.Im2grid((32, 32, 32)).cuda()(x, x)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, another width, axes below 2 and a short or misaligned workspace are answered with the library's error codes
    before any launch: the outputs keep their fill"""
    from smilecode_amd import _lib, ops
    L = _lib.load()
    dims = (1, 4, 4, 4, 8, 6)
    x, W, b, al = torch.zeros(1, 4, 4, 4, 8, device="cuda"), torch.zeros(6, 8, device="cuda"), torch.zeros(6, device="cuda"), torch.ones(1, device="cuda")
    tab = ops.posenc_table(4, 4, 4, device="cuda")
    y, gy, dx = torch.full((1, 4, 4, 4, 6), 7.0, device="cuda"), torch.ones(1, 4, 4, 4, 6, device="cuda"), torch.full_like(x, 7.0)
    dW, db, da = torch.full_like(W, 7.0), torch.full_like(b, 7.0), torch.full_like(al, 7.0)
    P, st = (lambda t: t.data_ptr()), stream()
    NULL, DIM, UNSUP, WS = -1, -2, -3, -4
    assert L.modet_posenc_fwd_pair(P(x), None, P(W), P(b), P(al), P(tab), None, None, *dims, st) == NULL
    assert L.modet_posenc_fwd_pair(P(x), P(x), P(W), P(b), P(al), P(tab), P(y), None, *dims, st) == NULL
    assert L.modet_posenc_fwd_pair(P(x), None, P(W), P(b), None, P(tab), P(y), None, *dims, st) == NULL
    assert L.modet_posenc_fwd_pair(P(x), None, P(W), P(b), P(al), P(tab), P(y), None, 1, 4, 4, 4, 8, 12, st) == UNSUP
    assert L.modet_posenc_fwd_pair(P(x), None, P(W), P(b), P(al), P(tab), P(y), None, 1, 4, 1, 4, 8, 6, st) == DIM
    assert L.modet_posenc_bwd_data_pair(P(gy), None, P(W), None, None, *dims, st) == NULL
    assert L.modet_posenc_bwd_data_pair(None, None, P(W), P(dx), None, *dims, st) == NULL
    assert L.modet_posenc_bwd_data_pair(P(gy), None, P(W), P(dx), None, 1, 4, 4, 4, 6, 6, st) == UNSUP
    nb = L.modet_posenc_ws_bytes(*dims)
    ws = torch.empty(nb + 32, dtype=torch.uint8, device="cuda")
    args = (P(x), P(gy), None, None, P(tab), P(dW), P(db), P(da))
    assert L.modet_posenc_bwd_params_pair(*args, P(ws), nb - 1, *dims, st) == WS
    assert L.modet_posenc_bwd_params_pair(*args, P(ws) + 4, nb, *dims, st) == WS
    assert L.modet_posenc_bwd_params_pair(*args, None, nb, *dims, st) == NULL
    assert L.modet_posenc_bwd_params_pair(P(x), P(gy), P(x), None, P(tab), P(dW), P(db), P(da), P(ws), nb, *dims, st) == NULL
    assert L.modet_posenc_bwd_params_pair(*args, P(ws), nb, 1, 4, 4, 1, 8, 6, st) == DIM
    torch.cuda.synchronize()
    for t in (y, dx, dW, db, da):
        assert bool((t == 7.0).all())                                   # nothing was launched


def test_every_launching_posenc_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- x2 and y2 of the
    forward, d_x1 and d_x2 of the data backward, x2 and d_y2 of the parameter backward -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_posenc_fwd_pair": ((1, 7), (0, 2, 3, 4, 5, 6)),                  # x1 x2 Wt bias alpha tab y1 y2 | stream
        "modet_posenc_bwd_data_pair": ((3, 4), (2,)),                           # d_y1 d_y2 Wt d_x1 d_x2 | stream
        "modet_posenc_bwd_params_pair": ((2, 3), (0, 1, 4, 5, 6, 7, 8)),        # x1 d_y1 x2 d_y2 tab d_Wt d_bias d_alpha ws | stream
    })
