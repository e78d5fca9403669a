"""-m gpu: WHERE the PCNet family's kernels read and write -- tests/test_gpu_deconv_guard.py's assertions over the family's own table
(_lib.FAMILIES["pcnet"], include/modet_hip_pcnet.h).  Every caller-supplied tensor sits between guard bands (tests/guard.py), every
workspace is exactly modet_pcnet_nff_ws_bytes(..., pass) bytes, outputs and workspaces are poisoned, and the library is reached
through a recording proxy over the new table.  Per case: no band is damaged, every result is finite, the results equal an unguarded
run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits.

The shapes are those of tests/test_gpu_pcnet_ops.py: the upsampling of the smallest field by 8, of 3x5x7 by 2 (840 fine voxels: a
partial workgroup) and a batch of two, into rows of 3, 6 and 9 floats at the first and the last offset; the gated sum with n = 1
and 3 over 630 voxels (a tail of two voxels behind the groups of four); the NFF tail at V = 12 with C = 8, at C = 20 (five of
eight lanes per voxel busy), at C = 64 and at V = 9600 (ten partial rows, the last one short); sums of 4099 and of 3 floats."""
import pytest
import torch

from tests import guard
from tests import pcnet_oracle as orc
from tests.guard_family import DIM, NULL, UNSUP, WS, Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("pcnet")
px = H.fixture()


def _p(t):
    return None if t is None else t.data_ptr()


def up_abi(n, ld, off):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, (d, h, w), f = orc.UP_CASES[n]
        x, gy = orc.up_tensors(n)
        row = torch.zeros(B, f * d, f * h, f * w, ld)
        row[..., off:off + 3] = gy
        x, row = g(x), g(row)
        y, dx = g.empty(row.shape), g.empty(x.shape)
        _lib.check(L.modet_pcnet_upsample_fwd(_p(x), _p(y), B, d, h, w, f, ld, off, stream()), "upsample fwd")
        _lib.check(L.modet_pcnet_upsample_bwd(_p(row), _p(dx), B, d, h, w, f, ld, off, stream()), "upsample bwd")
        return {"y": y[..., off:off + 3], "d_x": dx}
    return case


def dfi_abi(n):
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        x, lg, gy = (g(t) for t in orc.dfi_tensors(n))
        nf, N = orc.DFI_CASES[n][2], gy.numel() // 3
        out, dx, dl = g.empty(gy.shape), g.empty(x.shape), g.empty(x.shape)
        _lib.check(L.modet_pcnet_dfi_gate_fwd(_p(x), _p(lg), _p(out), N, nf, stream()), "dfi fwd")
        _lib.check(L.modet_pcnet_dfi_gate_bwd(_p(x), _p(lg), _p(gy), _p(dx), _p(dl), N, nf, stream()), "dfi bwd")
        return {"out": out, "d_x": dx, "d_logits": dl}
    return case


def nff_abi(n, wants=(True, True, True, True), params=True):
    """the six entry points in the wrapper's order, each workspace exactly as large as its query says"""
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        B, shape, C = orc.NFF_CASES[n]
        V = shape[0] * shape[1] * shape[2]
        t0, t1, t2, lg, W1, W2, gy = (g(t) for t in orc.nff_tensors(n))
        nbs = [L.modet_pcnet_nff_ws_bytes(B, V, C, k) for k in range(3)]
        assert min(nbs) > 0
        ws = [g.ws(nb) for nb in nbs]
        avg, mx, gate, dg, davg, dmx = (g.empty((B, 3 * C)) for _ in range(6))
        arg = g.empty((B, 3 * C), torch.int32)
        out = g.empty(gy.shape)
        s = stream()
        _lib.check(L.modet_pcnet_nff_pool(_p(t0), _p(t1), _p(t2), _p(lg), _p(avg), _p(mx), _p(arg), _p(ws[0]), nbs[0], B, V, C, s), "pool")
        _lib.check(L.modet_pcnet_nff_gate_fwd(_p(avg), _p(mx), _p(W1), _p(W2), _p(gate), B, C, s), "gate fwd")
        _lib.check(L.modet_pcnet_nff_apply_fwd(_p(t0), _p(t1), _p(t2), _p(lg), _p(gate), _p(out), B, V, C, s), "apply fwd")
        _lib.check(L.modet_pcnet_nff_apply_bwd_gate(_p(t0), _p(t1), _p(t2), _p(lg), _p(gy), _p(dg), _p(ws[1]), nbs[1], B, V, C, s), "bwd gate")
        dW1, dW2 = (g.empty(W1.shape), g.empty(W2.shape)) if params else (None, None)
        _lib.check(L.modet_pcnet_nff_gate_bwd(_p(avg), _p(mx), _p(W1), _p(W2), _p(gate), _p(dg), _p(davg), _p(dmx), _p(dW1), _p(dW2),
                                              _p(ws[2]), nbs[2], B, C, s), "gate bwd")
        grads = [g.empty(t.shape) if want else None for t, want in zip((t0, t1, t2, lg), wants)]
        _lib.check(L.modet_pcnet_nff_apply_bwd(_p(t0), _p(t1), _p(t2), _p(lg), _p(gy), _p(gate), _p(davg), _p(dmx), _p(arg),
                                               *(_p(t) for t in grads), B, V, C, s), "apply bwd")
        named = {"avg": avg, "mx": mx, "arg": arg.float(), "g": gate, "out": out, "d_g": dg, "d_avg": davg, "d_mx": dmx}
        named.update({"d%d" % i: t for i, t in enumerate(grads) if t is not None})
        if params:
            named.update({"d_W1": dW1, "d_W2": dW2})
        return named
    return case


def add_abi(n):
    def case(g):
        from smilecode_amd import _lib
        gen = orc.gen(7500 + n)
        a, b = g(torch.randn(n, generator=gen)), g(torch.randn(n, generator=gen))
        s = g.empty((n,))
        _lib.check(_lib.load().modet_pcnet_add(_p(a), _p(b), _p(s), n, stream()), "add")
        return {"s": s}
    return case


def ops_case(which, n):
    """the package's own wrappers under GuardedAlloc: outputs, gradients and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import ops
        if which == "up":
            x, gy = orc.up_tensors(n)
            leaves, y = [g(x).requires_grad_(True)], None
            y = ops.upsample_pow2(leaves[0], orc.UP_CASES[n][2])
        elif which == "dfi":
            x, lg, gy = orc.dfi_tensors(n)
            leaves = [g(x).requires_grad_(True), g(lg).requires_grad_(True)]
            y = ops.dfi_gate(*leaves)
        elif which == "nff":
            *t, gy = orc.nff_tensors(n)
            leaves = [g(v).requires_grad_(True) for v in t]
            y = ops.nff_fuse(*leaves)
        else:
            gen = orc.gen(7600 + n)
            leaves = [g(torch.randn(n, generator=gen)).requires_grad_(True) for _ in range(2)]
            gy = torch.randn(n, generator=gen)
            y = ops.residual_add(*leaves)
        grads = torch.autograd.grad(y, leaves, g(gy))
        out = {"y": y}
        out.update({"g%d" % i: v for i, v in enumerate(grads)})
        return out
    return case


CASES = {}
for _n, _ld, _off in ((3, 3, 0), (5, 3, 0), (6, 6, 3), (1, 9, 0), (4, 9, 6)):
    CASES["abi[up case%d,ld%d,off%d]" % (_n, _ld, _off)] = up_abi(_n, _ld, _off)
for _n in (1, 3):
    CASES["abi[dfi case%d]" % _n] = dfi_abi(_n)
    CASES["ops[dfi case%d]" % _n] = ops_case("dfi", _n)
for _n in (2, 4, 5, 6):
    CASES["abi[nff case%d]" % _n] = nff_abi(_n)
    CASES["ops[nff case%d]" % _n] = ops_case("nff", _n)
CASES["abi[nff case3,logits only]"] = nff_abi(3, wants=(False, False, False, True), params=False)
CASES["abi[nff case3,t1 only]"] = nff_abi(3, wants=(False, True, False, False))
for _n in (3, 5, 6):
    CASES["ops[up case%d]" % _n] = ops_case("up", _n)
for _n in (3, 4099):
    CASES["abi[add %d]" % _n] = add_abi(_n)
    CASES["ops[add %d]" % _n] = ops_case("add", _n)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_pcnet_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import ops
    px.refuse = True
    z = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    x, t, lg, W1, W2 = z(1, 2, 3, 5, 3), z(1, 2, 3, 2, 8), z(1, 2, 3, 2, 3), z(3, 24), z(24, 3)
    for bad in (lambda: ops.upsample_pow2(x, 16), lambda: ops.upsample_pow2(z(1, 2, 1, 5, 3), 2), lambda: ops.upsample_pow2(x.double(), 2),
                lambda: ops.upsample_pow2(x, 2, z(1, 4, 6, 10, 9), 7), lambda: ops.upsample_pow2(x, 2, z(1, 4, 6, 10, 9)[..., :6], 0),
                lambda: ops.upsample_pow2(x.permute(0, 3, 2, 1, 4), 2),
                lambda: ops.dfi_gate(z(4, 12), z(4, 12)), lambda: ops.dfi_gate(z(4, 6), z(4, 3)), lambda: ops.dfi_gate(z(4, 6).cpu(), z(4, 6)),
                lambda: ops.nff_fuse(t, t, t, lg, W2, W1), lambda: ops.nff_fuse(t, t, t[..., :4].contiguous(), lg, W1, W2),
                lambda: ops.nff_fuse(t, t, t, lg[..., :2].contiguous(), W1, W2), lambda: ops.nff_fuse(t[:0], t[:0], t[:0], lg[:0], W1, W2),
                lambda: ops.residual_add(z(4), z(4, 1)), lambda: ops.residual_add(z(4).double(), z(4).double())):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, factors, row widths, offsets, field and channel counts outside the kernels', an axis of 1, misaligned tensors
    and a short or misaligned workspace are answered with the library's error codes before any launch: the outputs keep their fill"""
    from smilecode_amd import _lib
    L, s = _lib.load(), stream()
    f7 = lambda *shape: torch.full(shape, 7.0, device="cuda")          # noqa: E731
    x, y = torch.zeros(1, 2, 3, 5, 3, device="cuda"), f7(1, 4, 6, 10, 9)
    up = lambda **kw: L.modet_pcnet_upsample_fwd(*({**dict(x=_p(x), y=_p(y), B=1, d=2, h=3, w=5, f=2, ld=9, off=3, s=s), **kw}.values()))  # noqa: E731
    assert up() == 0
    assert up(x=None) == NULL and up(y=None) == NULL and up(d=1) == DIM and up(w=1) == DIM and up(B=0) == DIM and up(h=4097) == DIM
    assert up(f=3) == UNSUP and up(f=16) == UNSUP and up(ld=4) == UNSUP and up(off=7) == UNSUP and up(off=-1) == UNSUP
    assert up(B=1 << 20) == DIM                                              # y of 2^31 floats or more
    dx = f7(1, 2, 3, 5, 3)
    assert L.modet_pcnet_upsample_bwd(_p(y), _p(dx), 1, 2, 3, 1, 2, 9, 3, s) == DIM
    assert L.modet_pcnet_upsample_bwd(_p(y), None, 1, 2, 3, 5, 2, 9, 3, s) == NULL
    a, out = torch.zeros(8, 6, device="cuda"), f7(8, 3)
    assert L.modet_pcnet_dfi_gate_fwd(_p(a), _p(a), _p(out), 8, 4, s) == UNSUP and L.modet_pcnet_dfi_gate_fwd(_p(a), _p(a), _p(out), 0, 2, s) == DIM
    assert L.modet_pcnet_dfi_gate_fwd(_p(a) + 4, _p(a), _p(out), 4, 2, s) == UNSUP and L.modet_pcnet_dfi_gate_fwd(_p(a), None, _p(out), 8, 2, s) == NULL
    assert L.modet_pcnet_dfi_gate_bwd(_p(a), _p(a), _p(out), _p(a), None, 8, 2, s) == NULL
    assert L.modet_pcnet_add(_p(a), _p(a) + 4, _p(out), 8, s) == UNSUP and L.modet_pcnet_add(_p(a), _p(a), None, 8, s) == NULL
    assert L.modet_pcnet_add(_p(a), _p(a), _p(out), 0, s) == DIM
    ws_bytes = L.modet_pcnet_nff_ws_bytes
    B, V, C = 2, 9600, 8
    assert ws_bytes(B, V, C, 0) == 2 * 10 * 24 * 16 and ws_bytes(B, V, C, 1) == 2 * 10 * 24 * 8 and ws_bytes(B, V, C, 2) == 2 * (24 + 4 * 3) * 4
    assert ws_bytes(1, 12, 4, 0) == 12 * 16 and ws_bytes(1, 160 * 192 * 160, 16, 1) == 1024 * 48 * 8
    for bad in ((B, V, C, 3), (B, V, 6, 0), (B, V, 0, 0), (B, V, 260, 0), (0, V, C, 0), (65536, V, C, 0), (B, 0, C, 0), (B, 1 << 31, C, 0)):
        assert ws_bytes(*bad) == 0, bad
    t, lg = torch.zeros(B, V, C, device="cuda"), torch.zeros(B, V, 3, device="cuda")
    avg, mx, gate, arg = f7(B, 24), f7(B, 24), f7(B, 24), torch.full((B, 24), 7, dtype=torch.int32, device="cuda")
    W1, W2, out = torch.zeros(3, 24, device="cuda"), torch.zeros(24, 3, device="cuda"), f7(B, V, 24)
    nb = [ws_bytes(B, V, C, k) for k in range(3)]
    ws = torch.empty(max(nb) + 32, dtype=torch.uint8, device="cuda")
    pool = lambda **kw: L.modet_pcnet_nff_pool(*({**dict(t0=_p(t), t1=_p(t), t2=_p(t), lg=_p(lg), avg=_p(avg), mx=_p(mx), arg=_p(arg),  # noqa: E731
                                                        ws=_p(ws), nb=nb[0], B=B, V=V, C=C, s=s), **kw}.values()))
    assert pool(t1=None) == NULL and pool(arg=None) == NULL and pool(ws=None) == NULL and pool(nb=nb[0] - 1) == WS and pool(ws=_p(ws) + 4) == WS
    assert pool(C=12) == WS and pool(C=6) == UNSUP and pool(t2=_p(t) + 4) == UNSUP and pool(V=0) == DIM and pool(B=0) == DIM
    assert L.modet_pcnet_nff_gate_fwd(_p(avg), _p(mx), _p(W1), _p(W2), None, B, C, s) == NULL
    assert L.modet_pcnet_nff_gate_fwd(_p(avg), _p(mx), _p(W1), _p(W2), _p(gate), B, 264, s) == UNSUP
    gb = lambda dW1, dW2, n: L.modet_pcnet_nff_gate_bwd(_p(avg), _p(mx), _p(W1), _p(W2), _p(gate), _p(avg), _p(mx), _p(avg), dW1, dW2,  # noqa: E731
                                                        _p(ws), n, B, C, s)
    assert gb(_p(W1), None, nb[2]) == NULL and gb(None, None, nb[2] - 4) == WS
    assert L.modet_pcnet_nff_apply_fwd(_p(t), _p(t), _p(t), _p(lg), _p(gate), None, B, V, C, s) == NULL
    assert L.modet_pcnet_nff_apply_fwd(_p(t), _p(t), _p(t), _p(lg), _p(gate), _p(out) + 8, B, V, C, s) == UNSUP
    assert L.modet_pcnet_nff_apply_bwd_gate(_p(t), _p(t), _p(t), _p(lg), _p(out), _p(gate), _p(ws), nb[1] - 8, B, V, C, s) == WS
    assert L.modet_pcnet_nff_apply_bwd(_p(t), _p(t), _p(t), _p(lg), _p(out), _p(gate), _p(avg), _p(mx), _p(arg), None, None, None, None,
                                       B, V, C, s) == NULL
    torch.cuda.synchronize()
    for v in (y[..., :3], y[..., 6:], dx, out, avg, mx, gate):
        assert bool((v == 7.0).all())                                       # nothing was launched (but the one valid upsampling)
    assert bool((arg == 7).all())


def test_every_launching_pcnet_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- the gate's parameter
    gradients and the four gradients of the apply backward -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_pcnet_upsample_fwd": ((), (0, 1)),                                        # x y | stream
        "modet_pcnet_upsample_bwd": ((), (0, 1)),                                        # d_y d_x | stream
        "modet_pcnet_dfi_gate_fwd": ((), (0, 1, 2)),                                     # x logits out | stream
        "modet_pcnet_dfi_gate_bwd": ((), (0, 1, 2, 3, 4)),                               # x logits d_out d_x d_logits | stream
        "modet_pcnet_nff_pool": ((), (0, 1, 2, 3, 4, 5, 6, 7)),                          # t0 t1 t2 logits avg mx arg ws | stream
        "modet_pcnet_nff_gate_fwd": ((), (0, 1, 2, 3, 4)),                               # avg mx W1 W2 g | stream
        "modet_pcnet_nff_gate_bwd": ((8, 9), (0, 1, 2, 3, 4, 5, 6, 7, 10)),              # ... d_g d_avg d_mx d_W1 d_W2 ws | stream
        "modet_pcnet_nff_apply_fwd": ((), (0, 1, 2, 3, 4, 5)),                           # t0 t1 t2 logits g out | stream
        "modet_pcnet_nff_apply_bwd_gate": ((), (0, 1, 2, 3, 4, 5, 6)),                   # t0 t1 t2 logits d_out d_g ws | stream
        "modet_pcnet_nff_apply_bwd": ((9, 10, 11, 12), (0, 1, 2, 3, 4, 5, 6, 7, 8)),     # ... arg d_t0 d_t1 d_t2 d_logits | stream
        "modet_pcnet_add": ((), (0, 1, 2)),                                              # a b s | stream
    })
