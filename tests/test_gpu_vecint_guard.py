"""-m gpu: WHERE the velocity-integration kernels read and write -- tests/test_gpu_reg_guard.py's assertions over the family's own
table (_lib.FAMILIES["vecint"], include/modet_hip_vecint.h).  Every caller-supplied tensor sits between guard bands
(tests/guard.py), workspaces are exactly modet_vecint_ws_bytes(...) bytes, outputs, step buffers, scratch fields and workspaces
are poisoned, and the library is reached through a recording proxy over the new table.  Per case: no band is damaged, every
result is finite, the results equal an unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and
poison gives the same bits.  Samples leave the volume in every case with amp > 1 (by many voxels at amp 12); the shapes have every
voxel on the border (5 x 6 x 7), a row longer than a wave (4 x 5 x 67) and partial 4 x 4 x 16 tiles along every axis.  Fields with
entries of 1e30 and a NaN voxel, and a broken bound promise, assert intact bands only."""
import pytest
import torch

from tests import guard
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("vecint")
px = H.fixture()


def _field(shape, B, amp, spoil=False):
    gen = torch.Generator().manual_seed(33)
    f = torch.randn((B,) + tuple(shape) + (3,), generator=gen) * amp
    if spoil:                                           # entries of +-1e30 and one NaN voxel
        flat = f.view(-1, 3)
        flat[1] = 1e30
        flat[flat.shape[0] // 2, 1] = -1e30
        flat[flat.shape[0] // 3] = float("nan")
    return f


def abi_case(shape, B, nsteps, bound, amp, spoil=False):
    """the C ABI directly, exact workspace: the forward in both forms, then the backward on the saved steps"""
    def case(g):
        from smilecode_amd import _lib
        L, gen = _lib.load(), torch.Generator().manual_seed(31)
        D, H, W = shape
        vec = g(_field(shape, B, amp, spoil))
        d_out = g(torch.randn(vec.shape, generator=gen))
        nb = L.modet_vecint_ws_bytes(B, D, H, W, nsteps, bound)
        general = any(not (bound > 0 and bound * 2.0 ** (k - nsteps) <= 1.0) for k in range(nsteps))
        assert (nb > 0) == general
        out_a, out_b, d_vec = g.empty(vec.shape), g.empty(vec.shape), g.empty(vec.shape)
        steps = g.empty((nsteps - 1,) + tuple(vec.shape)) if nsteps >= 2 else None
        scr_f = g.empty(vec.shape) if nsteps >= 2 else None
        scr_b = g.empty(vec.shape) if nsteps >= 2 else None
        ws = g.ws(nb) if nb else None
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        _lib.check(L.modet_vecint_fwd(p(vec), p(out_a), p(steps), None, B, D, H, W, nsteps, stream()), "vecint fwd (steps)")
        _lib.check(L.modet_vecint_fwd(p(vec), p(out_b), None, p(scr_f), B, D, H, W, nsteps, stream()), "vecint fwd (scratch)")
        _lib.check(L.modet_vecint_bwd(p(vec), p(steps), p(d_out), p(d_vec), p(scr_b), p(ws), nb, B, D, H, W, nsteps, bound, stream()),
                   "vecint bwd")
        return {"out": out_a, "out_inference": out_b, "d_vec": d_vec}
    return case


def ops_case(shape, B, nsteps, bound, amp, spoil=False):
    """the package's own wrappers under GuardedAlloc: outputs, saved steps, scratch fields and workspaces are guarded allocations"""
    def case(g):
        from smilecode_amd import models, ops
        gen = torch.Generator().manual_seed(32)
        vec = g(_field(shape, B, amp, spoil)).requires_grad_(True)
        cot = g(torch.randn(vec.shape, generator=gen))
        out = ops.vecint(vec, nsteps, bound)
        (d_vec,) = torch.autograd.grad(out, [vec], cot)
        with torch.no_grad():
            inf = ops.vecint(vec.detach(), nsteps, bound)
            planar = models.VecInt(shape, nsteps)(g(vec.detach().permute(0, 4, 1, 2, 3).contiguous()))
        return {"out": out, "d_vec": d_vec, "out_inference": inf, "out_planar": planar}
    return case


# tag -> (case, finite): ``finite`` cases carry the four assertions, the others intact bands only
CASES = {}
for _shape, _B in (((5, 6, 7), 2), ((4, 5, 67), 1), ((9, 13, 35), 2)):
    for _n, _bound, _amp in ((7, 1.0, 1.0), (7, 0.0, 2.0), (7, 8.0, 8.0), (3, 0.0, 12.0), (1, 1.0, 1.0), (1, 0.0, 3.0), (2, 2.0, 2.0)):
        _f = _field(_shape, _B, 1.0)
        _a = _amp if _bound == 0.0 else _bound / float(_f.abs().max()) * 0.999        # the promise max |vec| <= bound is kept
        CASES["abi[%dx%dx%d,B%d,n%d,bound%g]" % (_shape + (_B, _n, _bound))] = (abi_case(_shape, _B, _n, _bound, _a), True)
CASES["abi[6x6x6,n0]"] = (abi_case((6, 6, 6), 1, 0, 0.0, 2.0), True)
CASES["ops[9x13x35,B2,n7,bound1]"] = (ops_case((9, 13, 35), 2, 7, 1.0, 1.0 / 6.0), True)
CASES["ops[5x6x7,n3,bound0]"] = (ops_case((5, 6, 7), 1, 3, 0.0, 4.0), True)
CASES["ops[4x5x67,n7,bound8]"] = (ops_case((4, 5, 67), 1, 7, 8.0, 1.0), True)
for _bound in (1.0, 0.0, 64.0):
    CASES["abi[nonfinite,6x7x9,n3,bound%g]" % _bound] = (abi_case((6, 7, 9), 1, 3, _bound, 2.0, spoil=True), False)
    CASES["ops[nonfinite,9x13x35,n7,bound%g]" % _bound] = (ops_case((9, 13, 35), 1, 7, _bound, 2.0, spoil=True), False)
CASES["abi[broken promise,6x7x9,n3,bound1,amp12]"] = (abi_case((6, 7, 9), 1, 3, 1.0, 12.0), False)
CASES["ops[broken promise,9x13x35,B2,n7,bound1,amp12]"] = (ops_case((9, 13, 35), 2, 7, 1.0, 12.0), False)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_vecint_between_guard_bands(px, tag):
    case, finite = CASES[tag]
    if finite:
        H.run_guarded(case, px, tag)
    else:
        H.run(case, 0xFF, px)          # memory-safe whatever the values are: intact bands (asserted inside), nothing about the results
    H.ran.add(tag)


def test_entry_points_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import models, ops
    px.refuse = True
    v = torch.rand(1, 9, 9, 9, 3, device="cuda")
    for bad in (lambda: ops.vecint(v.double()), lambda: ops.vecint(v.half()), lambda: ops.vecint(v[0]), lambda: ops.vecint(v[..., :2].contiguous()),
                lambda: ops.vecint(v.permute(0, 3, 2, 1, 4)), lambda: ops.vecint(v[:, ::2]), lambda: ops.vecint(v, -1), lambda: ops.vecint(v, 13),
                lambda: ops.vecint(v, 2.0), lambda: ops.vecint(v, True), lambda: ops.vecint(v, 7, -1.0), lambda: ops.vecint(v, 7, float("nan")),
                lambda: ops.vecint(v, 7, float("inf")), lambda: ops.vecint(v[:0]), lambda: ops.vecint(v.cpu()),
                lambda: models.VecInt((9, 9, 9), 13), lambda: models.VecInt((9, 9, 9))(v)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, nsteps outside 0..12, a negative or non-finite bound, 2^31 elements and a short or misaligned workspace are
    answered with the library's error codes before any launch (the pointers below are never dereferenced)"""
    from smilecode_amd import _lib
    L = _lib.load()
    v = torch.zeros(1, 4, 4, 4, 3, device="cuda")
    o, s, d = torch.full_like(v, 7.0), torch.full_like(v, 7.0), torch.full_like(v, 7.0)
    P, st = (lambda t: t.data_ptr()), stream()
    NULL, DIM, WS = -1, -2, -4
    codes = {L.modet_hip_strerror(c).decode(): c for c in (NULL, DIM, WS)}
    assert codes == {"required pointer is NULL": NULL, "invalid or inconsistent dimensions": DIM,
                     "workspace too small (see *_ws_bytes)": WS}
    assert L.modet_vecint_fwd(None, P(o), None, P(s), 1, 4, 4, 4, 2, st) == NULL
    assert L.modet_vecint_fwd(P(v), None, None, P(s), 1, 4, 4, 4, 2, st) == NULL
    assert L.modet_vecint_fwd(P(v), P(o), None, None, 1, 4, 4, 4, 2, st) == NULL          # two steps need steps or scratch
    assert L.modet_vecint_fwd(P(v), P(o), None, P(s), 1, 4, 4, 4, 13, st) == DIM
    assert L.modet_vecint_fwd(P(v), P(o), None, P(s), 1, 4, 4, 4, -1, st) == DIM
    assert L.modet_vecint_fwd(P(v), P(o), None, P(s), 0, 4, 4, 4, 2, st) == DIM
    assert L.modet_vecint_fwd(P(v), P(o), None, P(s), 1, 1024, 1024, 1024, 2, st) == DIM   # 3 * 2^30 elements
    nb = L.modet_vecint_ws_bytes(1, 4, 4, 4, 2, 0.0)
    assert nb > 0
    ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    args = (1, 4, 4, 4, 2)
    assert L.modet_vecint_bwd(None, P(s), P(o), P(d), P(s), P(ws), nb, *args, 0.0, st) == NULL
    assert L.modet_vecint_bwd(P(v), None, P(o), P(d), P(s), P(ws), nb, *args, 0.0, st) == NULL
    assert L.modet_vecint_bwd(P(v), P(s), None, P(d), P(s), P(ws), nb, *args, 0.0, st) == NULL
    assert L.modet_vecint_bwd(P(v), P(s), P(o), None, P(s), P(ws), nb, *args, 0.0, st) == NULL
    assert L.modet_vecint_bwd(P(v), P(s), P(o), P(d), None, P(ws), nb, *args, 0.0, st) == NULL
    assert L.modet_vecint_bwd(P(v), P(s), P(o), P(d), P(s), None, nb, *args, 0.0, st) == NULL
    assert L.modet_vecint_bwd(P(v), P(s), P(o), P(d), P(s), P(ws), nb - 1, *args, 0.0, st) == WS
    assert L.modet_vecint_bwd(P(v), P(s), P(o), P(d), P(s), P(ws) + 4, nb, *args, 0.0, st) == WS
    for bound in (-1.0, float("nan"), float("inf")):
        assert L.modet_vecint_bwd(P(v), P(s), P(o), P(d), P(s), P(ws), nb, *args, bound, st) == DIM
    assert L.modet_vecint_bwd(P(v), P(s), P(o), P(d), P(s), P(ws), nb, 1, 4, 4, 4, 13, 0.0, st) == DIM
    torch.cuda.synchronize()
    assert bool((d == 7.0).all()) and bool((o == 7.0).all()) and bool((s == 7.0).all())       # nothing was launched


def test_every_launching_vecint_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table: every launching name of _lib.FAMILIES["vecint"]
    was called at least once with every device pointer inside a guarded buffer, and no case handed the library a device pointer
    outside one.  Cases deselected from this session are run here, guarded once."""
    # forward (vec, out, steps, scratch, stream): both forms were seen; backward (vec, steps, d_out, d_vec, scratch, ws, stream):
    # with and without a workspace
    H.check_coverage(px, {tag: c[0] for tag, c in CASES.items()}, {"modet_vecint_fwd": ((), (0, 1)), "modet_vecint_bwd": ((5,), (0, 2, 3))})
    fwd = [cs for m, cs in H.seen if m == "modet_vecint_fwd"]
    assert {(cs[2], cs[3]) for cs in fwd} >= {("guarded", "null"), ("null", "guarded"), ("null", "null")}
