"""-m gpu: WHERE the surface-distance kernels read and write -- tests/test_gpu_vecint_guard.py's assertions over the family's own
table (_lib.FAMILIES["surface"], include/modet_hip_surface.h).  Both label maps, both result tables and the workspace sit
between guard bands (tests/guard.py), the workspace is exactly modet_surface_ws_bytes(...) bytes, results and workspace are
poisoned, and the library is reached through a recording proxy over the new table.  Per case: no band is damaged, the results
equal an unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same bits
(the metrics are compared as their int64 bit patterns: a label missing on one side is NaN by contract).  Maps filled with 32767 or
-32768 assert intact bands only."""
import numpy as np
import pytest
import torch

from tests import guard
from tests import surface_oracle as so
from tests.guard_family import Harness, stream

pytestmark = pytest.mark.gpu

H = Harness("surface")
px = H.fixture()


def _maps(tag):
    if tag in so.VORONOI:
        shape, nl, seed = so.VORONOI[tag]
        return so.voronoi_pair(shape, nl, seed) + (nl,)
    return so.constructed()[tag]


def abi_case(maps, q=95.0):
    """the C ABI directly, exact workspace"""
    def case(g):
        from smilecode_amd import _lib
        L = _lib.load()
        a_np, b_np, nl = maps() if callable(maps) else _maps(maps)
        D, Hh, W = a_np.shape
        a, b = g(torch.from_numpy(np.ascontiguousarray(a_np))), g(torch.from_numpy(np.ascontiguousarray(b_np)))
        nb = L.modet_surface_ws_bytes(D, Hh, W, nl)
        assert nb > 0
        metrics, counts, ws = g.empty((nl, 5), torch.float64), g.empty((nl, 7), torch.int64), g.ws(nb)
        _lib.check(L.modet_surface_distances(a.data_ptr(), b.data_ptr(), metrics.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb,
                                             D, Hh, W, nl, q, stream()), "surface distances")
        return {"metrics_bits": metrics.view(torch.int64), "counts": counts}
    return case


def ops_case(tag, q=95.0):
    """the package's own wrapper under GuardedAlloc: result tables and workspace are guarded allocations"""
    def case(g):
        from smilecode_amd import ops
        a_np, b_np, nl = _maps(tag)
        metrics, counts = ops.surface_distances(g(torch.from_numpy(a_np)), g(torch.from_numpy(b_np)), nl, q)
        return {"metrics_bits": metrics.view(torch.int64), "counts": counts}
    return case


def _filled(value, shape=(6, 7, 20), nl=54):
    return lambda: (np.full(shape, value, np.int16), np.full(shape, value, np.int16), nl)


# tag -> (case, compared): ``compared`` cases carry the bit comparisons, the others intact bands only
CASES = {}
for _tag in sorted(so.VORONOI):
    CASES["abi[%s]" % _tag] = (abi_case(_tag), True)
for _tag in ("one label fills the volume", "opposite corners", "label 2 in A only, label 3 in B only", "values outside 1..nlabels",
             "nlabels=54, most absent", "two border voxels in all"):
    CASES["abi[%s]" % _tag] = (abi_case(_tag), True)
CASES["abi[9x13x35,q0]"] = (abi_case("9x13x35", 0.0), True)
CASES["abi[9x13x35,q100]"] = (abi_case("9x13x35", 100.0), True)
CASES["abi[lds table]"] = (abi_case(so.labels_above_the_lds_table), True)
for _tag in ("5x6x7", "3x4x300", "9x13x35", "label 2 in A only, label 3 in B only"):
    CASES["ops[%s]" % _tag] = (ops_case(_tag), True)
CASES["abi[filled 32767,nlabels 54]"] = (abi_case(_filled(32767)), False)
CASES["abi[filled -32768,nlabels 54]"] = (abi_case(_filled(-32768)), False)
CASES["abi[filled 32767,nlabels 32767]"] = (abi_case(_filled(32767, (3, 4, 5), 32767)), False)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_surface_between_guard_bands(px, tag):
    case, compared = CASES[tag]
    if compared:
        H.run_guarded(case, px, tag)
    else:
        H.run(case, 0xFF, px)          # intact bands (asserted inside), nothing about the results
    H.ran.add(tag)


def test_entry_points_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import ops, utils
    px.refuse = True
    a = torch.ones(4, 5, 6, dtype=torch.int16, device="cuda")
    sd = ops.surface_distances
    for bad in (lambda: sd(a.int(), a), lambda: sd(a, a.float()), lambda: sd(a[0], a[0]), lambda: sd(a[None], a[None]),
                lambda: sd(a, a[:, :, :5].contiguous()), lambda: sd(a, a.permute(2, 1, 0)), lambda: sd(a[:, ::2], a[:, ::2]),
                lambda: sd(a.cpu(), a), lambda: sd(a, a.cpu()), lambda: sd(a[:0], a[:0]), lambda: sd(a, a, 0), lambda: sd(a, a, 32768),
                lambda: sd(a, a, 54.0), lambda: sd(a, a, 54, -1.0), lambda: sd(a, a, 54, 101.0), lambda: sd(a, a, 54, float("nan")),
                lambda: utils.hd95_val(a, a, 1, voxelspacing=(1, 1, 2)), lambda: utils.assd_val(a, a, 1, connectivity=3),
                lambda: utils.hd_val(a[0], a[0], 1), lambda: utils.surface_val_VOI(torch.stack((a, a))[:, None], torch.stack((a, a))[:, None])):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, dimensions of 0 or 513, nlabels of 0, a percentile of -1, 101 or NaN and a short or misaligned workspace
    are answered with the library's error codes before any launch (the pointers below are never dereferenced)"""
    from smilecode_amd import _lib
    L = _lib.load()
    D, Hh, W, nl = 4, 5, 6, 3
    a = torch.ones(D, Hh, W, dtype=torch.int16, device="cuda")
    b = a.clone()
    m = torch.full((nl, 5), 7.0, dtype=torch.float64, device="cuda")
    c = torch.full((nl, 7), 7, dtype=torch.int64, device="cuda")
    nb = L.modet_surface_ws_bytes(D, Hh, W, nl)
    assert nb > 0
    ws = torch.full((nb + 64,), 7, dtype=torch.uint8, device="cuda")
    P, st = (lambda t: t.data_ptr()), stream()
    NULL, DIM, WS = -1, -2, -4
    codes = {L.modet_hip_strerror(k).decode(): k for k in (NULL, DIM, WS)}
    assert codes == {"required pointer is NULL": NULL, "invalid or inconsistent dimensions": DIM,
                     "workspace too small (see *_ws_bytes)": WS}
    f = L.modet_surface_distances
    good = [P(a), P(b), P(m), P(c), P(ws), nb, D, Hh, W, nl, 95.0, st]
    for at in range(5):
        args = list(good)
        args[at] = None
        assert f(*args) == NULL, at
    for at, v in ((6, 0), (7, 0), (8, 0), (6, 513), (7, 513), (8, 513), (6, -1), (9, 0), (9, -1), (9, 32768), (10, -1.0), (10, 101.0),
                  (10, float("nan")), (10, float("inf"))):
        args = list(good)
        args[at] = v
        assert f(*args) == DIM, (at, v)
    args = list(good); args[5] = nb - 1
    assert f(*args) == WS
    args = list(good); args[5] = 0
    assert f(*args) == WS
    for off in (2, 4, 8):
        args = list(good); args[4] = P(ws) + off
        assert f(*args) == WS, off
    torch.cuda.synchronize()
    assert bool((m == 7.0).all()) and bool((c == 7).all()) and bool((ws == 7).all())       # nothing was launched


def test_every_launching_surface_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table: the one launching name of
    _lib.FAMILIES["surface"] was called with every device pointer (both maps, both tables, the workspace) inside a guarded buffer,
    and no case handed the library a device pointer outside one.  Cases deselected from this session are run here, guarded once."""
    H.check_coverage(px, {tag: c[0] for tag, c in CASES.items()}, {"modet_surface_distances": ((), (0, 1, 2, 3, 4))})
