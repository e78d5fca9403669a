"""NCC without a GPU: the separable restatement of tests/ncc_oracle.py against the dense oracle (oracle/modet_torch.py) and the
reference's recorded results, and its restatement of csrc/losses.hip's z-chunk plan against the library and against the chunking
the cases of tests/test_gpu_ncc_grad3d.py are meant to reach.  The GPU file takes the fp64 reference of its two largest volumes
from the restatement; this file is what entitles it to."""
import numpy as np
import pytest
import torch

from oracle import modet_torch as orc
from tests import ncc_oracle
from tests.util import gold

WINDOWS = (9, 5, 3, [4, 4, 4], [5, 3, 7], [2, 6, 3], [11, 11, 11])


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _volumes(tag):
    if tag == "4x5x6":
        return ncc_oracle.noise_pair((4, 5, 6), 1)
    if tag == "13x27x35":
        g = gold("op_eval.npz")
        return T(g["nccw5.a"]), T(g["nccw5.b"])
    g = gold("op_ncc_windows.npz")
    return T(g["ncc[4x4x4].a"]), T(g["ncc[4x4x4].b"])


@pytest.mark.parametrize("tag", ["4x5x6", "13x27x35", "14x22x19_B2"])
def test_separable_restatement_equals_the_dense_oracle_in_fp64(tag):
    """three 1-D box sums against one dense conv3d: the same sums in another order, so in fp64 the value agrees to 1e-12 relative
    and both gradients to 1e-12 of their largest entry, for cubic, even, anisotropic and over-long windows on volumes shorter
    than the window, ragged, and of batch 2"""
    a, b = _volumes(tag)
    assert tuple(a.shape[2:]) == tuple(int(v) for v in tag.split("_")[0].split("x")) and a.shape[0] == (2 if tag.endswith("B2") else 1)
    for w in WINDOWS:
        want = ncc_oracle.value_and_grads(orc.ncc_loss, a, b, torch.float64, win=w)
        got = ncc_oracle.value_and_grads(ncc_oracle.ncc_loss, a, b, torch.float64, win=w)
        assert float(want[0]) != 0.0 and abs(float(got[0]) - float(want[0])) <= 1e-12 * abs(float(want[0])), (tag, w)
        for g, r in zip(got[1:], want[1:]):
            assert g.shape == r.shape == a.shape and float(r.abs().max()) > 0.0
            assert float((g - r).abs().max()) <= 1e-12 * float(r.abs().max()), (tag, w)


def _stored(g, key):
    """a stored result and the relative precision of its storage"""
    v = g[key]
    assert v.dtype in (np.float64, np.float32), key
    return T(v), (1e-12 if v.dtype == np.float64 else 2.0 ** -23)


def test_separable_restatement_equals_the_reference_goldens():
    """... and what the reference's own NCC_vxm returned (tests/golden/make_goldens*.py), to the precision the files store"""
    misc, ev, wins = gold("op_misc.npz"), gold("op_eval.npz"), gold("op_ncc_windows.npz")
    cases = [(misc, "ncc", 9, ("da", "db")), (ev, "ncc1", 9, ("da",))]
    cases += [(ev, f"nccw{w}", w, ("da", "db")) for w in (3, 5, 7)]
    tags = [k[:-2] for k in wins.files if k.endswith(".a")]
    assert len(tags) == 7
    cases += [(wins, t, [int(v) for v in t[4:-1].split("x")], ("da", "db")) for t in tags]
    for g, key, w, grads in cases:
        a, b = T(g[key + ".a"]), T(g[key + ".b"])
        loss, da, db = ncc_oracle.value_and_grads(ncc_oracle.ncc_loss, a, b, torch.float64, win=w)
        want, tol = _stored(g, key + ".val")
        assert abs(float(loss) - float(want)) <= tol * abs(float(want)), key
        for name, got in (("da", da), ("db", db)):
            if name in grads:
                ref, tol = _stored(g, f"{key}.{name}")
                assert float((got - ref).abs().max()) <= tol * float(ref.abs().max()), (key, name)


SHAPES = [(1, 160, 192, 160), (2, 160, 192, 224), (1, 4, 5, 6), (1, 1, 1, 1), (2, 20, 192, 256), (2, 37, 169, 353), (3, 9, 24, 32),
          (1, 70, 49, 33), (32, 7, 120, 160), (1, 2, 3, 70)]


def test_plan_restatement_equals_the_library():
    """modet_ncc_ws_bytes is host code: three coefficient volumes + one loss partial per workgroup of the window-3 launch (the
    largest grid of the four windows) + 64 floats, so the restated grid is checked against the library without a GPU"""
    from smilecode_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    shapes = SHAPES + [(c[1],) + c[0] for c in ncc_oracle.MARCH_CASES.values()]
    for B, D, H, W in shapes:
        tiles_x, tiles_y, zc, nchunk, grid = ncc_oracle.march_plan(B, D, H, W, 3)
        assert lib.modet_ncc_ws_bytes(B, D, H, W) == (3 * B * D * H * W + grid + 64) * 4, (B, D, H, W)
        assert grid == B * tiles_x * tiles_y * nchunk and (nchunk - 1) * zc < D <= nchunk * zc
        for w in (5, 7, 9):                     # the workspace sized for window 3 holds every other window's partials
            assert ncc_oracle.march_plan(B, D, H, W, w)[4] <= grid, (B, D, H, W, w)


def test_plan_of_the_benchmarked_step():
    """160 x 192 x 160: 5 x 8 = 40 tile columns -> 20 chunks wanted -> 8 planes: below window 9, so chunks of 9 there (zc == win:
    the zc != win replacement order of the ring is reached by the two plan* cases of the GPU file alone), and 8 at window 3"""
    assert ncc_oracle.march_plan(1, 160, 192, 160, 9) == (5, 8, 9, 18, 720)
    assert ncc_oracle.march_plan(1, 160, 192, 160, 3) == (5, 8, 8, 20, 800)


def test_gpu_cases_reach_the_chunking_they_are_there_for():
    """every (case, window) of the GPU file: chunk length, chunk count and the planes left to the last chunk; every window has a
    batch-2 case with several chunks and a short last one, and both plan* cases have zc != win"""
    seen = set()
    for tag, (shape, batch, _, _, _, windows, _) in ncc_oracle.MARCH_CASES.items():
        for w in windows:
            _, _, zc, nchunk, _ = ncc_oracle.march_plan(batch, *shape, w)
            last = shape[0] - (nchunk - 1) * zc
            assert (zc, nchunk, last) == ncc_oracle.MARCH_CHUNKS[(tag, w)], (tag, w, zc, nchunk, last)
            seen.add((tag, w))
            if tag.startswith("plan"):
                assert zc > w
    assert seen == set(ncc_oracle.MARCH_CHUNKS) and len(seen) == 21
    for w in (3, 5, 7, 9):
        cases = [t for (t, cw) in seen if cw == w]
        assert len(cases) >= 3, w
        assert any(ncc_oracle.MARCH_CASES[t][1] == 2 and ncc_oracle.MARCH_CHUNKS[(t, w)][1] > 1
                   and ncc_oracle.MARCH_CHUNKS[(t, w)][2] < ncc_oracle.MARCH_CHUNKS[(t, w)][0] for t in cases), w
