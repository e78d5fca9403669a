"""No GPU: the restatement of tests/surface_oracle.py against the recorded results of medpy's algorithm over scipy.ndimage, the
seventh header / table / export agreement, host-side answers of modet_surface_ws_bytes, and the argument checks of
ops.surface_distances and the utils functions in front of the library."""
import numpy as np
import pytest
import torch

from tests import guard
from tests import surface_oracle as so
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import gold

GOLDEN_TAGS = ("voronoi 5x6x7", "voronoi 4x5x67", "voronoi 9x13x35", "voronoi 17x20x23 q50", "interior hole", "two components",
               "label 2 in A only, label 3 in B only", "values outside 1..nlabels", "opposite corners", "integer virtual index")


def rel_err(got, ref):
    """largest |got - ref| / |ref| over the finite entries, absolute where ref is 0; NaN must sit in the same places"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    d = np.abs(got[ok] - ref[ok])
    return float(np.max(np.where(ref[ok] == 0.0, d, d / np.where(ref[ok] == 0.0, 1.0, np.abs(ref[ok])))))


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
def test_oracle_reproduces_the_goldens(tag):
    g = gold("op_surface.npz")
    a, b = g[tag + ".a"], g[tag + ".b"]
    assert a.dtype == np.int16 and b.dtype == np.int16
    m, c = so.surface_distances(a, b, int(g[tag + ".nlabels"]), float(g[tag + ".percentile"]))
    assert np.array_equal(c, g[tag + ".counts"]), tag
    assert rel_err(m, g[tag + ".metrics"]) <= 1e-12, tag


def test_goldens_hold_exactly_the_golden_cases():
    g = gold("op_surface.npz")
    assert sorted(g.files) == sorted("%s.%s" % (t, q) for t in GOLDEN_TAGS for q in ("a", "b", "nlabels", "percentile", "metrics", "counts"))
    # both kinds of missing label and a non-default percentile are among them
    c = g["label 2 in A only, label 3 in B only.counts"]
    assert c[1, 0] > 0 and c[1, 1] == 0 and c[2, 0] == 0 and c[2, 1] > 0 and (c[1:3, 4:] == -1).all()
    assert float(g["voronoi 17x20x23 q50.percentile"]) == 50.0


def test_voronoi_maps_hold_every_label():
    """the skip cap of the GPU tests is zero: no case may lose a label by accident"""
    for tag, (shape, nl, seed) in so.VORONOI.items():
        for m in so.voronoi_pair(shape, nl, seed):
            assert m.shape == shape and m.dtype == np.int16 and sorted(np.unique(m)) == list(range(1, nl + 1)), tag
    a, b, nl = so.labels_above_the_lds_table()
    assert sorted(np.unique(a)) == sorted(np.unique(b)) == [1, 1024, 1025, 3000] and nl == 3000


def test_constructed_cases_are_what_their_names_say():
    c = so.constructed()
    a, b, _ = c["opposite corners"]
    _, cnt = so.surface_distances(a, b, 1)
    assert cnt[0, 4] == sum((s - 1) ** 2 for s in a.shape)                  # the last histogram bin
    _, cnt = so.surface_distances(*c["two border voxels in all"])
    assert cnt[0, 2] + cnt[0, 3] == 2
    _, cnt = so.surface_distances(*c["integer virtual index"])
    n = int(cnt[0, 2] + cnt[0, 3])
    assert (n - 1) * 0.95 == 19.0 and (n - 1) * 0.5 == 10.0
    m, cnt = so.surface_distances(*c["identical maps"])
    assert not m.any() and not cnt[:, 4:].any()
    _, cnt = so.surface_distances(*c["nlabels=54, most absent"])
    assert int((cnt[:, 0] > 0).sum()) == 3


def test_surface_header_table_and_exports_agree():
    """every name include/modet_hip_surface.h declares has a signature in _lib.FAMILIES["surface"] and is exported by the library,
    the table holds nothing else and shares no name with another family (tests/guard_family.py)"""
    check_family_table("surface", {"modet_surface_ws_bytes", "modet_surface_distances"}, ["modet_surface_distances"])
    from smilecode_amd import _lib, build, ops
    txt = open(_lib.FAMILIES["surface"][0]).read()
    assert "MODET_SURFACE_MAX_DIM = %d" % ops.SURFACE_MAX_DIM in txt and "MODET_SURFACE_MAX_LABELS = %d" % ops.SURFACE_MAX_LABELS in txt
    assert "surface.hip" in build.SOURCES
    assert not [n for n in dir(_lib) if "SURFACE" in n]                      # a new family gets no legacy alias
    assert _lib.load().modet_hip_version() >= 444


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("surface", tmp_path, "return modet_surface_ws_bytes(0, 0, 0, MODET_SURFACE_MAX_LABELS) != 0;")


def test_workspace_size_answers_on_the_host():
    """12 bytes per voxel, two histograms and 48 bytes per label, each part rounded up to 256 bytes: a small multiple of the
    volume that does not grow with nlabels x volume; 0 for arguments out of range"""
    from smilecode_amd import _lib
    q = _lib.load().modet_surface_ws_bytes
    up = lambda n: (n + 255) // 256 * 256      # noqa: E731

    def want(D, H, W, nl):
        V, bins = D * H * W, (D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1
        return up((nl + 1) * 48) + up(8 * bins) + 2 * up(4 * V) + 2 * up(2 * V)
    for args in ((5, 6, 7, 4), (1, 1, 9, 2), (40, 48, 40, 8), (160, 192, 160, 54), (512, 512, 512, 32767), (3, 4, 300, 1)):
        assert q(*args) == want(*args), args
    V = 160 * 192 * 160
    assert q(160, 192, 160, 54) < 12.2 * V and q(160, 192, 160, 32767) - q(160, 192, 160, 54) < 2 * 2 ** 20
    for bad in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, -1, 4), (513, 4, 4, 4), (4, 513, 4, 4), (4, 4, 513, 4), (4, 4, 4, 0), (4, 4, 4, -1),
                (4, 4, 4, 32768)):
        assert q(*bad) == 0, bad


class _Fake:
    """a tensor that claims to live on the GPU (the checks in front of the library look at nothing else)"""
    is_cuda = True

    def __init__(self, dtype=torch.int16, shape=(4, 5, 6), contiguous=True, device="cuda:0"):
        self.dtype, self.shape, self._c, self.device = dtype, tuple(shape), contiguous, torch.device(device)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c


def test_ops_check_arguments_before_the_launch(monkeypatch):
    """every refusal of ops.surface_distances fires before anything that launches is reached"""
    from smilecode_amd import _lib, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["surface"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    sd, ok = ops.surface_distances, _Fake()
    for a, b in ((_Fake(torch.int32), ok), (ok, _Fake(torch.float32)), (_Fake(torch.int64), ok)):
        with pytest.raises(RuntimeError, match="int16"):
            sd(a, b)
    for a, b in ((_Fake(shape=(5, 6)), ok), (ok, _Fake(shape=(1, 4, 5, 6))), (_Fake(shape=(2, 1, 4, 5, 6)), ok)):
        with pytest.raises(RuntimeError, match=r"\(D,H,W\)"):
            sd(a, b)
    with pytest.raises(RuntimeError, match="2-D"):
        sd(_Fake(shape=(5, 6)), ok)
    with pytest.raises(RuntimeError, match="B > 1"):
        sd(_Fake(shape=(2, 4, 5, 6)), ok)
    with pytest.raises(RuntimeError, match="contiguous"):
        sd(ok, _Fake(contiguous=False))
    with pytest.raises(RuntimeError, match="does not match"):
        sd(ok, _Fake(shape=(4, 5, 7)))
    with pytest.raises(RuntimeError, match="lives on"):
        sd(ok, _Fake(device="cuda:1"))
    with pytest.raises(RuntimeError, match="GPU"):
        sd(torch.zeros(4, 5, 6, dtype=torch.int16), ok)
    with pytest.raises(RuntimeError, match="GPU"):
        sd(ok, torch.zeros(4, 5, 6, dtype=torch.int16))
    for shape in ((0, 5, 6), (4, 5, 513), (513, 1, 1)):
        with pytest.raises(RuntimeError, match="1..512"):
            sd(_Fake(shape=shape), _Fake(shape=shape))
    for n in (0, -1, 32768, 54.0, "54", True, None):
        with pytest.raises(RuntimeError, match="nlabels"):
            sd(ok, ok, n)
    for q in (-1, -1e-9, 100.5, 101, float("nan"), float("inf"), "95", None, True):
        with pytest.raises(RuntimeError, match="percentile"):
            sd(ok, ok, 54, q)
    assert not [n for n, _ in px.records if guard.is_launching(n)]


def test_utils_refuse_what_is_left_out_by_name(monkeypatch):
    """voxel spacing, connectivity other than 1, 2-D maps and B > 1 are named in the refusal, before the library is reached"""
    from smilecode_amd import _lib, utils
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["surface"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    vol = np.ones((4, 5, 6), np.int16)
    for fn in (utils.assd_val, utils.hd_val, utils.hd95_val):
        with pytest.raises(RuntimeError, match="voxelspacing"):
            fn(vol, vol, 1, voxelspacing=(1.0, 1.0, 2.0))
        with pytest.raises(RuntimeError, match="connectivity"):
            fn(vol, vol, 1, connectivity=2)
        with pytest.raises(RuntimeError, match="2-D"):
            fn(vol[0], vol[0], 1)
        with pytest.raises(RuntimeError, match="B > 1"):
            fn(np.ones((2, 1, 4, 5, 6), np.int16), np.ones((2, 1, 4, 5, 6), np.int16), 1)
        with pytest.raises(TypeError):
            fn(vol, vol, 1, (1.0, 1.0, 1.0))               # the reference's signature: (y_pred, y_true, C=None) and nothing positional after
    with pytest.raises(RuntimeError, match="B > 1"):
        utils.surface_val_VOI(torch.ones(2, 1, 4, 5, 6), torch.ones(2, 1, 4, 5, 6))
    assert not [n for n, _ in px.records if guard.is_launching(n)]


def test_infer_parser_has_the_surface_flag():
    from smilecode_amd import infer
    assert infer.make_parser().parse_args([]).surface is False
    assert infer.make_parser().parse_args(["--surface"]).surface is True
