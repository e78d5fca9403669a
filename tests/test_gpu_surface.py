"""-m gpu: ops.surface_distances (csrc/surface.hip) against the all-pairs numpy restatement of tests/surface_oracle.py.

counts (voxels, border voxels, the integer squares of the maximum and of the two order statistics) are EXACTLY equal; metrics are
within 1e-12 relative (absolute where the value is 0): both sides take correctly rounded square roots of the same integers, and the
means are fp64 sums of at most about 10^4 non-negative terms, each within an ulp, in different orders -- n * 2^-53 ~ 1e-12 is the
first-order bound of either, the observed error is a few 1e-16.  NaN sits exactly where the oracle has an empty side.

Shapes: 5x6x7 every voxel on the volume's face; 4x5x67 a row longer than a wave; 3x4x300 a line longer than a workgroup; 9x13x35
partial 16-line tiles on every axis; 1x1x9 and 1x8x8 unit dimensions; 40x48x40 with 8 labels the largest.  Voronoi maps hold
every label by construction (tests/test_cpu_surface.py asserts it): no case is skipped for a missing label."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import surface_oracle as so
from tests.test_cpu_surface import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-12
_REF = {}


def reference(key, a, b, nlabels, q=95.0):
    """the oracle's answer, computed once per case and shared (read-only)"""
    k = (key, nlabels, float(q))
    if k not in _REF:
        m, c = so.surface_distances(a, b, nlabels, q)
        m.setflags(write=False); c.setflags(write=False)
        _REF[k] = (m, c)
    return _REF[k]


def run(a, b, nlabels, q=95.0):
    from smilecode_amd import ops
    m, c = ops.surface_distances(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), nlabels, q)
    assert m.shape == (nlabels, 5) and m.dtype == torch.float64 and c.shape == (nlabels, 7) and c.dtype == torch.int64 and m.is_cuda
    return m.cpu().numpy(), c.cpu().numpy()


def check(key, a, b, nlabels, q=95.0):
    m, c = run(a, b, nlabels, q)
    rm, rc = reference(key, a, b, nlabels, q)
    err = rel_err(m, rm)                       # (asserts NaN in the same places)
    print("%s q=%g: worst metric error %.3e, labels present in both %d / %d" % (key, q, err, int((~np.isnan(rm[:, 0])).sum()), nlabels))
    assert np.array_equal(c, rc), (key, c, rc)
    assert err <= TOL, (key, err)
    return m, c


@pytest.mark.parametrize("tag", sorted(so.VORONOI))
def test_voronoi_maps_match_the_oracle(tag):
    shape, nl, seed = so.VORONOI[tag]
    a, b = so.voronoi_pair(shape, nl, seed)
    m, c = check(tag, a, b, nl)
    assert not np.isnan(m).any() and (c[:, :4] > 0).all()         # skip cap zero: every label was measured


@pytest.mark.parametrize("tag", sorted(so.constructed()))
def test_constructed_cases_match_the_oracle(tag):
    a, b, nl = so.constructed()[tag]
    m, c = check(tag, a, b, nl)
    if tag == "identical maps":
        assert not m.any() and not c[:, 4:].any()
    if tag == "opposite corners":
        assert c[0, 4] == sum((s - 1) ** 2 for s in a.shape)       # the last histogram bin
    if tag == "label 2 in A only, label 3 in B only":
        assert np.isnan(m[1]).all() and np.isnan(m[2]).all() and c[1, 1] == 0 and c[2, 0] == 0 and (c[1:3, 4:] == -1).all()
        assert not np.isnan(m[[0, 3]]).any()
    if tag == "nlabels=54, most absent":
        assert int((~np.isnan(m[:, 0])).sum()) == 3


@pytest.mark.parametrize("q", [0.0, 50.0, 95.0, 100.0])
@pytest.mark.parametrize("tag", ["9x13x35", "integer virtual index", "two border voxels in all"])
def test_percentiles(tag, q):
    if tag in so.VORONOI:
        shape, nl, seed = so.VORONOI[tag]
        a, b = so.voronoi_pair(shape, nl, seed)
    else:
        a, b, nl = so.constructed()[tag]
    m, c = check(tag, a, b, nl, q)
    if q == 100.0:
        assert np.array_equal(m[:, 1], m[:, 0]) and np.array_equal(c[:, 5], c[:, 4]) and np.array_equal(c[:, 6], c[:, 4])
    if q == 0.0:
        assert (c[:, 5] <= c[:, 6]).all() and np.array_equal(m[:, 1], np.sqrt(c[:, 5].astype(np.float64)))


def test_labels_on_both_sides_of_the_lds_table():
    a, b, nl = so.labels_above_the_lds_table()
    m, c = check("lds table", a, b, nl)
    assert sorted(np.flatnonzero(~np.isnan(m[:, 0])) + 1) == [1, 1024, 1025, 3000]


def test_two_runs_give_identical_bits():
    from smilecode_amd import ops
    shape, nl, seed = so.VORONOI["40x48x40"]
    a, b = (torch.from_numpy(v).cuda() for v in so.voronoi_pair(shape, nl, seed))
    m1, c1 = ops.surface_distances(a, b, nl)
    m2, c2 = ops.surface_distances(a, b, nl)
    assert torch.equal(m1.view(torch.int64), m2.view(torch.int64)) and torch.equal(c1, c2)


def test_utils_return_the_reference_layout():
    """a list of per-label values with their mean appended; C defaults to the number of distinct values of y_true; numpy arrays
    and tensors are both taken"""
    from smilecode_amd import utils
    shape, nl, seed = so.VORONOI["9x13x35"]
    a, b = so.voronoi_pair(shape, nl, seed)
    rm, _ = reference("9x13x35", a, b, nl)
    for fn, col in ((utils.hd_val, 0), (utils.hd95_val, 1), (utils.assd_val, 2)):
        for got in (fn(a, b, nl), fn(torch.from_numpy(a), torch.from_numpy(b).cuda(), nl), fn(a.astype(np.float32), b[None, None], nl)):
            assert isinstance(got, list) and len(got) == nl + 1
            assert rel_err(got[:nl], rm[:, col]) <= TOL and abs(got[nl] - np.mean(got[:nl])) <= TOL * got[nl]
    # the default C counts the distinct values of y_true, background or not (as the reference does): 6 values, labels 1..6
    b0 = b.copy(); b0[b0 == 7] = 6
    a0 = a.copy(); a0[a0 == 7] = 6
    assert len(utils.hd95_val(a0, b0)) == 6 + 1
    allv = utils.surface_vals(a, b, nl)
    assert sorted(allv) == ["assd", "hd", "hd95"] and allv["hd"] == utils.hd_val(a, b, nl)


def test_utils_raise_medpys_messages():
    from smilecode_amd import utils
    a, b, nl = so.constructed()["label 2 in A only, label 3 in B only"]
    for fn in (utils.hd_val, utils.hd95_val, utils.assd_val):
        with pytest.raises(RuntimeError, match="The second supplied array does not contain any binary object."):
            fn(a, b, nl)                   # label 2 is the first one missing: it is missing in y_true
        with pytest.raises(RuntimeError, match="The first supplied array does not contain any binary object."):
            fn(b, a, nl)
        assert len(fn(a, b, 1)) == 2       # label 1 is in both


def test_surface_val_voi_skips_and_counts_missing_labels():
    from smilecode_amd import utils
    a, b, nl = so.constructed()["label 2 in A only, label 3 in B only"]
    rm, _ = reference("label 2 in A only, label 3 in B only", a, b, nl)
    got = utils.surface_val_VOI(torch.from_numpy(a)[None, None], torch.from_numpy(b)[None, None].cuda(), nl)
    assert sorted(got) == ["assd", "hd", "hd95", "n_skipped"] and got["n_skipped"] == 2
    for name, col in (("hd", 0), ("hd95", 1), ("assd", 2)):
        assert rel_err(got[name], np.mean(rm[[0, 3], col])) <= TOL
    got = utils.surface_val_VOI(a, b)                       # 54 labels: 50 absent from both, 2 from one
    assert got["n_skipped"] == 52
    none = utils.surface_val_VOI(np.zeros_like(a), b, nl)
    assert none["n_skipped"] == nl and all(np.isnan(none[k]) for k in ("hd", "hd95", "assd"))


def _infer_lines(argv):
    from smilecode_amd import infer
    out = io.StringIO()
    torch.manual_seed(5)                   # the synthetic run draws its weights: the same ones in both runs
    with contextlib.redirect_stdout(out):
        infer.main(argv)
    return out.getvalue().splitlines()


def test_infer_surface_prints_the_new_lines_and_nothing_else_changes():
    base = ["--synthetic", "2", "--img-size", "32,32,32"]
    plain, surf = _infer_lines(base), _infer_lines(base + ["--surface"])
    npairs = sum(1 for ln in plain if ln.startswith("Trans dsc:"))
    assert npairs >= 1 and len(plain) == npairs + 2
    assert plain[-2].startswith("Deformed DSC:") and plain[-1].startswith("deformed det:")
    assert not [ln for ln in plain if "hd95" in ln.lower() or "assd" in ln.lower()]
    new = [ln for ln in surf if ln not in plain]
    assert [ln for ln in surf if ln in plain] == plain                # today's lines, in today's order
    per_pair = [ln for ln in new if ln.startswith("Trans hd95:")]
    assert len(per_pair) == npairs and len(new) == npairs + 1
    assert new[-1] == surf[-1] and new[-1].startswith("Deformed HD95:") and "ASSD:" in new[-1] and "+-" in new[-1]
    for ln in per_pair:
        vals = [float(p.split(",")[0]) for p in ln.split(": ")[1:5]]
        assert all(np.isfinite(v) and v >= 0.0 for v in vals), ln
