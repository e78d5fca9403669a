"""Host-only proof that tests/test_gpu_warp_exact.py may ask for EQUALITY: on the lattice cases of tests/warp_exact.py the fp64
oracle's out, d_src and d_flow are fp32 numbers, the same oracle run in fp32 gives the same bits, and the cap holds under which
ANY order of float additions is exact.

The cap is a condition, not a measurement.  Every contribution to a d_src cell is w * d_out with w a multiple of 1/64 and d_out
an integer, so every partial sum -- of any subset, in any order -- is a multiple of 1/64 whose magnitude is at most
S = sum |w * d_out| over the cell.  A multiple of 1/64 below 2^24 / 64 is an fp32 number, so with 64 S < 2^24 no addition
rounds.  d_flow: a term is (+-) a product of two weights (a multiple of 1/16) times src * d_out (an integer), so its lsb is 1/16;
per axis the weights of the four (dy, dx) pairs sum to 1 on each of the two dz levels, so with |src| <= 8 the sum of the |terms|
is at most 2 * 8 * sum_c |d_out_c|, plus |d_out| <= 4 of add_flow's identity term and |d_flow_add| <= 2.
`collapse` on 24x32x40 with C = 16 reaches 64 S = 1.3e6, thirteen times below the cap; on 41x100x100 it would reach 2.0e7 and break
it, which is why that family is confined to the one small shape."""
import numpy as np
import pytest
import torch

from tests import warp_exact as wx

CAP = float(2 ** 24)


@pytest.mark.parametrize("case", wx.CASES, ids=wx.case_id)
def test_lattice_case_is_exact_in_fp32_and_under_the_cap(case):
    s, C, fam = case
    x = wx.inputs(case)
    src, flow, dout, add = (x[k].numpy() for k in ("src", "flow", "dout", "add"))
    # the inputs are what the table promises
    assert np.array_equal(src, np.round(src)) and np.abs(src).max() <= 8
    assert np.array_equal(src, torch.from_numpy(src).bfloat16().float().numpy())
    assert np.array_equal(dout, np.round(dout)) and np.abs(dout).max() <= 4 and (np.abs(dout).max(-1) == 0).any()
    assert np.array_equal(add * 4, np.round(add * 4)) and np.abs(add).max() <= 2
    step = 2 if fam in wx.HALF_LATTICE else 4
    assert np.array_equal(flow * step, np.round(flow * step))
    pos = wx.positions(flow)
    dims = np.array(wx.SHAPES[s][1:], dtype=np.float64)
    assert (pos >= -2).all() and (pos <= dims + 1).all()
    if fam == "white1":
        assert np.abs(flow).max() == 1.0 and (flow == 1.0).any() and (flow == -1.0).any()
    # fp64 reference == its own fp32 rounding == the fp32 oracle
    r64 = wx.oracle(case, torch.float64)
    r32 = wx.oracle(case, torch.float32)
    for name, a, b in zip(("out", "d_src", "d_flow", "nearest"), r64, r32):
        assert torch.equal(a.float().double(), a), (name, "fp64 result is not an fp32 number")
        assert torch.equal(b.double(), a), (name, "fp32 oracle differs from fp64", int((b.double() != a).sum()))
    ref = wx.reference(case)
    assert torch.equal(ref["dsrc"].double(), r64[1]) and torch.equal(ref["dflow"].double(), r64[2])
    # the cap
    s_abs = wx.oracle(case, torch.float64, abs_dout=True)[1]
    assert float(s_abs.abs().max()) * 64.0 < CAP, float(s_abs.abs().max()) * 64.0
    flow_terms = 2.0 * 8.0 * np.abs(dout).sum(-1).max() + 4.0 + 2.0
    assert flow_terms * 16.0 < CAP
    # the derived forms stay fp32 numbers
    if C == 3:
        assert torch.equal(wx.expected_out(case, True).double(), r64[0] + x["flow"].double())
        assert torch.equal(wx.expected_dflow(case, True, True).double(), r64[2] + x["dout"].double() + x["add"].double())
    assert torch.equal(wx.expected_dflow(case, False, True).double(), r64[2] + x["add"].double())


def test_collapse_cap_margin():
    """the figure of the docstring: 64 * sum |w d_out| of the heaviest cell of `collapse` at C = 16"""
    s_abs = wx.oracle(("24x32x40", 16, "collapse"), torch.float64, abs_dout=True)[1]
    worst = float(s_abs.abs().max()) * 64.0
    print("collapse 24x32x40 C=16: 64 * S = %.3e (cap %.3e)" % (worst, CAP))
    assert worst * 8.0 < CAP
    assert all(s == "24x32x40" for s, _, f in wx.CASES if f == "collapse")


def test_collapse_lands_on_tile_corners_and_overflows_the_segment():
    flow = wx.inputs(("24x32x40", 8, "collapse"))["flow"]
    pos = wx.positions(flow)
    for b, t in enumerate(wx.COLLAPSE_TARGETS):
        assert all(v % 8 == 0 for v in t)
        assert np.abs(pos[b] - np.array(t)).max() <= 0.5
    # 30 720 voxels of a sample land in the eight tiles around the corner: far beyond one tile's 1 536-entry segment
    assert pos[0].reshape(-1, 3).shape[0] > 8 * 1536


@pytest.mark.parametrize("s", sorted(wx.SHAPES))
def test_half_family_is_mostly_ties(s):
    flow = wx.make_flow("half", wx.SHAPES[s])
    frac = wx.tie_fraction(flow)
    print("half %s: %.1f %% of the voxels have a coordinate at an exact tie" % (s, 100 * frac))
    assert frac > 0.5


@pytest.mark.parametrize("s", sorted(wx.SHAPES))
def test_faces_family_reaches_every_boundary_position_on_every_face(s):
    shape = wx.SHAPES[s]
    pos = wx.positions(wx.make_flow("faces", shape))
    for a, n in enumerate(shape[1:]):
        lo = np.take(pos[..., a], 0, axis=1 + a)
        hi = np.take(pos[..., a], n - 1, axis=1 + a)
        for v in wx.FACE_SWEEP:
            assert (lo == v).any(), (s, a, "low", v)
            assert (hi == n + v).any(), (s, a, "high", n + v)
    assert list(wx.FACE_SWEEP) == [-1.25, -1.0, -0.75, -0.5, -0.25, 0.0, 0.25]


def test_shapes_sit_where_the_table_says():
    """the host conditions of modet_warp_bwd_acc and tiles_launch, restated in warp_exact"""
    for s in ("5x6x7", "9x13x35"):
        assert not any(wx.runs_patch_kernel(wx.SHAPES[s], C) for C in (3, 8, 12, 16, 64)) and wx.fill_sz(wx.SHAPES[s]) == 1
    assert not any(wx.runs_patch_kernel(wx.SHAPES["24x32x40"], C) for C in (3, 8, 16))
    s = wx.SHAPES["17x41x250"]
    assert wx.patch_items(s, 8) == 66000 and not wx.runs_patch_kernel(s, 3) and all(wx.runs_patch_kernel(s, C) for C in (8, 12, 16))
    assert wx.fill_sz(s) == 1
    s = wx.SHAPES["33x45x137"]
    assert wx.patch_items(s, 3) == 65760 and all(wx.runs_patch_kernel(s, C) for C in (3, 8, 16)) and wx.fill_sz(s) == 4
    assert all(d % 4 for d in s[1:])
    for sk, C, _ in wx.CASES:
        assert C <= 16 or sk in ("5x6x7", "9x13x35")


def test_label_cases_hold_uncounted_labels_and_ties():
    for key in wx.LABEL_CASES:
        mov, fix, flow, warped, counts = wx.label_case(key)
        assert mov.dtype == np.int16 and mov.max() == wx.LABEL_MAX and mov.min() == 0 and fix.max() == wx.LABEL_MAX
        assert counts.shape[1:] == (3, wx.NLABELS + 1)
        assert (counts[:, 0].sum(-1) < mov.size).all(), "some warped voxels carry 55 / 56 and stay uncounted"
        assert (counts[:, 2] <= counts[:, 0]).all() and (counts[:, 2] <= counts[:, 1]).all() and counts[:, 2].sum() > 0
        if key[1] == "half":
            assert wx.tie_fraction(flow) > 0.5
