"""-m gpu: the label-overlap (soft Dice) kernels of csrc/segdice.hip against the ATen composition in fp64 on the CPU
(tests/segdice_oracle.py): the [I, P, T] table bit for bit on lattice flows and against modet_label_warp_counts on integer ones, the
loss within 4 fp32 ulp, d_flow within the larger of 2 x the error of the same composition in fp32 on the GPU and 16 * 2^-24; a
general flow; bit-reproducibility, batch independence, the add-into option, flows of 1e9 and NaN, the autograd Function; and the
train step with the term: seeded against autograd, captured against eager on a second pair, and unchanged without it.

Shapes (tests/segdice_oracle.py): odd sizes, two batch items, a degenerate axis with a row longer than a wave, and 16^3 (16
workgroups' worth of rows, whole waves inside one region).  Labels 1, 5, 54 and 256 with 0, -32768, 32767 and L + 1 in both maps and
one label in neither."""
import functools

import numpy as np
import pytest
import torch

from tests import segdice_oracle as so
from tests.util import note_many

pytestmark = pytest.mark.gpu

CASES = [(shape, L) for shape in so.SHAPES for L in so.LABELS]
IDS = ["%dx%dx%dx%d-L%d" % (shape + (L,)) for shape, L in CASES]
FLOOR = 16 * 2.0 ** -24          # eight products of three factors and one table rounding, relative to max |d_flow|


def _seed(shape, L):
    return 1000 * so.SHAPES.index(shape) + L


@functools.lru_cache(maxsize=None)
def _inputs(shape, L, kind="lattice"):
    mov, fix = so.make_labels(shape, L, seed=_seed(shape, L))
    flow = {"lattice": so.lattice_flow, "integer": so.integer_flow, "general": so.general_flow}[kind](shape, _seed(shape, L) + 7)
    return mov, fix, flow


@functools.lru_cache(maxsize=None)
def _reference(shape, L, kind="lattice"):
    """(fp64 on the CPU, fp32 on the GPU) of the ATen composition: (table, loss, d_flow) each; computed once per case"""
    mov, fix, flow = _inputs(shape, L, kind)
    r64 = so.value_and_grad(mov, flow, fix, L, torch.float64)
    r32 = tuple(t.cpu() for t in so.value_and_grad(mov.cuda(), flow.cuda(), fix.cuda(), L, torch.float32))
    return r64, r32


@functools.lru_cache(maxsize=None)
def _hip(shape, L, kind="lattice"):
    """(table, loss, d_flow planar) of one call on the channels-last flow, on the host"""
    from smilecode_amd import ops
    mov, fix, flow = _inputs(shape, L, kind)
    loss, d = ops.seg_dice_value_and_grad_cl(so.cl(flow).cuda(), mov.cuda(), fix.cuda(), L)
    table = ops.seg_dice_sums(mov.cuda(), flow.cuda(), fix.cuda(), L)
    return table.cpu(), loss.cpu(), so.planar(d).cpu()


def _grad_errors(shape, L, kind, mask=None):
    (_, _, g64), (_, _, g32) = _reference(shape, L, kind)
    _, _, gh = _hip(shape, L, kind)
    scale = float(g64.abs().max())
    assert scale > 0.0
    keep = torch.ones_like(g64, dtype=torch.bool) if mask is None else mask
    e_hip = float(((gh.double() - g64).abs() * keep).max()) / scale
    e_aten = float(((g32.double() - g64).abs() * keep).max()) / scale
    return e_hip, e_aten


@pytest.mark.parametrize("shape,L", CASES, ids=IDS)
def test_lattice_flow_table_bit_for_bit_loss_within_4_ulp_and_gradient_within_aten(shape, L):
    (t64, l64, g64), _ = _reference(shape, L)
    table, loss, gh = _hip(shape, L)
    assert table.dtype == torch.float64 and table.shape == t64.shape == (shape[0], 3, L + 1)
    assert float(t64[:, 0, 1:].max()) > 0.0 and float(t64[:, 1, 1:].max()) > float(t64[:, 0, 1:].max())
    assert bool((t64 * 4096 == (t64 * 4096).round()).all())                    # the weights are multiples of 2^-12
    assert torch.equal(table, t64), float((table - t64).abs().max())
    a = so.absent_label(L)
    if a is not None:
        assert float(table[:, :, a].abs().max()) == 0.0
    want = np.float32(float(l64))
    ulp = float(np.spacing(want))
    err = abs(float(loss) - float(l64))
    print(f"segdice[{shape},L{L}] loss {float(loss):.9g} fp64 {float(l64):.17g} err {err / ulp:.3f} ulp")
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss)) and err <= 4 * ulp, (float(loss), float(l64))
    e_hip, e_aten = _grad_errors(shape, L, "lattice")
    tag = "segdice[%dx%dx%dx%d.L%d]" % (shape + (L,))
    note_many({tag + ".dflow.e_hip": e_hip, tag + ".dflow.e_aten": e_aten, tag + ".loss.err_ulp": err / ulp})
    print(f"{tag} d_flow: hip {e_hip:.3e} aten-fp32 {e_aten:.3e} bound {max(2 * e_aten, FLOOR):.3e}")
    assert gh.shape == g64.shape and bool(torch.isfinite(gh).all())
    assert e_hip <= max(2 * e_aten, FLOOR), (e_hip, e_aten)


@pytest.mark.parametrize("shape,L", CASES, ids=IDS)
def test_integer_flow_table_equals_label_warp_counts(shape, L):
    """modet_label_warp_counts keeps its histogram of nlabels + 1 bins in a table of 256, so it counts at most 255 labels: with
    L = 256 the labels 1..255 are compared with its counts and label 256 with the voxels of the label map it warped"""
    from smilecode_amd import ops
    mov, fix, flow = _inputs(shape, L, "integer")
    table, loss, _ = _hip(shape, L, "integer")
    n = min(L, 255)
    for b in range(shape[0]):
        warped, counts = ops.label_warp_counts(mov[b, 0].cuda(), so.cl(flow[b:b + 1]).cuda(), fix[b, 0].cuda(), nlabels=n)
        counts, warped = counts.cpu().double(), warped.cpu()
        assert torch.equal(table[b, 0, 1:n + 1], counts[2, 1:]) and torch.equal(table[b, 1, 1:n + 1], counts[0, 1:])
        assert torch.equal(table[b, 2, 1:n + 1], counts[1, 1:]) and float(table[b, :, 0].abs().max()) == 0.0
        for l in range(n + 1, L + 1):
            a, t = warped == l, fix[b, 0] == l
            assert [float(v) for v in table[b, :, l]] == [float((a & t).sum()), float(a.sum()), float(t.sum())], l
    t64, l64 = so.table_and_loss(mov, flow, fix, L)
    assert torch.equal(table, t64)
    assert abs(float(loss) - float(l64)) <= 4 * float(np.spacing(np.float32(float(l64))))


def test_pure_regions_take_the_wave_wide_path_to_the_same_counts():
    """maps without noise and a zero flow: whole waves see one label at all eight corners, the sums are the regions' sizes"""
    from smilecode_amd import ops
    shape, L = (1, 16, 16, 16), 54
    mov, fix = so.make_labels(shape, L, seed=5, noise=0.0)
    flow = torch.zeros((1, 3) + shape[1:])
    flow[:, 2, :, :, 8:] = 0.5                                                # and half of each row between two voxels
    table = ops.seg_dice_sums(mov.cuda(), flow.cuda(), fix.cuda(), L).cpu()
    t64, _ = so.table_and_loss(mov, flow, fix, L)
    assert torch.equal(table, t64) and float(t64[0, 1].sum()) > 0.9 * 16 ** 3 * 0.9


def test_no_label_present_gives_loss_one_and_no_nan():
    from smilecode_amd import ops
    shape = (1, 5, 6, 7)
    lab = torch.tensor(so.hostile(1), dtype=torch.int16)[torch.randint(4, shape, generator=torch.Generator().manual_seed(1))][:, None]
    flow = so.lattice_flow(shape, seed=2)
    loss, d = ops.seg_dice_value_and_grad_cl(so.cl(flow).cuda(), lab.cuda(), lab.flip(-1).contiguous().cuda(), 1)
    assert float(loss) == 1.0 and not bool(d.any())
    assert not bool(ops.seg_dice_sums(lab.cuda(), flow.cuda(), lab.cuda(), 1).any())


@pytest.mark.parametrize("shape,L", [((2, 4, 5, 9), 5), ((1, 16, 16, 16), 54)], ids=["2x4x5x9-L5", "1x16x16x16-L54"])
def test_general_flow_within_the_aten_fp32_bound(shape, L):
    """a flow that is not dyadic.  Value: within the larger of 2 x the fp32 composition's own error and 16 * 2^-24 of the value (the
    weights that make up the sums carry the roundings the gradient's floor counts).  Gradient: compared only at voxels whose p is
    at least 1e-3 from an integer on every axis -- by construction of the flow (fractional parts in [0.01, 0.99]) that is every
    voxel, so the mask leaves none out and the fp64 gradient is never evaluated at a kink."""
    mov, fix, flow = _inputs(shape, L, "general")
    (t64, l64, _), (t32, l32, _) = _reference(shape, L, "general")
    table, loss, _ = _hip(shape, L, "general")
    p = so.positions(flow)
    away = ((p - p.round()).abs() >= 1e-3).all(1, keepdim=True).expand_as(p)
    assert bool(away.all())
    e_val, e_val_aten = abs(float(loss) - float(l64)), abs(float(l32) - float(l64))
    e_tab = float((table - t64).abs().max() / t64.abs().max())
    e_tab_aten = float((t32.double() - t64).abs().max() / t64.abs().max())
    e_hip, e_aten = _grad_errors(shape, L, "general", away)
    tag = "segdice.general[%dx%dx%dx%d.L%d]" % (shape + (L,))
    note_many({tag + ".loss.e_hip": e_val, tag + ".loss.e_aten": e_val_aten, tag + ".table.e_hip": e_tab, tag + ".table.e_aten": e_tab_aten,
               tag + ".dflow.e_hip": e_hip, tag + ".dflow.e_aten": e_aten})
    print(f"{tag} loss: hip {e_val:.3e} aten {e_val_aten:.3e}; table: hip {e_tab:.3e} aten {e_tab_aten:.3e}; "
          f"d_flow: hip {e_hip:.3e} aten {e_aten:.3e}")
    assert e_val <= max(2 * e_val_aten, FLOOR * abs(float(l64))), (e_val, e_val_aten)
    assert e_tab <= max(2 * e_tab_aten, FLOOR), (e_tab, e_tab_aten)
    assert e_hip <= max(2 * e_aten, FLOOR), (e_hip, e_aten)


def _vg(shape, L, flow=None, B=None, **kw):
    from smilecode_amd import ops
    mov, fix, f = _inputs(shape, L)
    f = f if flow is None else flow
    s = slice(None) if B is None else slice(0, B)
    return ops.seg_dice_value_and_grad_cl(so.cl(f[s]).cuda(), mov[s].cuda(), fix[s].cuda(), L, **kw)


def test_two_runs_are_bit_identical():
    from smilecode_amd import ops
    for shape, L in (((2, 4, 5, 9), 54), ((1, 16, 16, 16), 256), ((1, 1, 3, 70), 5)):
        mov, fix, flow = _inputs(shape, L)
        l1, d1 = _vg(shape, L)
        t1 = ops.seg_dice_sums(mov.cuda(), flow.cuda(), fix.cuda(), L)
        junk = torch.rand(1 << 20, device="cuda")                 # another allocation pattern for the second run's workspace
        l2, d2 = _vg(shape, L)
        t2 = ops.seg_dice_sums(mov.cuda(), so.cl(flow).cuda(), fix.cuda(), L, channels_last=True)
        del junk
        assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(t1, t2), (shape, L)
        assert float(d1.abs().max()) > 0.0


def test_item_0_of_a_batch_of_two_equals_the_call_on_it_alone():
    """the table rows as they are; d_flow with the mean over b taken out: 1 / (B L) halves every coefficient exactly, and
    grad_scale = 2 doubles the result exactly, so the bits are those of the B = 1 call"""
    from smilecode_amd import ops
    shape, L = (2, 4, 5, 9), 5
    mov, fix, flow = _inputs(shape, L)
    t2 = ops.seg_dice_sums(mov.cuda(), flow.cuda(), fix.cuda(), L)
    t1 = ops.seg_dice_sums(mov[:1].cuda(), flow[:1].cuda(), fix[:1].cuda(), L)
    assert torch.equal(t2[:1], t1)
    _, d2 = _vg(shape, L, grad_scale=2.0)
    _, d1 = _vg(shape, L, B=1)
    assert torch.equal(d2[:1], d1) and float(d1.abs().max()) > 0.0


def test_add_into_equals_a_separate_write_and_one_fp32_add():
    for shape, L in (((2, 4, 5, 9), 54), ((1, 16, 16, 16), 5)):
        base = torch.randn(shape[:1] + shape[1:] + (3,), generator=torch.Generator().manual_seed(9)).cuda() * 1e-3
        loss, d = _vg(shape, L, grad_scale=0.75)
        loss2, got = _vg(shape, L, grad_scale=0.75, d_flow_add=base.clone())
        assert torch.equal(loss, loss2) and torch.equal(got, base + d), float((got - (base + d)).abs().max())
        assert not torch.equal(got, base)


def test_huge_and_non_finite_flows_are_outside():
    """a displacement of 1e9 and a NaN or inf in one component: finite results, zero gradient there, and the sums, the loss and every
    other voxel's gradient of the same flow with those voxels sent outside by 1e4"""
    from smilecode_amd import ops
    shape, L = (2, 4, 5, 9), 5
    mov, fix, flow = _inputs(shape, L)
    bad, out = flow.clone(), flow.clone()
    spots = [((0, 1, 2, 3), 0, 1e9), ((0, 2, 0, 8), 2, -1e9), ((1, 0, 4, 0), 1, float("nan")), ((1, 3, 3, 5), 2, float("inf")),
             ((0, 3, 1, 1), 0, float("-inf")), ((1, 2, 2, 2), 0, 3e38)]
    for (b, z, y, x), a, v in spots:
        bad[b, a, z, y, x] = v
        out[b, :, z, y, x] = 1e4
    lb, db = _vg(shape, L, flow=bad)
    lo, do = _vg(shape, L, flow=out)
    tb = ops.seg_dice_sums(mov.cuda(), bad.cuda(), fix.cuda(), L)
    assert bool(torch.isfinite(lb)) and bool(torch.isfinite(db).all()) and bool(torch.isfinite(tb).all())
    for (b, z, y, x), _, _ in spots:
        assert not bool(db[b, z, y, x].any())
    assert torch.equal(lb, lo) and torch.equal(db, do)
    t64, _ = so.table_and_loss(mov, out, fix, L)
    assert torch.equal(tb.cpu(), t64)
    # add-into leaves such a voxel's entry as it was
    base = torch.full_like(db, 0.5)
    _, got = _vg(shape, L, flow=bad, d_flow_add=base.clone())
    for (b, z, y, x), _, _ in spots:
        assert bool((got[b, z, y, x] == 0.5).all())


def test_autograd_function_has_the_bits_of_value_and_grad_times_the_upstream_scalar():
    from smilecode_amd import losses, ops
    shape, L = (2, 4, 5, 9), 54
    mov, fix, flow = _inputs(shape, L)
    mov, fix = mov.cuda(), fix.cuda()
    l_cl, d_cl = ops.seg_dice_value_and_grad_cl(so.cl(flow).cuda(), mov, fix, L)
    f = flow.cuda().requires_grad_(True)
    loss = ops.seg_dice_loss(mov, f, fix, L)
    assert loss.shape == () and torch.equal(loss.detach(), l_cl)
    assert torch.equal(ops.seg_dice_loss(mov, f.detach(), fix, L), l_cl)       # no gradient wanted: the same value bits
    (g1,) = torch.autograd.grad(loss, [f], retain_graph=True)
    assert torch.equal(g1, so.planar(d_cl))
    u = torch.tensor(0.37, device="cuda")
    (gu,) = torch.autograd.grad(loss * u, [f])
    assert torch.equal(gu, so.planar(d_cl) * u)
    _, d_u = ops.seg_dice_value_and_grad_cl(so.cl(flow).cuda(), mov, fix, L, grad_scale=0.37)   # the same product inside the kernel
    assert torch.equal(gu, so.planar(d_u))
    f2 = flow.cuda().requires_grad_(True)
    (gm,) = torch.autograd.grad(losses.LabelDice(L)(f2, mov, fix), [f2])
    assert torch.equal(gm, g1)


# ------------------------------------------------------------------------------------------------ the train step
STEP_SHAPE = (32, 32, 32)


def _modet():
    from smilecode_amd import models, synth
    m = models.ModeT(STEP_SHAPE, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


@functools.lru_cache(maxsize=None)
def _pairs(shape=STEP_SHAPE):
    from smilecode_amd import data
    ds = data.SyntheticPairs(shape, n=3, seed=24, with_labels=True)
    return [tuple(t[None].cuda() for t in ds[i]) for i in (0, 3)]


def _per_tensor(tr, got, ref, what):
    """relative L2 per parameter tensor within Trainer._verify_tolerance(), as Trainer._verify_replay measures it"""
    rel, floor_frac = tr._verify_tolerance()
    seg, n = tr.fp.segment_index(), len(tr.fp.params)
    ref_sq = torch.zeros(n, device=ref.device, dtype=torch.float64).index_add_(0, seg, ref.double() ** 2)
    err_sq = torch.zeros(n, device=ref.device, dtype=torch.float64).index_add_(0, seg, (got - ref).double() ** 2)
    floor = floor_frac ** 2 * float(ref_sq.max())
    bad = torch.nonzero(~(err_sq <= rel ** 2 * ref_sq + floor)).flatten().tolist()
    assert float(ref_sq.max()) > 0.0 and not bad, (what, bad[:5], float((err_sq / (ref_sq + floor)).max()) ** 0.5)


def _seeded_vs_autograd(make, pair, weight):
    from smilecode_amd import losses
    from smilecode_amd.engine import Trainer
    mov, fix, ml, fl = pair
    res = {}
    for seeded in (True, False):
        tr = Trainer(make(), seg=losses.LabelDice(54), seg_weight=weight)
        tr.seed_backward = seeded
        assert tr._seedable() == seeded
        if seeded:
            out = tr._fwd_bwd(mov, fix, (ml, fl))
        else:                                                  # loss(...)[0].backward(), as the issue states the reference path
            tr.fp.zero_grad()
            out = tr.loss(mov, fix, (ml, fl))
            out[0].backward()
            tr.fp.gather_grads()
        assert len(out) == 4
        res[seeded] = (tr, tr.fp.grad.clone(), [float(v) for v in out])
    (tr, ga, la), (_, gb, lb) = res[True], res[False]
    assert la[3] == pytest.approx(lb[3], rel=1e-6) and 0.0 < la[3] <= weight and la[0] == pytest.approx(lb[0], rel=1e-5, abs=1e-6)
    _per_tensor(tr, ga, gb, "seeded vs autograd")
    return ga


def test_modet_seeded_step_with_the_term_equals_the_autograd_path():
    from smilecode_amd.engine import Trainer
    pair = _pairs()[0]
    g = _seeded_vs_autograd(_modet, pair, 0.5)
    plain = Trainer(_modet())
    plain._fwd_bwd(*pair[:2])
    assert float((g - plain.fp.grad).abs().max()) > 0.0, "the term reaches the parameters"


def test_subflow_model_seeded_step_with_the_term_equals_the_autograd_path():
    """a model with reg_on_subflows (RDNStages, two stages, at the shape of its own tests): the composed flow is one more root"""
    from smilecode_amd import models
    from tests import rdn_stages_oracle as orc
    shape, channels = (32, 48, 32), 4
    _, stages, levels, diff, share = orc.RUNS["rdn_s2"]

    def make():
        m = models.RDNStages(shape, channels=channels, stage_recursion=stages, level_recursion=list(levels), diff=diff, share=share,
                             return_stage_flows=True).cuda()
        models.load_numpy_weights(m, {n: v.float().numpy() for n, v in orc.make_weights(stages, share, channels=channels).items()})
        assert m.reg_on_subflows
        return m
    _seeded_vs_autograd(make, _pairs(shape)[0], 1.0)


def test_captured_step_refreshes_its_label_buffers():
    """capture verifies on the first pair; a replay fed a SECOND pair's images and labels gives the eager step's gradients and
    values on that pair, and differs from a replay that kept the first pair's labels"""
    from smilecode_amd import losses
    from smilecode_amd.engine import Trainer
    (m1, f1, a1, b1), (m2, f2, a2, b2) = _pairs()
    tr = Trainer(_modet(), seg=losses.LabelDice(54)).capture(m1, f1, labels=(a1, b1))
    assert tr._graph is not None and tr._static_labels is not None
    eager = Trainer(_modet(), seg=losses.LabelDice(54))
    want = eager._fwd_bwd(m2, f2, (a2, b2))
    # what train_step does in front of the optimizer: copy the pair and its labels into the static buffers, replay
    tr._static_in[0].copy_(m2); tr._static_in[1].copy_(f2)
    tr._graph.replay()
    stale = tr.fp.grad.clone()                                  # images of pair 2, labels of pair 1
    tr._static_labels[0].copy_(a2); tr._static_labels[1].copy_(b2)
    tr._graph.replay()
    torch.cuda.synchronize()
    _per_tensor(tr, tr.fp.grad, eager.fp.grad, "replay on the second pair vs eager")
    assert len(tr._static_out) == 4
    for got, ref in zip(tr._static_out, want):
        assert float(got) == pytest.approx(float(ref), rel=1e-5, abs=1e-6)
    assert float((stale - tr.fp.grad).abs().max()) > 0.0
    # and through train_step itself: the 4-tuple, the second pair's seg value
    out = tr.train_step(m2, f2, labels=(a2, b2))
    assert len(out) == 4 and float(out[3]) == pytest.approx(float(want[3]), rel=1e-5)


def test_without_the_term_the_step_is_what_it_was():
    from smilecode_amd.engine import Trainer
    mov, fix = _pairs()[0][:2]
    a, b = Trainer(_modet()), Trainer(_modet(), seg=None)
    oa, ob = a._fwd_bwd(mov, fix), b._fwd_bwd(mov, fix)
    assert len(oa) == len(ob) == 3 and all(torch.equal(x, y) for x, y in zip(oa, ob))
    a.seed_backward = b.seed_backward = True
    from smilecode_amd import ops
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)                                 # the warp scatter in a fixed order: bit-identical gradients
    try:
        a._fwd_bwd(mov, fix); b._fwd_bwd(mov, fix)
        assert torch.equal(a.fp.grad, b.fp.grad)
        out = b.train_step(mov, fix)
        assert len(out) == 3
    finally:
        ops.set_deterministic(was)
