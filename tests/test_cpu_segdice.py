"""The label-overlap (soft Dice) term without a GPU: the family's header against its ctypes table and the library's exports, the
workspace query, the entry points' refusals, the oracle of tests/segdice_oracle.py against ``oracle.modet_torch.dice_voi`` on
integer flows, every Python-side refusal by name, the trainer's ``seg`` argument and train.py's flags."""
import pytest
import torch

from oracle import modet_torch as orc
from tests import guard, segdice_oracle as so
from tests.guard_family import check_family_table, check_header_is_c99

NAMES = {"modet_segdice_ws_bytes", "modet_segdice_sums", "modet_segdice_fwd_bwd"}


def test_segdice_header_table_and_exports_agree():
    lib = check_family_table("segdice", NAMES, ["modet_segdice_sums", "modet_segdice_fwd_bwd"])
    from smilecode_amd import _lib, build, ops
    assert lib.modet_hip_version() == 447                    # a new family, no change to what exists
    assert "segdice.hip" in build.SOURCES
    txt = open(_lib.FAMILIES["segdice"][0]).read()
    assert "MODET_SEGDICE_MAX_LABELS = %d" % ops.SEGDICE_MAX_LABELS in txt and ops.SEGDICE_MAX_LABELS == 256
    for word in ("NON-FINITE", "any magnitude", "2^-32"):    # the flow rule and the fixed point's rounding are stated
        assert word in txt, word


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("segdice", tmp_path, "return modet_segdice_ws_bytes(0, 0, 0, 0, MODET_SEGDICE_MAX_LABELS) != 0;")


def test_workspace_is_zero_for_refused_shapes_and_holds_no_volume():
    from smilecode_amd import _lib
    lib = _lib.load()
    full = lib.modet_segdice_ws_bytes(1, 160, 192, 160, 54)
    # at most 1024 rows of 3 (L+1) 64-bit sums + 2 (L+1) floats per batch item: far below one label map (2 B per voxel)
    assert 0 < full <= 1024 * 3 * 55 * 8 + 2 * 55 * 4 + 16 < 2 * 160 * 192 * 160
    assert full == lib.modet_segdice_ws_bytes(1, 160, 192, 160, 54)
    for B, D, H, W in so.SHAPES:
        for L in so.LABELS:
            assert 0 < lib.modet_segdice_ws_bytes(B, D, H, W, L) <= 1024 * 3 * (L + 1) * 8 + B * 2 * (L + 1) * 4 + 16
    for bad in ((0, 4, 4, 4, 5), (1, 0, 4, 4, 5), (1, 4, 0, 4, 5), (1, 4, 4, 0, 5), (-1, 4, 4, 4, 5), (1, 4, 4, 4, 0), (1, 4, 4, 4, -3),
                (1, 4, 4, 4, 257), (1, 2048, 2048, 512, 5), (2, 1024, 1024, 1024, 5), (65536, 1, 1, 1, 5)):
        assert lib.modet_segdice_ws_bytes(*bad) == 0, bad
    assert lib.modet_segdice_ws_bytes(1, 2048, 2048, 511, 5) > 0 and lib.modet_segdice_ws_bytes(1, 1, 1, 1, 256) > 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers, bad sizes, label counts out of range and a short or misaligned workspace come back as error codes from the
    host checks (the pointers are never dereferenced on these paths); d_flow may be NULL"""
    from smilecode_amd import _lib
    lib = _lib.load()
    p = 4096                                                   # a non-NULL value that is never dereferenced

    def sums(mov=p, flow=p, fix=p, table=p, ws=p, nb=1 << 24, dims=(1, 4, 5, 6), L=5, cl=0):
        return lib.modet_segdice_sums(mov, flow, fix, table, ws, nb, *dims, L, cl, None)

    def both(mov=p, flow=p, fix=p, loss=p, table=p, ws=p, nb=1 << 24, dims=(1, 4, 5, 6), L=5, cl=1, add=0):
        return lib.modet_segdice_fwd_bwd(mov, flow, fix, loss, table, None, ws, nb, *dims, L, cl, 1.0, add, None)

    for k in ("mov", "flow", "fix", "table", "ws"):
        assert sums(**{k: None}) == -1 and both(**{k: None}) == -1, k
    assert both(loss=None) == -1
    for fn in (sums, both):
        for dims in ((0, 4, 5, 6), (1, 0, 5, 6), (1, 4, -1, 6), (1, 4, 5, 0), (1, 2048, 2048, 512), (65536, 1, 1, 1)):
            assert fn(dims=dims) == -2, dims
        for L in (0, -1, 257, 1 << 20):
            assert fn(L=L) == -3, L
        full = lib.modet_segdice_ws_bytes(1, 4, 5, 6, 5)
        assert fn(nb=full - 1) == -4 and fn(nb=0) == -4
        assert fn(ws=p + 4) == -4 and fn(ws=p + 2) == -4        # the workspace begins with 64-bit sums


@pytest.mark.parametrize("L", [1, 5, 54])
def test_oracle_on_an_integer_flow_is_one_minus_dice_voi_of_the_nearest_warp(L):
    """what the term is the differentiable form of: on an integer-valued flow the trilinear warp of the one-hot labels is the
    nearest warp of the label map, the sums are voxel counts and the loss is 1 - dice_val_VOI"""
    shape = (1, 6, 7, 9)
    mov, fix = so.make_labels(shape, L, seed=3)
    flow = so.integer_flow(shape, seed=4)
    table, loss = so.table_and_loss(mov, flow, fix, L)
    warped = orc.warp(mov.double(), flow.double(), mode="nearest")
    want = 1.0 - orc.dice_voi(warped, fix.double(), nlabels=L)
    assert abs(float(loss) - want) <= 1e-12, (float(loss), want)
    assert bool((table == table.round()).all()) and float(table[:, :, 0].abs().max()) == 0.0
    for l in range(1, L + 1):
        assert float(table[0, 1, l]) == float((warped == l).sum()) and float(table[0, 2, l]) == float((fix == l).sum())
        assert float(table[0, 0, l]) == float(((warped == l) & (fix == l)).sum())
    a = so.absent_label(L)
    if a is not None:                                          # absent on both sides: dsc = 0, not NaN
        assert float(table[0, :, a].abs().max()) == 0.0 and bool(torch.isfinite(loss))


def test_shared_inputs_hold_what_the_gpu_tests_rely_on():
    for shape in so.SHAPES:
        B, D, H, W = shape
        f = so.lattice_flow(shape, seed=11)
        assert bool((f * 16 == (f * 16).round()).all()) and not bool((f == f.round()).any())
        assert float(f.min()) >= -3.0 and float(f.max()) <= 3.0 + 15 / 16
        p = so.positions(f)
        for a, n in enumerate((D, H, W)):                      # near every face: wholly and partly outside
            pa = p[:, a]
            assert bool((pa < -1).any()) and bool(((pa > -1) & (pa < 0)).any()), (shape, a)
            assert bool((pa > n).any()) and bool(((pa > n - 1) & (pa < n)).any()), (shape, a)
        g = so.general_flow(shape, seed=12)
        frac = so.positions(g) - so.positions(g).floor()
        assert float(frac.min()) >= 1e-3 and float(frac.max()) <= 1 - 1e-3     # no voxel within 1e-3 of a kink
        for L in so.LABELS:
            mov, fix = so.make_labels(shape, L, seed=13)
            assert mov.dtype == fix.dtype == torch.int16 and mov.shape == fix.shape == (B, 1, D, H, W)
            for lab in (mov, fix):
                for h in so.hostile(L):
                    assert bool((lab == h).any()), (shape, L, h)
                if so.absent_label(L) is not None:
                    assert not bool((lab == so.absent_label(L)).any())


class _Fake:
    """what the argument checks look at first, for the refusals on a machine without a GPU"""
    is_cuda = True

    def __init__(self, dtype, shape=(1, 1, 4, 5, 6)):
        self.dtype, self.shape = dtype, shape

    def is_contiguous(self):
        return True

    def dim(self):
        return len(self.shape)


def test_python_side_refusals_are_raised_by_name(monkeypatch):
    from smilecode_amd import _lib, losses, ops
    px = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES["segdice"][1], segments=lambda: [], refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    lab = torch.zeros(1, 1, 4, 5, 6, dtype=torch.int16)
    flow, flow_cl = torch.zeros(1, 3, 4, 5, 6), torch.zeros(1, 4, 5, 6, 3)
    for fn, f in ((ops.seg_dice_loss, flow), (ops.seg_dice_sums, flow)):
        with pytest.raises(RuntimeError, match="GPU"):         # no CPU fallback: a host tensor is an error, not a slow path
            fn(lab, f, lab, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.seg_dice_value_and_grad_cl(flow_cl, lab, lab, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        losses.LabelDice(5)(flow, lab, lab)
    for bad in (0, -1, 257, 5.0, True, None, "5"):
        with pytest.raises(RuntimeError, match="nlabels"):
            ops.seg_dice_loss(lab, flow, lab, bad)
        with pytest.raises(RuntimeError, match="nlabels"):
            losses.LabelDice(bad)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.float32):
        with pytest.raises(RuntimeError, match=r"mov_lab must be int16.*convert"):
            ops._segdice_args("seg_dice_loss", _Fake(dt), flow, _Fake(torch.int16), 5, False)
        with pytest.raises(RuntimeError, match=r"fix_lab must be int16.*convert"):
            ops._segdice_args("seg_dice_loss", _Fake(torch.int16), flow, _Fake(dt), 5, False)
    with pytest.raises(RuntimeError, match="float32"):
        ops._segdice_args("seg_dice_loss", _Fake(torch.int16), _Fake(torch.float64, (1, 3, 4, 5, 6)), _Fake(torch.int16), 5, False)
    # the shapes, with the device and dtype checks out of the way
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for m, f in ((lab[0], lab), (lab, lab[0]), (torch.zeros(1, 2, 4, 5, 6, dtype=torch.int16), lab), (lab[:0], lab[:0])):
        with pytest.raises(RuntimeError, match=r"\(B,1,D,H,W\)"):
            ops.seg_dice_loss(m, flow, f, 5)
    with pytest.raises(RuntimeError, match="does not match"):
        ops.seg_dice_loss(lab, flow, torch.zeros(1, 1, 4, 5, 7, dtype=torch.int16), 5)
    for bad in (flow_cl, flow[0], torch.zeros(1, 2, 4, 5, 6), torch.zeros(2, 3, 4, 5, 6), torch.zeros(1, 3, 4, 5, 7)):
        with pytest.raises(RuntimeError, match=r"planar \(B,3,D,H,W\)"):
            ops.seg_dice_loss(lab, bad, lab, 5)
        with pytest.raises(RuntimeError, match=r"planar \(B,3,D,H,W\)"):
            ops.seg_dice_sums(lab, bad, lab, 5)
    for bad in (flow, flow_cl[0], torch.zeros(1, 4, 5, 6, 2), torch.zeros(1, 4, 5, 7, 3)):
        with pytest.raises(RuntimeError, match=r"channels-last \(B,D,H,W,3\)"):
            ops.seg_dice_value_and_grad_cl(bad, lab, lab, 5)
        with pytest.raises(RuntimeError, match=r"channels-last \(B,D,H,W,3\)"):
            ops.seg_dice_sums(lab, bad, lab, 5, channels_last=True)
    with pytest.raises(RuntimeError, match="d_flow_add"):
        ops.seg_dice_value_and_grad_cl(flow_cl, lab, lab, 5, d_flow_add=torch.zeros(1, 4, 5, 6, 1))
    for bad in (flow_cl, flow[0], torch.zeros(1, 2, 4, 5, 6)):
        with pytest.raises(RuntimeError, match="LabelDice"):
            losses.LabelDice(5)(bad, lab, lab)
    assert not [n for n, _ in px.records if guard.is_launching(n)]


def test_trainer_takes_a_label_term_and_refuses_what_is_not_built():
    from smilecode_amd import engine, losses

    class WithCl(torch.nn.Linear):
        def forward_cl(self, a, b):
            raise AssertionError("not called here")

    assert losses.SEG_TERMS == {"dice": losses.LabelDice} and losses.LabelDice().nlabels == 54
    plain = engine.Trainer(WithCl(3, 2))
    assert plain.seg is None and plain._seedable()
    tr = engine.Trainer(WithCl(3, 2), seg=losses.LabelDice(7), seg_weight=0.5)
    assert tr.seg.nlabels == 7 and tr.seg_weight == 0.5 and tr._seedable() and losses.seeds(tr.seg)

    class Sub(losses.LabelDice):
        pass
    assert not engine.Trainer(WithCl(3, 2), seg=Sub(7))._seedable()          # exact types only, as for the other terms
    with pytest.raises(RuntimeError, match="overlap_allreduce"):
        engine.Trainer(WithCl(3, 2), seg=losses.LabelDice(7), overlap_allreduce=True)
    x = torch.zeros(1, 1, 4, 4, 4)
    lab = torch.zeros(1, 1, 4, 4, 4, dtype=torch.int16)
    for call in (lambda t, **kw: t.train_step(x, x, **kw), lambda t, **kw: t.capture(x, x, **kw), lambda t, **kw: t.loss(x, x, **kw)):
        with pytest.raises(RuntimeError, match="needs labels"):
            call(tr)
        with pytest.raises(RuntimeError, match="needs labels"):
            call(tr, labels=(lab,))
        with pytest.raises(RuntimeError, match="no seg term"):
            call(plain, labels=(lab, lab))


def test_train_flags():
    from smilecode_amd import train
    ap = train.make_parser()
    a = train.check_model_args(ap, ap.parse_args([]))
    assert a.seg is None and a.seg_weight == 1 and a.seg_labels == 54
    heads, hd = [8, 4, 2, 1, 1], 6
    base = train.save_dir_name(a, heads, hd, [1, 1])
    a = train.check_model_args(ap, ap.parse_args(["--seg", "dice", "--seg-weight", "0.25", "--seg-labels", "32"]))
    assert a.seg == "dice" and a.seg_weight == 0.25 and a.seg_labels == 32
    assert train.save_dir_name(a, heads, hd, [1, 1]) == base        # checkpoints and their directory are unchanged
    for bad in (["--seg", "jaccard"], ["--seg", "dice", "--overlap-allreduce"], ["--seg", "dice", "--seg-labels", "0"],
                ["--seg", "dice", "--seg-labels", "257"]):
        with pytest.raises(SystemExit):
            train.check_model_args(ap, ap.parse_args(bad))
