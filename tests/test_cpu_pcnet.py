"""The PCNet family without a GPU: the header of the family against its ctypes table and the library's exports, the header as C99,
the workspace sizes, and what the GPU tests of the four operators assume about their CPU oracle (tests/pcnet_oracle.py): the ATen
compositions run in fp32 and fp64, x4 is not x2 twice, the align_corners cell rule of the header written out, ATen's tie rule of
the max pool, and the argmax condition of every planted case."""
import os

import pytest
import torch

from tests import pcnet_oracle as orc
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import rel_err

NAMES = {"modet_pcnet_upsample_fwd", "modet_pcnet_upsample_bwd", "modet_pcnet_dfi_gate_fwd", "modet_pcnet_dfi_gate_bwd",
         "modet_pcnet_nff_ws_bytes", "modet_pcnet_nff_pool", "modet_pcnet_nff_gate_fwd", "modet_pcnet_nff_gate_bwd",
         "modet_pcnet_nff_apply_fwd", "modet_pcnet_nff_apply_bwd_gate", "modet_pcnet_nff_apply_bwd", "modet_pcnet_add"}


def test_pcnet_header_table_and_exports_agree():
    from smilecode_amd import build
    lib = check_family_table("pcnet", NAMES, sorted(NAMES - {"modet_pcnet_nff_ws_bytes"}))
    assert lib.modet_hip_version() == 447                      # a new header changes no existing signature
    assert "pcnet.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "pcnet.hip"))


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("pcnet", tmp_path, "return modet_pcnet_nff_ws_bytes(0, 0, MODET_PCNET_MAX_C, MODET_PCNET_NFF_PASS_POOL) != 0;")


def test_workspace_sizes_and_zero_for_refused_arguments():
    from smilecode_amd import _lib, ops
    ws = _lib.load().modet_pcnet_nff_ws_bytes
    for n, (B, shape, C) in orc.NFF_CASES.items():
        V = shape[0] * shape[1] * shape[2]
        chunk = max(1024, -(-V // 1024))
        rows = -(-V // chunk)
        assert ws(B, V, C, 0) == B * rows * 3 * C * 16 and ws(B, V, C, 1) == B * rows * 3 * C * 8, n
        assert ws(B, V, C, 2) == B * (3 * C + 4 * (3 * C // 8)) * 4, n
    assert ws(1, 160 * 192 * 160, 64, 0) == 1024 * 192 * 16                      # the default network's widest NFF: 3 MiB
    limit = ops._lib_limit("MODET_PCNET_MAX_C")
    assert limit == 256 and ws(1, 12, limit, 0) > 0 and ws(1, 12, limit + 4, 0) == 0
    for bad in ((1, 12, 6, 0), (1, 12, 0, 0), (1, 12, 8, 3), (1, 12, 8, -1), (0, 12, 8, 0), (1, 0, 8, 0), (65536, 12, 8, 0), (1, 2 ** 31, 8, 0)):
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_by_4_is_not_twice_by_2(dtype):
    """align_corners=True: x4 samples at o (n - 1) / (4 n - 1), x2 twice at points of the x2 grid -- different functions (the
    guard against that 'simplification'; 0.76 on this field)"""
    x = orc.up_tensors(1)[0].to(dtype)
    four, twice = orc.upsample_pow2(x, 4), orc.upsample_pow2(orc.upsample_pow2(x, 2), 2)
    assert four.shape == twice.shape == (1, 8, 12, 20, 3) and float((four - twice).abs().max()) > 0.1


@pytest.mark.parametrize("n", sorted(orc.UP_CASES))
def test_the_headers_cell_rule_is_atens_upsampling(n):
    """quotient and remainder of o (n - 1) by f n - 1, written out in fp64, against F.interpolate in fp64"""
    x = orc.up_tensors(n)[0].double()
    B, (d, h, w), f = orc.UP_CASES[n]

    def axis(t, dim, n_in):
        den = f * n_in - 1
        o = torch.arange(f * n_in)
        q, r = (o * (n_in - 1)) // den, (o * (n_in - 1)) % den
        q1 = torch.clamp(q + 1, max=n_in - 1)
        frac = (r.double() / den).reshape([-1 if i == dim else 1 for i in range(5)])
        return t.index_select(dim, q) * (1 - frac) + t.index_select(dim, q1) * frac

    got = axis(axis(axis(x, 1, d), 2, h), 3, w)
    assert rel_err(got, orc.upsample_pow2(x, f)) < 1e-14
    assert torch.equal(got[:, ::f * d - 1, ::f * h - 1, ::f * w - 1], x[:, ::d - 1, ::h - 1, ::w - 1])          # corners, exactly


def test_oracles_run_in_fp32_near_fp64():
    x, gy = orc.up_tensors(2)
    for fn, t, g in ((lambda v: orc.upsample_pow2(v, 4), {"x": x}, gy),
                     (orc.dfi_gate, dict(zip(("x", "logits"), orc.dfi_tensors(3)[:2])), orc.dfi_tensors(3)[2]),
                     (orc.nff_fuse, dict(zip(orc.NFF_NAMES, orc.nff_tensors(3)[:6])), orc.nff_tensors(3)[6])):
        r32, r64 = orc.value_and_grads(fn, t, g, torch.float32), orc.value_and_grads(fn, t, g, torch.float64)
        assert set(r32) == set(r64) == {"out"} | {"d_" + k for k in t}
        for q in r64:
            assert r32[q].dtype == torch.float32 and 0 < rel_err(r32[q], r64[q]) < 1e-4, q


def test_dfi_gate_is_the_references_loop():
    x, lg, _ = orc.dfi_tensors(3)
    x, lg = x.double(), lg.double()
    want = sum(x[..., 3 * i:3 * i + 3] * torch.sigmoid(lg[..., 3 * i:3 * i + 3]) for i in range(3))
    assert torch.equal(orc.dfi_gate(x, lg), want) and want.shape == (2, 5, 7, 9, 3)


def test_aten_max_pool_sends_a_tie_to_the_first_voxel():
    """the rule the kernels follow (lowest voxel index among equal maxima), on ATen itself and through the oracle"""
    v = torch.zeros(1, 1, 2, 3, 2, dtype=torch.float64)
    v.view(-1)[3] = v.view(-1)[8] = 5.0
    v.requires_grad_(True)
    torch.nn.functional.adaptive_max_pool3d(v, 1).sum().backward()
    assert v.grad.view(-1).nonzero().flatten().tolist() == [3]
    for n in (3, 6):
        t = orc.nff_tensors(n, plant="tie")
        V = t[0][0, ..., 0].numel()
        lo, hi = orc.TIE_AT(V)
        for dtype in (torch.float32, torch.float64):
            cat = orc.nff_cat(*(u.to(dtype) for u in t[:4])).reshape(t[0].shape[0], -1, V)
            assert bool((cat[:, 0, lo] == cat[:, 0, hi]).all()) and bool((cat[:, 0].argmax(-1) == lo).all()), (n, dtype)


@pytest.mark.parametrize("n", sorted(orc.NFF_CASES))
def test_every_planted_case_meets_the_argmax_condition(n):
    """(top1 - top2) / |top1| of every (sample, channel) is at least 100 x ATen fp32's relative error on the pooled tensor; plain
    randn does not meet it at V = 9600 (gaps down to 1e-5 and below), the planted factor of 1.5 leaves a gap of a third"""
    t0, t1, t2, lg = orc.nff_tensors(n)[:4]
    gaps = orc.nff_gaps(t0, t1, t2, lg)
    e_cat = rel_err(orc.nff_cat(t0, t1, t2, lg), orc.nff_cat(*(t.double() for t in (t0, t1, t2, lg))))
    assert float(gaps.min()) >= 100.0 * e_cat and float(gaps.min()) > 0.3, (n, float(gaps.min()), e_cat)
    assert float(gaps.min()) >= 1 - 1 / orc.PLANT - 1e-5          # the winner is 1.5 x the old maximum, the runner-up at most that
    *t, gy = orc.nff_tensors(n)
    ref = orc.value_and_grads(orc.nff_fuse, dict(zip(orc.NFF_NAMES, t)), gy, torch.float64)
    assert all(float(v.abs().max()) > 1e-6 for v in ref.values()), {k: float(v.abs().max()) for k, v in ref.items()}
    a32 = orc.nff_cat(t0, t1, t2, lg).flatten(2).argmax(-1)
    a64 = orc.nff_cat(*(t.double() for t in (t0, t1, t2, lg))).flatten(2).argmax(-1)
    assert torch.equal(a32, a64)


# ------------------------------------------------------------------------------------------------ the network
import functools  # noqa: E402
import json  # noqa: E402

import numpy as np  # noqa: E402

from tests.util import GOLD, gold  # noqa: E402

NPZ = "e2e_pcnet_32x48x32.npz"
N_GOLD_GRADS = 67          # every bias, fc, weight_conv and reg_conv weight and both encoders' first convolution


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def recorded():
    """tests/golden/REPORT_pcnet.txt: quantity -> (max|oracle - reference|, max|reference|) as the generator measured them"""
    out = {}
    for line in open(os.path.join(GOLD, "REPORT_pcnet.txt")):
        if line.startswith("#") or not line.strip():
            continue
        name, err, mag = line.rstrip("\n").split("\t")
        out[name] = (float(err), float(mag))
    return out


def within_recorded(name, got, want, rec):
    """10 x the recorded deviation (another summation order or thread count); where the generator measured less, what another
    order of an n-term fp64 sum can move: n * 2^-53 of the recorded maximum, n = 2 x 49 152 voxels for the longest sums here"""
    err, mag = rec[name]
    dev = float((got.double() - want.double()).abs().max())
    bound = max(10.0 * err, 98304 * 2.0 ** -53 * max(mag, 1.0))
    assert dev <= bound, (name, dev, err, bound)


@functools.lru_cache(maxsize=None)
def e2e_oracle(B):
    mov, fix = orc.golden_pair()
    taps = {}
    return orc.net_value_and_grads(orc.golden_weights(), mov[:B], fix[:B], torch.float64, taps), taps


def test_the_seeded_pair_is_the_generators():
    g = gold(NPZ)
    mov, fix = orc.golden_pair()
    stride = int(g["stride"])
    assert tuple(mov.shape) == (2, 1) + orc.GOLD_SHAPE == tuple(fix.shape) and tuple(g["shape"]) == orc.GOLD_SHAPE
    assert int(g["seed"]) == orc.GOLD_SEED and int(g["channels"]) == orc.GOLD_CHANNELS
    assert torch.equal(mov.reshape(-1)[::stride], T(g["moving"])) and torch.equal(fix.reshape(-1)[::stride], T(g["fixed"]))
    assert float(mov.double().sum()) == float(g["pair_sum"][0]) and float(fix.double().sum()) == float(g["pair_sum"][1])


@pytest.mark.parametrize("B", [1, 2])
def test_oracle_network_equals_the_reference_golden(B):
    """outputs, the three warping fields, the integrated last prediction, the loss and the reference's own gradients (B = 1 and the
    B = 2 ones the GPU tests do not reach); THE CONDITIONS of the generator hold: every field is of the order of a voxel, every
    pooled channel's two largest values are at least 100 x ATen fp32's error apart, nothing is analytically zero"""
    g, rec, tag = gold(NPZ), recorded(), "B%d" % B
    stride = int(g["stride"])
    (loss, moved, flow, grads), taps = e2e_oracle(B)
    named = [("flow", flow), ("moved", moved)] + [(k, taps[k]) for _, k in orc.FIELD_TAPS]
    for name, got in named:
        within_recorded("e2e[%s] %s" % (tag, name), got.reshape(-1)[::stride], T(g["%s.%s" % (tag, name)]), rec)
    within_recorded("e2e[%s] loss" % tag, loss, T(g[tag + ".loss"])[0], rec)
    kept = sorted(n for n in grads if "%s.grad.%s" % (tag, n) in g.files)
    assert len(kept) == N_GOLD_GRADS
    for n in kept:
        within_recorded("e2e[%s] grad %s" % (tag, n), grads[n], T(g["%s.grad.%s" % (tag, n)]), rec)
    for _, k in orc.FIELD_TAPS:
        assert orc.FIELD_RANGE[0] <= float(taps[k].abs().max()) <= orc.FIELD_RANGE[1], (tag, k)
        assert orc.FIELD_RANGE[0] <= float(g["%s.%s_absmax" % (tag, k)]) <= orc.FIELD_RANGE[1]
    weights = [n for n in grads if not n.endswith(".bias")]
    assert all(float(grads[n].abs().max()) > 1e-9 for n in weights), [n for n in weights if float(grads[n].abs().max()) <= 1e-9]


def test_golden_run_meets_the_argmax_condition():
    """recomputed here on the oracle (the generator measured it on the reference itself): per NFF block the smallest gap between a
    pooled channel's two largest values against 100 x the fp32 run's relative error on that tensor, B = 1 and B = 2"""
    mov, fix = orc.golden_pair()
    lines = [ln for ln in open(os.path.join(GOLD, "REPORT_pcnet.txt")) if ln.startswith("gap[")]
    assert len(lines) == 6
    for ln in lines:
        _, gap, err = ln.rstrip("\n").rsplit("\t", 2)
        assert float(gap) >= 100.0 * float(err), ln
    for B in (1, 2):
        for k, (gap, err) in orc.argmax_condition(orc.golden_weights(), mov[:B], fix[:B]).items():
            assert gap >= 100.0 * err, (B, k, gap, err)


def test_report_records_the_field_range_of_every_run():
    rec = recorded()
    rng = {k: v for k, v in rec.items() if k.startswith("range[")}
    assert len(rng) == 2 * 4
    assert all(orc.FIELD_RANGE[0] <= v[1] <= orc.FIELD_RANGE[1] for v in rng.values())
    assert all(v[0] <= 1e-9 * max(v[1], 1.0) for k, v in rec.items() if k.startswith("e2e["))      # the oracle IS the reference


def _reference_keys(which):
    return json.load(open(os.path.join(GOLD, "pcnet_state_dict.json")))[which]


def test_state_dict_keys_are_the_references():
    from smilecode_amd import models
    for which, shape, c in (("PCNet(32x48x32, channels=4)", (32, 48, 32), 4), ("PCNet(16x16x16, channels=16)", (16, 16, 16), 16)):
        want = _reference_keys(which)
        m = models.PCNet(shape, channels=c, legacy_grid_buffers=True)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == want, which
        params = {k: list(v.shape) for k, v in m.named_parameters()}
        assert list(params) == list(orc.pcnet_shapes(c)) and params == {k: list(v) for k, v in orc.pcnet_shapes(c).items()}
        bare = models.PCNet(shape, channels=c).state_dict()
        assert sorted(bare) == sorted(k for k in want if not k.endswith(".grid")) and len(want) - len(bare) == 8
    for key in ("encoder_float.conv1.0.weight", "encoder_float.conv1.1.block.2.weight", "conv_bottleNeck.0.main.weight",
                "dfi_1.conv.0.main.weight", "dfi_1.weight_conv.0.0.weight", "nff_2.weight_conv.0.weight",
                "nff_2.channel_attention.fc.0.weight", "nff_2.channel_attention.fc.2.weight", "upconv2.upconv.weight",
                "reg_conv0.0.weight", "dfi_2.integrate.transformer.grid", "transformer_out.grid"):
        assert key in want, key
    assert want["dfi_0.conv.0.main.weight"] == [48, 9, 3, 3, 3] and want["dfi_2.conv.1.main.weight"] == [16, 16, 3, 3, 3]      # channel = 16 always


def test_checkpoint_round_trip(tmp_path):
    """a reference-format checkpoint (grid buffers included) loads strictly, and what is saved loads back equal"""
    from smilecode_amd import models
    src = models.PCNet((16, 24, 16), channels=4, legacy_grid_buffers=True)
    path = str(tmp_path / "ck.pth.tar")
    torch.save({"state_dict": src.state_dict()}, path)
    sd = torch.load(path, map_location="cpu")["state_dict"]
    assert torch.equal(sd["transformer_1.grid"][0, 1, 0, :, 0], torch.arange(12.0))
    dst = models.PCNet((16, 24, 16), channels=4)
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (n, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        assert torch.equal(a, b), n
    assert not any(k.endswith(".grid") for k in dst.state_dict())


def test_every_refusal_names_its_argument():
    from smilecode_amd import models
    P = models.PCNet
    for kw, word in (({"channels": 6}, "channels = 6"), ({"channels": 20}, "channels = 20"), ({"channels": 0}, "channels = 0"),
                     ({"channels": 2}, "channels = 2"), ({"act_dtype": torch.bfloat16}, "act_dtype"),
                     ({"overlap_allreduce": True}, "overlap_allreduce"), ({"in_channel": 0}, "in_channel"),
                     ({"inshape": (32, 36, 32)}, "multiple of 8"), ({"inshape": (32, 8, 32)}, "at least 16"), ({"inshape": (32, 32)}, "D, H, W")):
        with pytest.raises(RuntimeError, match=word):
            P(**{"inshape": (32, 32, 32), "channels": 4, **kw})
    for c in (4, 8, 12, 16):
        assert models.pcnet_unsupported_config(1, c) is None
    assert "16" in models.pcnet_unsupported_config(1, 20) and P.unsupported_shape((160, 192, 160)) is None
    m = P((16, 16, 16), channels=4)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        m(torch.zeros(1, 1, 16, 20, 16), torch.zeros(1, 1, 16, 20, 16))
    with pytest.raises(RuntimeError, match="same shape"):
        m(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 24))
    with pytest.raises(RuntimeError, match="kernel_size"):
        models.UpConvInsBlock(4, 4, 3, 2)
    with pytest.raises(RuntimeError, match="reduction"):
        models.ChannelAttention(24, 4)


def test_train_and_infer_take_the_model_switch():
    from smilecode_amd import infer, train
    ap = train.make_parser()
    args = train.check_model_args(ap, ap.parse_args(["--model", "pcnet", "--channels", "8"]))
    m = train.make_model(args, (16, 16, 16), training=True)
    assert type(m).__name__ == "PCNet" and m.channels == 8 and m.stage_buckets is False
    assert train.save_dir_name(args, [8, 4, 2, 1, 1], 6, [1, 1]) == "PCnet_ncc_1_reg_1_lr_0.0001_54r/"
    for bad in (["--model", "pcnet", "--diff"], ["--model", "pcnet", "--overlap-allreduce"]):
        with pytest.raises(SystemExit):
            train.check_model_args(ap, ap.parse_args(bad))
    ia = infer.make_parser().parse_args(["--model", "pcnet", "--channels", "4"])
    assert ia.model == "pcnet" and ia.channels == 4
