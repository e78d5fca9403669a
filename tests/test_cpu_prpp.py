"""The PR++ family without a GPU: the header of the family against its ctypes table and the library's exports, the header as C99, the
workspace sizes, what the GPU tests assume about their CPU oracle (tests/prpp_oracle.py): the cross-grid composition is not
upsample-then-warp and reduces to warp + add on equal grids, the exactness lattice is exact -- and the network: the oracle
against the reference's golden run, the state-dict keys, a checkpoint round trip, every refusal, the scripts' model switch."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import modet_torch as mt
from tests import prpp_oracle as orc
from tests.guard_family import check_family_table, check_header_is_c99
from tests.util import GOLD, gold, rel_err

NAMES = {"modet_prpp_upcat_fwd", "modet_prpp_upcat_bwd", "modet_prpp_relu_fwd", "modet_prpp_relu_add_fwd", "modet_prpp_relu_bwd",
         "modet_prpp_stack_ws_bytes", "modet_prpp_stack_fwd", "modet_prpp_stack_bwd", "modet_prpp_compose_ws_bytes",
         "modet_prpp_compose_fwd", "modet_prpp_compose_bwd"}
QUERIES = {"modet_prpp_stack_ws_bytes", "modet_prpp_compose_ws_bytes"}


def test_prpp_header_table_and_exports_agree():
    from smilecode_amd import build
    lib = check_family_table("prpp", NAMES, sorted(NAMES - QUERIES))
    assert lib.modet_hip_version() == 447                      # a new header changes no existing signature
    assert "prpp.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "prpp.hip"))
    assert os.path.isfile(os.path.join(build.CSRC, "corr3d_internal.h"))          # corr3d's kernels, shared, not copied
    src = open(os.path.join(build.CSRC, "prpp.hip")).read()
    assert "box3_kernel" in src and "__global__ __launch_bounds__(BLK) void box3_kernel" not in src


def test_header_parses_as_c99(tmp_path):
    check_header_is_c99("prpp", tmp_path, "return modet_prpp_stack_ws_bytes(0, 0, 0, 0, MODET_PRPP_MAX_C) + modet_prpp_compose_ws_bytes(0, 0, 0, MODET_PRPP_CORR) != 0;")


def test_workspace_sizes_and_zero_for_refused_arguments():
    from smilecode_amd import _lib, ops
    L = _lib.load()
    sw, cw = L.modet_prpp_stack_ws_bytes, L.modet_prpp_compose_ws_bytes
    for n, (B, (D, H, W), C) in orc.STACK_CASES.items():
        want = 2 * (B * D * H * W * C + B * (D + 2) * (H + 2) * (W + 2) * C) * 4          # pm | pfx | d_pm | d_pfx
        assert sw(B, D, H, W, C) == want == L.modet_corr3d_ws_bytes(B, D, H, W, C), n
    limit = ops._prpp_limit("MODET_PRPP_MAX_C")
    assert limit == 128 and ops._prpp_limit("MODET_PRPP_CORR") == ops.PRPP_CORR == 27
    assert sw(1, 2, 2, 2, limit) > 0 and sw(1, 2, 2, 2, limit + 4) == 0
    for bad in ((1, 2, 2, 2, 6), (1, 2, 2, 2, 0), (0, 2, 2, 2, 8), (1, 0, 2, 2, 8), (1, 2, 2, 0, 8), (1, 1024, 1024, 1024, 8)):
        assert sw(*bad) == 0, bad
    for n, (B, (Dc, Hc, Wc), _) in orc.COMPOSE_CASES.items():
        assert cw(B, Dc, Hc, Wc) == 64 * -(-B // 16) + B * Dc * Hc * Wc * 3 * 8, n
    assert cw(1, 80, 96, 80) == 64 + 80 * 96 * 80 * 24                          # the coarse field of the finest cross-grid composition
    assert cw(17, 1, 2, 2) == 128 + 17 * 4 * 24
    for bad in ((0, 2, 2, 2), (1, 0, 2, 2), (1, 2, 2, 0), (65536, 2, 2, 2)):
        assert cw(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the oracle's operators
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cross_grid_compose_is_not_upsample_then_warp(dtype):
    """a random 2 x 3 x 5 -> 4 x 6 x 10 pair: sampling the coarse field at (p + w) (Sc - 1) / (Sf - 1) against trilinear upsampling
    followed by a same-grid warp (the guard against that 'simplification')"""
    src, w, _ = orc.compose_tensors(1)
    a, b = orc.compose(src.to(dtype), w.to(dtype)), orc.upsample_then_warp(src.to(dtype), w.to(dtype))
    diff = float((a - b).abs().max())
    print("max |compose - upsample_then_warp| =", diff)
    assert a.shape == b.shape == (2, 4, 6, 10, 3) and diff > 1e-2


def test_compose_on_equal_grids_is_warp_plus_add():
    src, w, _ = orc.compose_tensors(4)
    s, f = orc.to_planar(src.double()), orc.to_planar(w.double())
    assert rel_err(orc.compose(src.double(), w.double()), orc.to_cl(mt.warp(s, f) + f)) < 1e-14


def test_compose_is_the_headers_formula():
    """c = (p + w) (Sc - 1) / (Sf - 1) per axis, zeros outside, written out in fp64 against grid_sample as the reference calls it"""
    for n in (1, 2, 3):
        src, w, _ = orc.compose_tensors(n)
        src, w = src.double(), w.double()
        sc, sf = src.shape[1:4], w.shape[1:4]
        grid = torch.stack(torch.meshgrid([torch.arange(s, dtype=torch.float64) for s in sf], indexing="ij"), -1)
        ratio = torch.tensor([(sc[i] - 1) / (sf[i] - 1) for i in range(3)], dtype=torch.float64)
        c = (grid + w) * ratio                                   # coarse coordinates
        # a same-grid warp of the coarse field, evaluated at the coarse points c: express c as displacement from a coarse identity
        # grid is not possible (other size), so sample directly
        c0 = torch.floor(c)
        fr = c - c0
        out = torch.zeros_like(w)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    idx = [c0[..., i].long() + d for i, d in enumerate((dz, dy, dx))]
                    ok = functools.reduce(lambda u, v: u & v, [(idx[i] >= 0) & (idx[i] < sc[i]) for i in range(3)])
                    wt = functools.reduce(lambda u, v: u * v, [fr[..., i] if d else 1 - fr[..., i] for i, d in enumerate((dz, dy, dx))])
                    b = torch.arange(src.shape[0]).reshape(-1, 1, 1, 1).expand_as(ok)
                    val = src[b, idx[0].clamp(0, sc[0] - 1), idx[1].clamp(0, sc[1] - 1), idx[2].clamp(0, sc[2] - 1)]
                    out = out + val * (wt * ok.double()).unsqueeze(-1)
        assert rel_err(out + w, orc.compose(src, w)) < 1e-13, n
        assert orc.outside_share(w, sc) > 0.2, n                 # fields of +-3 voxels: the zero padding is exercised


def test_exactness_lattice_is_exact_in_both_precisions():
    """ratio exactly 1/2, w on the half-integer lattice, integer src and cotangent: fp32 and fp64 ATen agree bit for bit on the
    output and both gradients, so the GPU test may ask the kernels for the same bits"""
    src, w, gy = orc.compose_exact_tensors()
    sc, sf = orc.EXACT_SHAPES
    assert all(sf[i] - 1 == 2 * (sc[i] - 1) for i in range(3))
    c = (torch.tensor([0.0, 0.0, 0.0]) + w[0, 0, 0, 0]) / 2
    assert c.tolist() == [sc[0] - 1.0, sc[1] - 1.0, sc[2] - 1.0]                  # exactly on the last node
    c = (torch.tensor([0.0, 0.0, 1.0]) + w[0, 0, 0, 1]) / 2
    assert c.tolist() == [float(sc[0]), float(sc[1]), float(sc[2])]               # exactly one cell outside
    r32 = orc.value_and_grads(orc.compose, {"src": src, "w": w}, gy, torch.float32)
    r64 = orc.value_and_grads(orc.compose, {"src": src, "w": w}, gy, torch.float64)
    for k in r64:
        assert torch.equal(r32[k].double(), r64[k]) and float(r64[k].abs().max()) > 0, k


def test_oracles_run_in_fp32_near_fp64():
    cases = [(orc.upsample_nearest_cat, dict(zip(("x", "skip"), orc.upcat_tensors(2)[:2])), orc.upcat_tensors(2)[2]),
             (orc.relu_add, dict(zip(("x", "t"), orc.relu_tensors(1027)[:2])), orc.relu_tensors(1027)[2]),
             (orc.corr_stack, dict(zip(("mov", "fix"), orc.stack_tensors(3)[:2])), orc.stack_tensors(3)[2]),
             (orc.compose, dict(zip(("src", "w"), orc.compose_tensors(1)[:2])), orc.compose_tensors(1)[2])]
    for fn, t, g in cases:
        r32, r64 = orc.value_and_grads(fn, t, g, torch.float32), orc.value_and_grads(fn, t, g, torch.float64)
        assert set(r32) == set(r64) == {"out"} | {"d_" + k for k in t}
        for q in r64:
            assert r32[q].dtype == torch.float32 and rel_err(r32[q], r64[q]) < 1e-4, (fn.__name__, q)


def test_relu_cotangent_mask_leaves_nearly_everything():
    """the share of elements within RELU_EPS of the kink (their cotangent is zeroed in the gradient comparisons) stays below 1 %"""
    for n in orc.RELU_SIZES:
        _, t, _ = orc.relu_tensors(n)
        planted = (2 if n >= 3 else 0) + (2 if n >= 1027 else 0)
        near = int((t.abs() < orc.RELU_EPS).sum())
        assert near == planted, (n, near)                        # only the planted zeros
        if n >= 1027:
            assert near / n < 0.01
    x, t, _ = orc.relu_tensors(4)
    t = t.clone().requires_grad_(True)
    torch.relu(t).sum().backward()
    assert t.grad[1] == 0 and t.grad[2] == 0                     # ATen's gradient at +0 and at -0 is 0


# ------------------------------------------------------------------------------------------------ the network
NPZ = "e2e_prpp_32x48x32.npz"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def recorded():
    """tests/golden/REPORT_prpp.txt: quantity -> (max|oracle - reference|, max|reference|) as the generator measured them"""
    out = {}
    for line in open(os.path.join(GOLD, "REPORT_prpp.txt")):
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
    """outputs, the loss and the reference's own stored gradients; THE CONDITION of the generator holds on the oracle too: every
    block's field has max |w| between 0.25 and 1.5 voxels of its own grid, and nothing is analytically zero"""
    g, rec, tag = gold(NPZ), recorded(), "B%d" % B
    stride = int(g["stride"])
    (loss, moved, flow, grads), taps = e2e_oracle(B)
    for name, got in (("flow", flow), ("moved", moved)):
        within_recorded("e2e[%s] %s" % (tag, name), got.reshape(-1)[::stride], T(g["%s.%s" % (tag, name)]), rec)
    within_recorded("e2e[%s] loss" % tag, loss, T(g[tag + ".loss"])[0], rec)
    kept = sorted(n for n in grads if "%s.grad.%s" % (tag, n) in g.files)
    biases = [n for n in grads if n.endswith(".bias")]
    assert set(biases) <= set(kept) and len(kept) > len(biases) and (B == 1 or len(kept) > len(e2e_kept(1)))
    for n in kept:
        within_recorded("e2e[%s] grad %s" % (tag, n), grads[n], T(g["%s.grad.%s" % (tag, n)]), rec)
    for k, (amax, share) in orc.field_conditions(taps).items():
        assert orc.FIELD_RANGE[0] <= amax <= orc.FIELD_RANGE[1], (tag, k, amax)
        assert orc.FIELD_RANGE[0] <= float(g["%s.w%d_absmax" % (tag, k)]) <= orc.FIELD_RANGE[1]
    assert all(float(v.abs().max()) > 1e-9 for v in grads.values()), [n for n, v in grads.items() if float(v.abs().max()) <= 1e-9]


def e2e_kept(B):
    g = gold(NPZ)
    return [k for k in g.files if k.startswith("B%d.grad." % B)]


def test_report_ties_the_oracle_to_the_reference_and_records_the_conditions():
    rec = recorded()
    rng = {k: v for k, v in rec.items() if k.startswith("range[")}
    assert len(rng) == 2 * 5 and all(orc.FIELD_RANGE[0] <= v[1] <= orc.FIELD_RANGE[1] for v in rng.values())
    e2e = {k: v for k, v in rec.items() if k.startswith("e2e[")}
    n_params = len(orc.prpp_shapes(orc.GOLD_CHANNELS))
    assert sum(" grad " in k for k in e2e) == 2 * n_params                    # every gradient of every run is in the report
    assert all(v[0] <= 1e-9 * max(v[1], 1.0) for v in e2e.values())           # the oracle IS the reference
    shares = {k: v[1] for k, v in rec.items() if k.startswith("outside[")}
    assert len(shares) == 2 * 4
    assert max(shares.values()) > 0.0                                          # the zero padding is exercised
    assert max(shares.values()) < 0.25, shares                                 # and the fields are not mostly padding


def _reference_keys(which):
    return json.load(open(os.path.join(GOLD, "prpp_state_dict.json")))[which]


def test_state_dict_keys_are_the_references():
    from smilecode_amd import models
    for which, shape, c in (("PRNetplusplus(32x48x32, first_channel=4)", (32, 48, 32), 4), ("PRNetplusplus(16x16x16, first_channel=8)", (16, 16, 16), 8)):
        want = _reference_keys(which)
        m = models.PRNetplusplus(shape, first_channel=c, legacy_grid_buffers=True)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == want, which
        params = {k: list(v.shape) for k, v in m.named_parameters()}
        assert list(params) == list(orc.prpp_shapes(c)) and params == {k: list(v) for k, v in orc.prpp_shapes(c).items()}
        bare = models.PRNetplusplus(shape, first_channel=c).state_dict()
        assert sorted(bare) == sorted(k for k in want if not k.endswith(".grid")) and len(want) - len(bare) == 7
    for key in ("net.encoder.block1.main.weight", "net.decoder1.Conv.main.weight", "net.decoder5.main.weight", "prblock2.conv1.0.weight",
                "prblock2.conv1.1.bias", "prblock2.conv2.1.weight", "prblock2.flow.weight", "prblock2.stn.grid", "transformers.2.grid"):
        assert key in want, key
    assert want["prblock1.conv1.0.weight"] == [91, 91, 3, 3, 3] and want["prblock5.conv1.0.weight"] == [43, 43, 3, 3, 3]
    m = models.PRNetplusplus((16, 16, 16))
    assert float(m.prblock3.flow.weight.detach().abs().max()) < 1e-3 and float(m.prblock3.flow.bias.detach().abs().max()) == 0.0       # N(0, 1e-5), zero bias


def test_checkpoint_round_trip(tmp_path):
    """a reference-format checkpoint (grid buffers included) loads strictly, and what is saved loads back equal"""
    from smilecode_amd import models
    src = models.PRNetplusplus((16, 32, 16), first_channel=4, legacy_grid_buffers=True)
    path = str(tmp_path / "ck.pth.tar")
    torch.save({"state_dict": src.state_dict()}, path)
    sd = torch.load(path, map_location="cpu")["state_dict"]
    assert torch.equal(sd["transformers.1.grid"][0, 1, 0, :, 0], torch.arange(16.0)) and tuple(sd["prblock2.stn.grid"].shape) == (1, 3, 4, 8, 4)
    dst = models.PRNetplusplus((16, 32, 16), first_channel=4)
    res = dst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (n, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        assert torch.equal(a, b), n
    assert not any(k.endswith(".grid") for k in dst.state_dict())


def test_every_refusal_names_its_argument():
    from smilecode_amd import models
    P = models.PRNetplusplus
    for kw, word in (({"first_channel": 6}, "first_channel = 6"), ({"first_channel": 0}, "first_channel = 0"), ({"first_channel": 32}, "first_channel = 32"),
                     ({"act_dtype": torch.bfloat16}, "act_dtype"), ({"diff": True}, "diff"), ({"overlap_allreduce": True}, "overlap_allreduce"),
                     ({"in_channel": 0}, "in_channel"), ({"size": (32, 40, 32)}, "multiple of 16"), ({"size": (32, 0, 32)}, "multiple of 16"),
                     ({"size": (32, 32)}, "D, H, W")):
        with pytest.raises(RuntimeError, match=word):
            P(**{"size": (32, 32, 32), "first_channel": 4, **kw})
    for c in (4, 8, 16, 28):
        assert models.prpp_unsupported_config(1, c) is None
    assert "28" in models.prpp_unsupported_config(1, 32) and P.unsupported_shape((160, 192, 160)) is None and P.unsupported_shape((16, 32, 16)) is None
    m = P((16, 16, 16), first_channel=4)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        m(torch.zeros(1, 1, 16, 24, 16), torch.zeros(1, 1, 16, 24, 16))
    with pytest.raises(RuntimeError, match="same shape"):
        m(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 32))
    with pytest.raises(RuntimeError, match="kernel_size"):
        models.PRplusplusBlock((4, 4, 4), 8, kernel_size=5)
    with pytest.raises(RuntimeError, match="stride"):
        models.ConvBlockReLU(4, 4, stride=3)


def test_train_and_infer_take_the_model_switch():
    from smilecode_amd import infer, train
    ap = train.make_parser()
    args = train.check_model_args(ap, ap.parse_args(["--model", "prpp"]))
    assert args.channels == 8                                               # PRNetplusplus's own default, not the other baselines' 16
    m = train.make_model(args, (16, 16, 16), training=True)
    assert type(m).__name__ == "PRNetplusplus" and m.channels == 8 and m.stage_buckets is False and hasattr(m, "forward_cl")
    assert train.save_dir_name(args, [8, 4, 2, 1, 1], 6, [1, 1]) == "PRNetplusplus_ncc_1_reg_1_lr_0.0001_54r/"
    assert args.lr == 0.0001
    a4 = train.check_model_args(ap, ap.parse_args(["--model", "prpp", "--channels", "4"]))
    assert a4.channels == 4 and train.make_model(a4, (16, 16, 16)).channels == 4
    assert train.check_model_args(ap, ap.parse_args(["--model", "pcnet"])).channels == 16 and "prpp" in train.MODELS
    for bad in (["--model", "prpp", "--diff"], ["--model", "prpp", "--overlap-allreduce"]):
        with pytest.raises(SystemExit):
            train.check_model_args(ap, ap.parse_args(bad))
    ip = infer.make_parser()
    ia = train.check_model_args(ip, ip.parse_args(["--model", "prpp"]))
    assert ia.model == "prpp" and ia.channels == 8
    assert ip.parse_args(["--model", "prpp", "--channels", "4"]).channels == 4
