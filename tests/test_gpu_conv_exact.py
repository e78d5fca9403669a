"""-m gpu: the exact-f32 MFMA convolution kernels (csrc/conv3d.hip, kernel family 0) where the networks reach them, against ATen
fp64 on the CPU (F.conv3d, torch.nn.grad.conv3d_input, torch.nn.grad.conv3d_weight), measured in units of the error ATen fp32
makes on the same case.

THE RULE (tests/test_gpu_convs2.py's and tests/test_gpu_deconv.py's): per quantity, HIP's max|got - ref| / max|ref| against fp64
is at most A = 4 times ATen fp32's (CPU) on the same case; for a batch that repeats one sample "the same case" is the one sample.
Every figure, HIP's and ATen's, goes to the parity report (tests.util.note_many) before it is asserted.  The bit-for-bit and
run-to-run asserts have no tolerance.  Every case first asserts, through modet_conv3d_kernel_family_v, that each pass it checks
takes family 0, and that the launch falls in the plan class (tests/conv_layers.py: fwd_class / wgrad_class) the case is there
for: a later routing or planning change fails the test instead of silently testing another kernel.

FIXED TOLERANCES.  Measured on the MI355X, five quantities exceed A = 4 on some case -- the worst ratios to ATen fp32:
  a. y_act 5.24 (91->32, B = 164);  b. y 5.42 (59->16), d_x 6.54 (59->59);  c. d_w 4.41 (6->32, B = 274), d_b 4.84 (3->16).
HIP's error is 0.5e-6 .. 2.0e-6 of the tensor's maximum in all of them and grows with sqrt(Cin); ATen's stays at 2e-7 .. 6e-7.
Only the summation order differs: conv3d_mfma_kernel feeds v_mfma_f32_16x16x4_f32 unsplit fp32 operands and keeps ONE fp32
accumulator per output over all 27 * Cin / 4 steps of its (channel stage, tap, channel quad) loop -- a chain of 27 * 59 / 4 = 398
dependent additions at Cin = 59 -- and conv3d_wgrad_kernel one per (tap, ci, co) over every voxel of the tiles its workgroup walks
(d_b is tap 27 of that sum with A = 1), where ATen's GEMMs block K and its sum is pairwise.  The proof is in the tests: on integer
data in [-3, 3], where every product and every partial sum is exact in fp32 whatever the order, all three passes of every case of
a, b and c equal the fp64 result BIT FOR BIT.  So, as the rule's author laid down for this outcome, A is not raised: those five
quantities are asserted at test_conv_vs_oracle's fixed tolerances (FIXED) in every case, their figures are still written to the
parity report, and the other quantities (z, y_norm, z_norm: worst 2.28) keep the rule.  (Where a weight gradient sums k copies of
one sample, its reference and its absolute tolerance are the one sample's times k: fixed_tol.)

THREE WAYS lead to the family (csrc/conv3d.hip route_conv / route_wgrad):
 a. a fused LeakyReLU (variant 1), at any size: ACT_CASES.  The 46 instantiations conv3d_mfma_kernel<cfg, vector loads, several
    channel stages, P rows packed> that a plain launch can reach each have a case (cfg 0: 2 x 2 x 3; cfg 4: 2 x 1 x 3, its Cin <= 4
    is one stage; cfg 1, 2, 3, 5, 6, 7, 8: 2 x 2): test_every_reachable_forward_instantiation_has_a_case counts them.
 b. more than 6 000 000 voxels in one launch (the channel-quad kernel bows out): one 9x11x37 sample (3 663 voxels, ragged against
    every tile, below the z-march's 4 096) repeated B = 1 639 times on the device.  Plain forward, normalised input (Cin % 4 == 0)
    and the data gradient -- the pass that runs pack_weights_kernel's mode 1 with P = 2 and 4 (test_prepacked_weights_equal_per_
    launch_packing: pack_weights_many_kernel gives the same bits).  Sample 0 is held against fp64,
    every other sample must equal it bit for bit.  The fused statistics need B <= 32 (modet_conv3d_stats_bytes), so they are
    reached with 32 copies of a 47x50x80 sample: STAT_CASES, the ST (staged epilogue, Cout 4 / 8 / 16) and XF (direct-store
    epilogue, lazily normalised input) instantiations of cfg 0 .. 4.  Statistics rows are per (sample, workgroup), so there the 32
    samples are all held against fp64 and only the two calls against each other.
 c. the weight gradient of a layer with Cin < 4, or with a channel count that is no multiple of 4 and Cout > 16: WGRAD_CASES,
    conv3d_wgrad_kernel<4 | 8 | 16, 2> at B = 2 and <4, 4>, <8, 4> on 274 copies of the sample (>= 1 000 000 voxels).

THE IMAGE LAYERS (Cin = 1) report family 0 in every pass and have kernels of their own: IMAGE_CASES, PCNet's 1->16 on the tiles,
PR++'s 1->8 on conv_c1_fwd_kernel<8>, ModeT's 1->4 + LeakyReLU on conv_c1_march_kernel (from 500 000 voxels per sample on) with
conv_c1_wgrad_mfma_kernel; forward and weight gradient, FIXED throughout (d_b of 1->16 is at 6.19 x ATen's pairwise sum).

THE LEDGER.  tests/conv_layers.py lists every stride-1 convolution of the seven networks and names, per pass, the case of this file
or of tests/test_gpu_ops.py that stands for it (checked on the host by tests/test_cpu_conv_layers.py);
test_the_ledger_lists_what_the_network_launches holds that table against what each network launches at its golden shape.

NOT REACHABLE, hence without a case:
 - conv3d_wgrad_np_kernel needs 5 <= Cin <= 8 and Cout <= 8: those shapes are transpose-read eligible (family 4) until a tensor
   passes 2 GiB, and tensors of 2 GiB and beyond are not this file's subject.
 - route_wgrad's third reason, Cout > 256: conv_bwd_weight_impl refuses Cout > 256 (MODET_ERR_UNSUPPORTED) before it launches.
 - the XF / ST instantiations of cfg 5 and 7: a statistics or normalised-input launch takes family 0 only below 4 096 voxels
   (cfg 6, 8) or beyond 6 000 000 (cfg 0 .. 4); cfg 5 needs 60 000 .. 600 000 voxels and cfg 7 at least 8 000.
   Those of cfg 6 and 8 are the existing small cases of tests/test_gpu_ops.py (test_conv_instnorm_fused_vs_oracle,
   test_lazy_instnorm_conv_inference) and are held here once more in SMALL_STAT_CASES under this file's rule."""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_layers
from tests.conv_layers import c1_class, fwd_class, shape_str, voxels, wgrad_class
from tests.util import assert_close, cl, note_many, rel_err

pytestmark = pytest.mark.gpu

A = 4.0
# tests/test_gpu_ops.py test_conv_vs_oracle's fixed tolerances, by quantity, as functions of the launch's voxel count (see the
# module docstring: FIXED TOLERANCES)
FIXED = {"y": lambda n: dict(atol=2e-5, rtol=2e-5), "y_act": lambda n: dict(atol=2e-5, rtol=2e-5),
         "d_x": lambda n: dict(atol=5e-5, rtol=2e-5),
         "d_w": lambda n: dict(atol=5e-4 * max(1.0, (n / 2e4) ** 0.5), rtol=2e-4),
         "d_b": lambda n: dict(atol=5e-4 * max(1.0, (n / 2e4) ** 0.5), rtol=2e-4)}
S1, S2, S3, S4 = (9, 11, 37), (12, 18, 21), (17, 43, 45), (47, 50, 80)
B_SIX_M = 1639                      # 1 639 x 3 663 = 6 003 657 voxels


def key(cin, cout, shape, B):
    return "%d->%d,%s,B%d" % (cin, cout, shape_str(shape), B)


# (Cin, Cout, sample, B, repeated sample?) -> the class the case is there for: (cfg, vector loads, several stages, P)
ACT_CASES = {
    # below 60 000 voxels in total
    (59, 16, S1, 2, False): (8, False, True, 1), (12, 16, S1, 2, False): (8, True, True, 1),
    (4, 8, S1, 2, False): (8, True, False, 1), (3, 3, S1, 2, False): (8, False, False, 1),
    (43, 43, S1, 2, False): (6, False, True, 1), (16, 32, S1, 2, False): (6, True, True, 1),
    (8, 32, S1, 2, False): (6, True, False, 1), (6, 20, S1, 2, False): (6, False, False, 1),
    (64, 64, S2, 2, False): (7, True, True, 1), (43, 64, S2, 2, False): (7, False, True, 1),
    (8, 64, S2, 2, False): (7, True, False, 1), (6, 64, S2, 2, False): (7, False, False, 1),
    # 60 000 .. 600 000 voxels: 17x43x45, B = 2 (65 790), or 18 copies of 9x11x37 (65 934) where the z-march would take 17x43x45
    (24, 16, S3, 2, False): (0, True, True, 1), (43, 16, S3, 2, False): (0, False, True, 1),
    (8, 16, S1, 18, True): (0, True, False, 1), (6, 12, S3, 2, False): (0, False, False, 1),
    (16, 8, S1, 18, True): (0, True, True, 2), (43, 8, S3, 2, False): (0, False, True, 2),
    (8, 8, S1, 18, True): (0, True, False, 2), (6, 8, S3, 2, False): (0, False, False, 2),
    (16, 3, S3, 2, False): (0, True, True, 4), (43, 3, S3, 2, False): (0, False, True, 4),
    (8, 3, S3, 2, False): (0, True, False, 4), (6, 3, S3, 2, False): (0, False, False, 4),
    (3, 16, S3, 2, False): (4, False, False, 1), (3, 8, S3, 2, False): (4, False, False, 2),
    (3, 3, S3, 2, False): (4, False, False, 4), (4, 16, S1, 18, True): (4, True, False, 1),
    (4, 8, S1, 18, True): (4, True, False, 2), (4, 3, S3, 2, False): (4, True, False, 4),
    (32, 32, S3, 2, False): (5, True, True, 1), (43, 32, S3, 2, False): (5, False, True, 1),
    (4, 32, S3, 2, False): (5, True, False, 1), (3, 24, S3, 2, False): (5, False, False, 1),
    (16, 64, S3, 2, False): (2, True, True, 1), (43, 43, S3, 2, False): (2, False, True, 1),
    (4, 48, S3, 2, False): (2, True, False, 1), (3, 48, S3, 2, False): (2, False, False, 1),
    (16, 96, S3, 2, False): (3, True, True, 1), (91, 91, S3, 2, False): (3, False, True, 1),
    (4, 128, S3, 2, False): (3, True, False, 1), (3, 80, S3, 2, False): (3, False, False, 1),
    # at or above 600 000 voxels: 164 copies of 9x11x37 (600 732)
    (20, 32, S1, 164, True): (1, True, True, 1), (91, 32, S1, 164, True): (1, False, True, 1),
    (4, 32, S1, 164, True): (1, True, False, 1), (3, 32, S1, 164, True): (1, False, False, 1),
}
SIX_M_CASES = ((43, 43), (43, 8), (8, 3), (16, 3), (3, 16), (59, 59), (59, 16), (91, 32), (20, 20), (12, 2), (8, 8),
               (12, 16), (48, 3))        # (the last two: the data gradients of PCNet's 9->48 and 48->3 at two pairs)
# (Cin, Cout) -> (cfg, ST or XF) on 32 copies of 47x50x80 (6 016 000 voxels); the normalised input runs too where Cin % 4 == 0
STAT_CASES = {(20, 16): (0, "ST"), (43, 8): (0, "ST"), (20, 4): (0, "ST"), (3, 16): (4, "ST"), (20, 32): (1, "XF"), (9, 48): (2, "XF"),
              (20, 68): (3, "XF"), (20, 12): (0, "XF")}
# below 4 096 voxels with Cin >= 8, Cin % 4 == 0: a statistics or normalised-input launch takes family 0 there (5x9x37, B = 2)
SMALL_STAT_CASES = {(8, 16): (8, "ST"), (16, 8): (8, "ST"), (12, 20): (6, "XF"), (16, 64): (6, "XF"), (16, 12): (8, "XF")}
S0 = (5, 9, 37)
# (Cin, Cout, B) -> (channel tile, z tile); B > 2: a repeated sample
WGRAD_CASES = {(43, 43, 2): (16, 2), (91, 32, 2): (16, 2), (9, 48, 2): (16, 2), (10, 20, 2): (16, 2), (6, 32, 2): (8, 2),
               (3, 16, 2): (4, 2), (2, 12, 2): (4, 2), (3, 3, 2): (4, 2), (3, 16, 274): (4, 4), (6, 32, 274): (8, 4)}


# the one-channel layers (the image): (Cin, Cout, sample, B, fused LeakyReLU?).  1->16 (PCNet) runs the tiles, cfg 4 with scalar
# loads; 1->8 (PR++) conv_c1_fwd_kernel<8>; 1->4 + LeakyReLU (ModeT, Im2grid) conv_c1_march_kernel from 500 000 voxels per sample
# on and conv_c1_wgrad_mfma_kernel with LeakyReLU' folded into its d_y load.  274 copies: >= 1 000 000 voxels, z tile 4.
IMAGE_CASES = ((1, 16, S1, 274, False), (1, 8, S1, 274, False), (1, 4, (79, 80, 82), 2, True))


@pytest.fixture(scope="module")
def ops():
    from smilecode_amd import ops as o
    yield o
    torch.cuda.empty_cache()


def family(ops, B, shape, cin, cout, pas, variant=0):
    return ops._L().modet_conv3d_kernel_family_v(B, *shape, cin, cout, pas, variant)


@functools.lru_cache(maxsize=None)
def tensors(cin, cout, shape, B, kind="randn"):
    """x, w, b, d_y of a case in fp64 (fp32 values), NCDHW: computed once, shared, never modified.  x has a constant region.
    kind "int": integers in [-3, 3], for which every product and every sum of the three passes is exact in fp32."""
    gen = torch.Generator().manual_seed(cin * 1009 + cout * 31 + shape[2] + B)
    if kind == "int":
        x, w, b, gy = (torch.randint(-3, 4, s, generator=gen).double()
                       for s in ((B, cin) + shape, (cout, cin, 3, 3, 3), (cout,), (B, cout) + shape))
        x[:, :, :, : shape[1] // 3] = 1.0
        return x, w, b, gy
    x = torch.randn((B, cin) + shape, generator=gen).double()
    x[:, :, :, : shape[1] // 3] = 0.25
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double()
    b = (0.1 * torch.randn(cout, generator=gen)).double()
    gy = torch.randn((B, cout) + shape, generator=gen).double()
    return x, w, b, gy


def in_stats(x):
    """per-(sample, channel) InstanceNorm mean / rstd of x in fp64, rounded to the fp32 the kernel is handed"""
    mean = x.mean((2, 3, 4))
    rstd = (x.var((2, 3, 4), unbiased=False) + 1e-5).rsqrt()
    return mean.float(), rstd.float()


def normalised(x, mean, rstd):
    """LeakyReLU((x - mean) * rstd) with the GIVEN statistics, in x's precision"""
    s = tuple(mean.shape) + (1, 1, 1)
    return F.leaky_relu((x - mean.to(x.dtype).reshape(s)) * rstd.to(x.dtype).reshape(s), 0.1)


def aten(cin, cout, shape, B, dtype, want, kind="randn"):
    """the quantities named in ``want`` of a case in ATen on the CPU, in ``dtype``"""
    x, w, b, gy = (t.to(dtype) for t in tensors(cin, cout, shape, B, kind))
    out = {}
    if want & {"y", "y_act", "y_norm"}:
        y = F.conv3d(x, w, b, padding=1)
        out["y"], out["y_act"] = y, F.leaky_relu(y, 0.1)
        if "y_norm" in want:
            out["y_norm"] = F.leaky_relu(F.instance_norm(y, eps=1e-5), 0.1)
    if want & {"z", "z_norm"}:
        z = F.conv3d(normalised(x, *in_stats(tensors(cin, cout, shape, B)[0])), w, b, padding=1)
        out["z"] = z
        if "z_norm" in want:
            out["z_norm"] = F.leaky_relu(F.instance_norm(z, eps=1e-5), 0.1)
    if "d_x" in want:
        out["d_x"] = torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)
    if want & {"d_w", "d_b"}:
        out["d_w"] = torch.nn.grad.conv3d_weight(x, w.shape, gy, padding=1)
        out["d_b"] = gy.sum((0, 2, 3, 4))
    return {q: out[q] for q in want}


@functools.lru_cache(maxsize=None)
def yardstick(cin, cout, shape, B, want):
    """(fp64 results, ATen fp32's error per quantity) of a case"""
    ref = aten(cin, cout, shape, B, torch.float64, set(want))
    f32 = aten(cin, cout, shape, B, torch.float32, set(want))
    return ref, {q: rel_err(f32[q], ref[q]) for q in want}


def nc(t):
    """device channels-last -> NCDHW (a view)"""
    return t.permute(0, 4, 1, 2, 3)


def hold(tag, errs, e_f32, fixed=()):
    """note every figure, then assert the rule per quantity (but for those in ``fixed``, which the caller holds to FIXED)"""
    note_many({"conv_exact[%s].%s.e_hip" % (tag, q): e for q, e in errs.items()})
    note_many({"conv_exact[%s].%s.e_f32" % (tag, q): e_f32[q] for q in errs})
    bad = ["%s: e_hip %.3e, ATen fp32 %.3e (x %.2f)" % (q, e, e_f32[q], e / max(e_f32[q], 1e-30)) for q, e in errs.items()
           if q not in fixed and not e <= A * e_f32[q]]
    assert not bad, "%s beyond A = %g x ATen fp32's error: %s" % (tag, A, "; ".join(bad))


def fixed_tol(q, n, k=1):
    """FIXED for a launch of n voxels.  A sum over k copies of one sample is k times the one sample's sum, as its fp64 reference
    is (every |d_w| grows like k, not like sqrt(k)): the one sample's absolute tolerance times k."""
    tol = FIXED[q](n // k)
    return dict(tol, atol=tol["atol"] * k)


def check(tag, got, ref, e_f32, n, k=1):
    """got, ref: quantity -> tensor (device NCDHW views / fp64 host); n: the launch's voxels; k: copies of the sample a sum ran
    over.  Notes every figure, then asserts FIXED where the quantity has one and the rule elsewhere."""
    hold(tag, {q: rel_err(got[q], k * ref[q]) for q in got}, e_f32, fixed=FIXED)
    for q in got:
        if q in FIXED:
            assert_close(got[q].double().cpu().numpy(), (k * ref[q]).numpy(), what="%s %s" % (tag, q), **fixed_tol(q, n, k))


def check_int(tag, got, ref, k=1):
    for q in got:
        g, r = got[q].double().cpu(), k * ref[q]
        assert g.shape == r.shape and torch.equal(g, r), "%s %s on integer data: max |got - fp64| = %g (max |fp64| = %g)" % (
            tag, q, float((g - r).abs().max()), float(r.abs().max()))
        assert float(r.abs().max()) > 0 and float(r.abs().max()) < 2 ** 24


def device_case(cin, cout, shape, Bs, B, kind="randn"):
    """the case's tensors on the device, channels-last; Bs samples repeated to B"""
    x, w, b, gy = tensors(cin, cout, shape, Bs, kind)
    rep = (lambda t: t.repeat(B // Bs, 1, 1, 1, 1)) if B != Bs else (lambda t: t)
    return rep(cl(x.numpy())), w.float().cuda(), b.float().cuda(), rep(cl(gy.numpy()))


def run_twice(fn, what, Bs=None):
    """fn() twice: the same bits; with Bs = 1 (a repeated sample) every further sample equals sample 0, which is returned"""
    y = fn()
    assert torch.equal(y, fn()), "%s: a second call differs" % what
    if Bs is None:
        return y
    assert Bs == 1 and torch.equal(y[1:], y[:1].expand_as(y[1:])), "%s: a sample differs from sample 0" % what
    return y[:1]


# ------------------------------------------------------------------------------------------------ a. fused LeakyReLU
def test_every_reachable_forward_instantiation_has_a_case():
    want = {(c, v, m, p) for c in (1, 2, 3, 5, 6, 7, 8) for v in (False, True) for m in (False, True) for p in (1,)}
    want |= {(0, v, m, p) for v in (False, True) for m in (False, True) for p in (1, 2, 4)}
    want |= {(4, v, False, p) for v in (False, True) for p in (1, 2, 4)}
    assert len(want) == 46 and set(ACT_CASES.values()) == want


@pytest.mark.parametrize("case", list(ACT_CASES), ids=lambda c: key(*c[:4]))
def test_fused_leaky_relu_forward_vs_fp64(ops, case):
    cin, cout, shape, B, rep = case
    Bs = 1 if rep else B
    assert family(ops, B, shape, cin, cout, 0, 1) == 0, "forward + LeakyReLU does not take the exact-f32 kernel"
    assert fwd_class(voxels(B, shape), cin, cout) == ACT_CASES[case]
    ref, e_f32 = yardstick(cin, cout, shape, Bs, ("y_act",))
    xd, wd, bd, _ = device_case(cin, cout, shape, Bs, B)
    with torch.no_grad():
        y = run_twice(lambda: ops.conv3d_forward(xd, wd, bd, True), "forward + LeakyReLU", 1 if rep else None)
    check("a:" + key(cin, cout, shape, B), {"y_act": nc(y)}, ref, e_f32, voxels(B, shape))
    # integer data: the fp64 result bit for bit, whatever the summation order (LeakyReLU: one fp32 product with fp32's 0.1)
    want = F.leaky_relu(aten(cin, cout, shape, Bs, torch.float64, {"y"}, "int")["y"].float(), 0.1).double()
    xd, wd, bd, _ = device_case(cin, cout, shape, Bs, B, "int")
    with torch.no_grad():
        y = run_twice(lambda: ops.conv3d_forward(xd, wd, bd, True), "forward + LeakyReLU, integer data", 1 if rep else None)
    check_int("a:" + key(cin, cout, shape, B), {"y_act": nc(y)}, {"y_act": want})


# ------------------------------------------------------------------------------------------------ b. beyond 6 000 000 voxels
@pytest.mark.parametrize("cin,cout", SIX_M_CASES, ids=lambda v: str(v))
def test_beyond_six_million_voxels_vs_fp64(ops, cin, cout):
    B, shape = B_SIX_M, S1
    n = voxels(B, shape)
    assert n > 6000000
    assert family(ops, B, shape, cin, cout, 0, 0) == 0, "forward does not take the exact-f32 kernel"
    assert family(ops, B, shape, cin, cout, 1, 0) == 0, "data gradient does not take the exact-f32 kernel"
    assert fwd_class(n, cin, cout)[0] in (0, 1, 2, 3, 4) and fwd_class(n, cout, cin)[0] in (0, 1, 2, 3, 4)
    normin = cin % 4 == 0
    if normin:
        assert family(ops, B, shape, cin, cout, 0, 2) == 0, "forward with a normalised input does not take the exact-f32 kernel"
    want = ("y", "d_x") + (("z",) if normin else ())
    ref, e_f32 = yardstick(cin, cout, shape, 1, want)
    tag = "b:" + key(cin, cout, shape, B)
    for kind in ("randn", "int"):
        xd, wd, bd, gd = device_case(cin, cout, shape, 1, B, kind)
        got = {}
        with torch.no_grad():
            got["y"] = run_twice(lambda: ops.conv3d_forward(xd, wd, bd, False), "forward", 1).clone()
            if normin and kind == "randn":
                mean, rstd = (t.cuda().repeat(B, 1).reshape(-1) for t in in_stats(tensors(cin, cout, shape, 1)[0]))
                got["z"] = run_twice(lambda: ops.conv3d_forward_normin(xd, mean, rstd, wd, bd, False)[0],
                                     "forward, normalised on load", 1).clone()
            del xd
            got["d_x"] = run_twice(lambda: ops.conv3d_backward_data(gd, wd, cin), "data gradient", 1).clone()
            del gd
        torch.cuda.empty_cache()
        got = {q: nc(t) for q, t in got.items()}
        if kind == "randn":
            check(tag, got, ref, e_f32, n)
        else:                          # integer data: the fp64 results bit for bit, whatever the summation order
            check_int(tag, got, aten(cin, cout, shape, 1, torch.float64, {"y", "d_x"}, "int"))


def _stat_case(ops, cin, cout, shape, Bs, B, cfg, kind, tag):
    n = voxels(B, shape)
    assert family(ops, B, shape, cin, cout, 0, 3) == 0, "forward + statistics does not take the exact-f32 kernel"
    assert fwd_class(n, cin, cout)[0] == cfg and (kind == "ST") == (cout in (4, 8, 16))
    assert ops._L().modet_conv3d_stats_bytes(B, *shape, cin, cout) > 0
    normin = cin % 4 == 0                    # (a normalised input always runs the XF instantiation)
    if normin:
        assert family(ops, B, shape, cin, cout, 0, 2) == 0
        assert ops._L().modet_conv3d_normin_stats_bytes(B, *shape, cin, cout) > 0
    want = ("y_norm",) + (("z", "z_norm") if normin else ())
    ref, e_f32 = yardstick(cin, cout, shape, Bs, want)
    xd, wd, bd, _ = device_case(cin, cout, shape, Bs, B)

    def err(got, q):                   # every copy of the Bs samples against fp64, on the device
        r = ref[q].cuda()
        g = nc(got).reshape(B // Bs, *r.shape).double()
        return float((g - r).abs().max()) / float(r.abs().max())

    errs = {}
    with torch.no_grad():
        errs["y_norm"] = err(run_twice(lambda: ops.conv3d_instnorm_lrelu(xd, wd, bd), "forward + fused statistics"), "y_norm")
        if normin:
            mean, rstd = (t.cuda().repeat(B // Bs, 1).reshape(-1) for t in in_stats(tensors(cin, cout, shape, Bs)[0]))
            z, zst = ops.conv3d_forward_normin(xd, mean, rstd, wd, bd, True)
            assert zst is not None
            z2, zst2 = ops.conv3d_forward_normin(xd, mean, rstd, wd, bd, True)
            assert torch.equal(z, z2) and torch.equal(zst, zst2), "normalised input + statistics: a second call differs"
            errs["z"] = err(z, "z")
            errs["z_norm"] = err(ops._InstNormLReLU.apply(z, 1e-5, zst), "z_norm")
    del xd
    torch.cuda.empty_cache()
    hold(tag + key(cin, cout, shape, B), errs, e_f32)


@pytest.mark.parametrize("cin,cout", list(STAT_CASES), ids=lambda v: str(v))
def test_fused_statistics_beyond_six_million_voxels_vs_fp64(ops, cin, cout):
    _stat_case(ops, cin, cout, S4, 1, 32, *STAT_CASES[(cin, cout)], "b:stats:")


@pytest.mark.parametrize("cin,cout", list(SMALL_STAT_CASES), ids=lambda v: str(v))
def test_fused_statistics_below_4096_voxels_vs_fp64(ops, cin, cout):
    assert voxels(2, S0) < 4096
    _stat_case(ops, cin, cout, S0, 2, 2, *SMALL_STAT_CASES[(cin, cout)], "small:stats:")


# ------------------------------------------------------------------------------------------------ c. weight gradient
def test_every_weight_gradient_instantiation_has_a_case():
    assert set(WGRAD_CASES.values()) == {(4, 2), (8, 2), (16, 2), (4, 4), (8, 4)}


@pytest.mark.parametrize("cin,cout,B", list(WGRAD_CASES), ids=lambda v: str(v))
def test_weight_gradient_vs_fp64(ops, cin, cout, B):
    shape, Bs = S1, (2 if B == 2 else 1)
    assert family(ops, B, shape, cin, cout, 2, 0) == 0, "weight gradient does not take the exact-f32 kernel"
    assert wgrad_class(voxels(B, shape), cin, cout) == WGRAD_CASES[(cin, cout, B)]
    assert not (4 < cin <= 8 and cout <= 8)                      # (that would be conv3d_wgrad_np_kernel)
    ref, e_f32 = yardstick(cin, cout, shape, Bs, ("d_w", "d_b"))
    k = B // Bs                                                  # the fp64 reference of k copies is k times the one sample's
    for kind in ("randn", "int"):
        xd, _, _, gd = device_case(cin, cout, shape, Bs, B, kind)
        with torch.no_grad():
            dw, db = ops.conv3d_backward_weight(xd, gd, True)
            dw2, db2 = ops.conv3d_backward_weight(xd, gd, True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "weight gradient: a second call differs"
        if kind == "randn":
            check("c:" + key(cin, cout, shape, B), {"d_w": dw, "d_b": db}, ref, e_f32, voxels(B, shape), k)
        else:                          # integer data: sums below 2^24 (274 x 3 663 x 9), so the fp64 result bit for bit
            check_int("c:" + key(cin, cout, shape, B), {"d_w": dw, "d_b": db},
                      aten(cin, cout, shape, Bs, torch.float64, {"d_w", "d_b"}, "int"), k)


# ------------------------------------------------------------------------------------------------ the image layers
@pytest.mark.parametrize("case", IMAGE_CASES, ids=lambda c: key(*c[:4]))
def test_one_channel_layers_vs_fp64(ops, case):
    """forward and weight gradient of the layers that convolve the image (no data gradient exists in any network)"""
    cin, cout, shape, B, act = case
    Bs = 1 if B > 2 else B
    n, k, tag = voxels(B, shape), B // Bs, "image:" + key(cin, cout, shape, B)
    assert family(ops, B, shape, cin, cout, 0, int(act)) == 0 and family(ops, B, shape, cin, cout, 2, 0) == 0
    assert c1_class(voxels(1, shape), cout) == {16: "tiles", 8: "flat", 4: "march"}[cout]
    assert cout == 4 or (wgrad_class(n, cin, cout) == (4, 4) and fwd_class(n, cin, cout)[0] == 4)
    q = "y_act" if act else "y"
    for kind in ("randn", "int"):
        ref = aten(cin, cout, shape, Bs, torch.float64, {q, "d_w", "d_b"}, kind)
        xd, wd, bd, gd = device_case(cin, cout, shape, Bs, B, kind)
        with torch.no_grad():
            y = ops.conv3d_forward(xd, wd, bd, act)
            assert torch.equal(y, ops.conv3d_forward(xd, wd, bd, act)), "forward: a second call differs"
            if act:                    # the first block's form: d_y is the gradient behind the LeakyReLU, its slope taken from y
                slope = torch.where(nc(y) > 0, 1.0, float(np.float32(0.1))).double().cpu()
                x64, _, _, gy64 = tensors(cin, cout, shape, Bs, kind)
                ref["d_w"] = torch.nn.grad.conv3d_weight(x64, wd.shape, gy64 * slope, padding=1)
                ref["d_b"] = (gy64 * slope).sum((0, 2, 3, 4))
                dw, db = ops.conv3d_backward_weight(xd, gd, True, y_act=y)
                dw2, db2 = ops.conv3d_backward_weight(xd, gd, True, y_act=y)
            else:
                assert torch.equal(y[1:], y[:1].expand_as(y[1:])), "forward: a sample differs from sample 0"
                dw, db = ops.conv3d_backward_weight(xd, gd, True)
                dw2, db2 = ops.conv3d_backward_weight(xd, gd, True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "weight gradient: a second call differs"
        got = {q: nc(y[:Bs]), "d_w": dw, "d_b": db}
        if kind == "randn":
            f32 = aten(cin, cout, shape, Bs, torch.float32, {q, "d_w", "d_b"})
            ref0 = aten(cin, cout, shape, Bs, torch.float64, {q, "d_w", "d_b"})
            e_f32 = {v: rel_err(f32[v], ref0[v]) for v in ref0}          # (the yardstick's d_w, d_b: without the slope)
            hold(tag, {q: rel_err(got[q], ref[q])}, e_f32, fixed=FIXED)
            for v in got:
                scale = 1 if v == q else k
                assert_close(got[v].double().cpu().numpy(), (scale * ref[v]).numpy(), what="%s %s" % (tag, v), **fixed_tol(v, n, scale))
            note_many({"conv_exact[%s].%s.e_hip" % (tag, v): rel_err(got[v], k * ref[v]) for v in ("d_w", "d_b")})
            note_many({"conv_exact[%s].%s.e_f32" % (tag, v): e_f32[v] for v in ("d_w", "d_b")})
        else:
            check_int(tag, {q: got[q]}, {q: ref[q] if not act else F.leaky_relu(
                aten(cin, cout, shape, Bs, torch.float64, {"y"}, "int")["y"].float(), 0.1).double()})
            if not act:                # (with the fp32 slope 0.1 folded into d_y the sums are no integers)
                check_int(tag, {"d_w": dw, "d_b": db}, ref, k)
        del xd, gd, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the second weight packer
def test_prepacked_weights_equal_per_launch_packing(ops):
    """pack_weights_many_kernel (ops.StepContext.prepacked(): every recorded job packed in one launch) against pack_weights_kernel
    (one launch per convolution) on odd channel counts: mode 0 with P = 1, 2, 4 through the fused LeakyReLU, mode 1 (the data
    gradient) with P = 2 beyond 6 000 000 voxels.  The same bits."""
    layers = [(43, 43, S1, 2, 2), (43, 8, S1, 1, 18), (16, 3, S1, 1, 18), (3, 8, S1, 1, 18), (8, 3, S1, 1, B_SIX_M)]
    data = [device_case(*c) for c in layers]

    def run():
        out = []
        with torch.no_grad():
            for (cin, cout, shape, Bs, B), (xd, wd, bd, gd) in zip(layers, data):
                assert family(ops, B, shape, cin, cout, 0, 1) == 0
                out.append(ops.conv3d_forward(xd, wd, bd, True))
                if B == B_SIX_M:
                    assert family(ops, B, shape, cin, cout, 1, 0) == 0 and fwd_class(voxels(B, shape), cout, cin)[3] == 2
                    out.append(ops.conv3d_backward_data(gd, wd, cin))
        return out

    want = run()
    pp = ops.StepContext()
    with pp.prepacked():
        run()                                                    # the recording pass
    with pp.prepacked():
        got = run()                                              # one packing launch, no per-launch packing
    assert pp.recorded and pp.arena is not None
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    del data
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the ledger against the networks
@pytest.mark.parametrize("network", list(conv_layers.NETWORKS))
def test_the_ledger_lists_what_the_network_launches(ops, monkeypatch, network):
    """one forward + backward of the network (the ledger's channels) at its golden shape with the convolution entry points of
    smilecode_amd.ops behind a recorder: the multiset of (B as launched, log2 of the downsampling, Cin, Cout, variant) of the
    forward launches is the ledger's for that shape, and every layer launches one weight gradient"""
    from smilecode_amd import models, synth
    cls = {"ModeT": models.ModeT, "Im2grid": models.Im2grid, "RDN": models.RDN, "RDNStages": models.RDNStages, "RCN": models.RCN,
           "PCNet": models.PCNet, "PR++": models.PRNetplusplus}[network]
    shape = conv_layers.GOLDEN_SHAPE.get(network, (32, 48, 32))
    _, kw, rows = conv_layers.NETWORKS[network]
    fwd, wgrad = [], []
    f0, w0 = ops._conv_fwd, ops.conv3d_backward_weight

    def rec_fwd(x, w, b, step, bounded=False, act=False, norm=None, want_stats=False):
        fwd.append(tuple(x.shape) + (w.shape[0], 2 if norm else (3 if want_stats else int(bool(act)))))
        return f0(x, w, b, step, bounded=bounded, act=act, norm=norm, want_stats=want_stats)

    def rec_wgrad(x, dy, *a, **k):
        wgrad.append(tuple(x.shape) + (dy.shape[-1],))
        return w0(x, dy, *a, **k)

    monkeypatch.setattr(ops, "_conv_fwd", rec_fwd)
    monkeypatch.setattr(ops, "conv3d_backward_weight", rec_wgrad)
    torch.manual_seed(0)
    m = cls(shape, **kw).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    mov, fix = (torch.from_numpy(a).cuda() for a in synth.make_pair(shape, 24, batch=1))
    outs = m(mov, fix)
    outs = [t for o in (outs if isinstance(outs, (tuple, list)) else (outs,)) for t in (o if isinstance(o, (tuple, list)) else (o,))]
    sum(o.float().square().mean() for o in outs if torch.is_tensor(o) and o.requires_grad).backward()
    torch.cuda.synchronize()
    level = lambda D: int(round(np.log2(shape[0] / D)))          # noqa: E731
    L = ops._L()
    want = collections.Counter()
    for bmul, lvl, ci, co, role, n in rows:
        v = conv_layers.launch_variant(L, role, bmul, conv_layers.level_shape(shape, lvl), ci, co)
        want[(bmul, lvl, ci, co, v)] += n
    got = collections.Counter((B, level(D), ci, co, v) for B, D, H, W, ci, co, v in fwd)
    assert got == want, "launched but not in the ledger: %s; in the ledger but not launched: %s" % (
        sorted((got - want).items()), sorted((want - got).items()))
    assert all(tuple(s) == conv_layers.level_shape(shape, level(s[0])) for s in (f[1:4] for f in fwd))
    assert collections.Counter(f[:6] for f in fwd) == collections.Counter(wgrad), "a layer without exactly one weight gradient"
