"""The four fused operators of the PCNet family (include/modet_hip_pcnet.h, smilecode_amd.ops.upsample_pow2 / dfi_gate / nff_fuse /
residual_add) as ATen compositions on the CPU, written the way "Baseline methods/PCnet/models.py" writes them (nn.Upsample,
torch.cat, nn.Sigmoid, nn.Softmax(dim=1), AdaptiveAvgPool3d / AdaptiveMaxPool3d, two bias-free nn.Linear) with a dtype argument:
float64 is the oracle, float32 the yardstick of the GPU tests.  Tensors are channels-last here as in the package; the compositions
permute to the reference's planar layout and back.  Also the seeded cases of tests/test_gpu_pcnet_ops.py and the guard file."""
import torch
import torch.nn.functional as F


def to_planar(t):
    return t.permute(0, 4, 1, 2, 3)


def to_cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the operators
def upsample_pow2(x, f):
    """(B,d,h,w,3) -> (B,fd,fh,fw,3): DFIBlock.upsample[i]"""
    return to_cl(F.interpolate(to_planar(x), scale_factor=f, mode="trilinear", align_corners=True))


def dfi_gate(x, logits):
    """(N..,3n) x 2 -> (N..,3): the loop of DFIBlock.forward, prediction_i * sigmoid(weight_conv_i(x)) summed in order"""
    n = x.shape[-1] // 3
    out = None
    for i in range(n):
        term = x[..., 3 * i:3 * i + 3] * torch.sigmoid(logits[..., 3 * i:3 * i + 3])
        out = term if out is None else out + term
    return out


def nff_cat(t0, t1, t2, logits):
    """the concatenation of NFFBlock.forward, planar (B,3C,D,H,W)"""
    wm = torch.softmax(to_planar(logits), dim=1)
    return torch.cat([to_planar(t0) * wm[:, 0:1], to_planar(t1) * wm[:, 1:2], to_planar(t2) * wm[:, 2:3]], dim=1)


def nff_fuse(t0, t1, t2, logits, W1, W2):
    """NFFBlock.forward after weight_conv's convolution, ChannelAttention included: (B,D,H,W,3C)"""
    cat = nff_cat(t0, t1, t2, logits)
    b, c = cat.shape[:2]
    fc = lambda v: F.linear(torch.relu(F.linear(v, W1)), W2)        # noqa: E731
    y_avg = fc(F.adaptive_avg_pool3d(cat, 1).view(b, c))
    y_max = fc(F.adaptive_max_pool3d(cat, 1).view(b, c))
    return to_cl(cat * torch.sigmoid(y_avg + y_max).view(b, c, 1, 1, 1))


def value_and_grads(fn, tensors, gy, dtype, wrt=None):
    """fn on ``tensors`` (name -> tensor) in ``dtype`` and the gradients of <result, gy> for the names in ``wrt`` (default all)"""
    t = {k: v.detach().to(dtype).requires_grad_(wrt is None or k in wrt) for k, v in tensors.items()}
    y = fn(*t.values())
    names = [k for k in t if t[k].requires_grad]
    g = torch.autograd.grad(y, [t[k] for k in names], gy.to(dtype))
    out = {"out": y.detach()}
    out.update({"d_" + k: v for k, v in zip(names, g)})
    return out


# ------------------------------------------------------------------------------------------------ seeded cases
def gen(seed):
    return torch.Generator().manual_seed(seed)


UP_CASES = {                      # n: (B, coarse shape, f)
    1: (1, (2, 3, 5), 2), 2: (1, (2, 3, 5), 4), 3: (1, (2, 3, 5), 8), 4: (1, (2, 3, 2), 8), 5: (1, (3, 5, 7), 2), 6: (2, (2, 3, 5), 4),
}


def up_tensors(n, seed=None):
    B, (d, h, w), f = UP_CASES[n]
    g = gen(7100 + n if seed is None else seed)
    x = torch.randn(B, d, h, w, 3, generator=g)
    gy = torch.randn(B, f * d, f * h, f * w, 3, generator=g)
    return x, gy


DFI_CASES = {1: (2, (5, 7, 9), 1), 2: (2, (5, 7, 9), 2), 3: (2, (5, 7, 9), 3)}          # n: (B, shape, fields); 630 voxels = 157 x 4 + 2


def dfi_tensors(n, seed=None):
    B, shape, nf = DFI_CASES[n]
    g = gen(7200 + n if seed is None else seed)
    x = torch.randn(B, *shape, 3 * nf, generator=g)
    lg = 2.0 * torch.randn(B, *shape, 3 * nf, generator=g)
    gy = torch.randn(B, *shape, 3, generator=g)
    return x, lg, gy


# n: (B, shape, C).  V = 12, 315, 9600 (10 partial rows of 1024 voxels, the last of 384); hidden widths 1, 3, 7, 24
NFF_CASES = {
    1: (1, (2, 3, 2), 4), 2: (2, (2, 3, 2), 8), 3: (2, (5, 7, 9), 4), 4: (1, (5, 7, 9), 20), 5: (2, (5, 7, 9), 64),
    6: (2, (20, 24, 20), 8), 7: (1, (20, 24, 20), 20),
}
NFF_YARD = (1, 2, 3, 4, 5)        # the yardstick's cases, frozen
PLANT = 1.5                       # the factor on each channel's winning voxel (THE ARGMAX CONDITION of the GPU test file)


def nff_tensors(n, seed=None, plant="max"):
    """t0, t1, t2, logits, W1, W2, gy.  Every (sample, channel) of the concatenation gets ONE voxel that wins by a factor: the
    voxel where the channel's cat is largest in fp64 has its t scaled so that it becomes PLANT x the largest value -- sample b,
    channel j plants at a voxel of its own.  ``plant``: "max" as described; "ends": the winners of channels 0 and 1 are moved to
    the first and the last voxel; "tie": channel 0 holds its maximum at the two voxels of TIE_AT, equal bit for bit."""
    B, shape, C = NFF_CASES[n]
    V = shape[0] * shape[1] * shape[2]
    g = gen(7300 + n if seed is None else seed)
    ts = [torch.randn(B, *shape, C, generator=g) for _ in range(3)]
    lg = torch.randn(B, *shape, 3, generator=g)
    R = 3 * C // 8
    W1 = torch.randn(R, 3 * C, generator=g) / (3 * C) ** 0.5
    W1[0].abs_()                  # hidden unit 0 is active on the (planted, positive) maxima: with R = 1 no gradient is all zero
    W2 = torch.randn(3 * C, R, generator=g) / max(R, 1) ** 0.5
    gy = torch.randn(B, *shape, 3 * C, generator=g)
    if plant == "tie":
        lg.reshape(B, V, 3)[:, list(TIE_AT(V))] = 0.0
    wm = torch.softmax(lg.double(), dim=-1).reshape(B, V, 3)
    flat = [t.reshape(B, V, C) for t in ts]
    for b in range(B):
        for k in range(3):
            cat = flat[k][b].double() * wm[b, :, k:k + 1]                    # (V, C)
            top, at = cat.max(dim=0)
            for ch in range(C):
                v = int(at[ch])
                if plant == "ends" and k == 0 and ch in (0, 1):
                    v = 0 if ch == 0 else V - 1
                if plant == "tie" and k == 0 and ch == 0:
                    v = TIE_AT(V)[0]
                flat[k][b, v, ch] = float(PLANT * max(float(top[ch]), 1e-3) / float(wm[b, v, k]))
                if plant == "tie" and k == 0 and ch == 0:
                    flat[k][b, TIE_AT(V)[1], ch] = flat[k][b, v, ch]
    return (*ts, lg, W1, W2, gy)


def TIE_AT(V):
    """the two voxels of the planted tie: zero logits there (weights of exactly 1/3 in every implementation of softmax: exp(0) is
    1) and the same t value, so the two products are equal bit for bit in fp32 and in fp64, on the CPU and in the kernels"""
    return V // 3, (2 * V) // 3


NFF_NAMES = ("t0", "t1", "t2", "logits", "W1", "W2")


def nff_gaps(t0, t1, t2, logits, dtype=torch.float64):
    """per (sample, channel) of the concatenation: (top1 - top2) / |top1| over the voxels"""
    cat = nff_cat(*(t.to(dtype) for t in (t0, t1, t2, logits)))
    b, c = cat.shape[:2]
    top = cat.reshape(b, c, -1).topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) / top[..., 0].abs()


# ------------------------------------------------------------------------------------------------ the network
# "Baseline methods/PCnet/models.py" PCNet as pure functions over a name -> tensor dict with the reference's state-dict names, on
# planar (B,C,D,H,W) tensors, differentiable through autograd, in fp64 (the oracle) or fp32 (the ATen yardstick).
import functools  # noqa: E402
import math  # noqa: E402

from oracle import modet_torch as mt  # noqa: E402
from tests import vecint_oracle  # noqa: E402

DFI_CHANNEL = 16          # DFIBlock's width, whatever the network's


def _in_lrelu(x):
    return F.leaky_relu(F.instance_norm(x, eps=1e-5), mt.LRELU)


def _conv(p, name, x, stride=1):
    return F.conv3d(x, p[name + ".weight"], p[name + ".bias"], stride=stride, padding=1)


def encoder(p, pre, x):
    outs = [mt.conv_ins_block(p, pre + ".conv0", x)]
    for k in (1, 2, 3):
        y = _conv(p, "%s.conv%d.0" % (pre, k), outs[-1], stride=2)
        y = _conv(p, "%s.conv%d.1.block.2" % (pre, k), _in_lrelu(y)) + y
        outs.append(_in_lrelu(y))
    return outs


def upconv(p, name, x):
    return _in_lrelu(F.conv_transpose3d(x, p[name + ".upconv.weight"], p[name + ".upconv.bias"], stride=2, padding=1))


def dfi(p, name, preds):
    n = len(preds)
    ups = [F.interpolate(q, scale_factor=2 ** (n - i), mode="trilinear", align_corners=True) for i, q in enumerate(preds)]
    x = mt.conv_ins_block(p, name + ".conv.1", mt.conv_ins_block(p, name + ".conv.0", torch.cat(ups, dim=1)))
    field = None
    for i, u in enumerate(ups):
        term = u * torch.sigmoid(_conv(p, "%s.weight_conv.%d.0" % (name, i), x))
        field = term if field is None else field + term
    return vecint_oracle.vecint(field, 7)


def nff(p, name, a, b, c, taps=None):
    x = mt.conv_ins_block(p, name + ".conv.1", mt.conv_ins_block(p, name + ".conv.0", torch.cat([a, b, c], dim=1)))
    wm = torch.softmax(_conv(p, name + ".weight_conv.0", x), dim=1)
    cat = torch.cat([a * wm[:, 0:1], b * wm[:, 1:2], c * wm[:, 2:3]], dim=1)
    if taps is not None:
        taps[name + ".cat"] = cat
    B, C = cat.shape[:2]
    W1, W2 = p[name + ".channel_attention.fc.0.weight"], p[name + ".channel_attention.fc.2.weight"]
    fc = lambda v: F.linear(torch.relu(F.linear(v, W1)), W2)        # noqa: E731
    g = torch.sigmoid(fc(F.adaptive_avg_pool3d(cat, 1).view(B, C)) + fc(F.adaptive_max_pool3d(cat, 1).view(B, C)))
    return cat * g.view(B, C, 1, 1, 1)


def pcnet_forward(p, moving, fixed, taps=None):
    """PCNet.forward -> (y_moved, flow), planar.  ``taps`` (a dict) receives warping_field_{2,1,0}, pred0 (integrated) and the
    concatenation every NFF block pools, nff_{2,1,0}.cat"""
    M, Fx = encoder(p, "encoder_float", moving), encoder(p, "encoder_fixed", fixed)
    feat = mt.conv_ins_block(p, "conv_bottleNeck.1", mt.conv_ins_block(p, "conv_bottleNeck.0", torch.cat([Fx[3], M[3]], dim=1)))
    preds, field = [], None
    for lvl in (2, 1, 0):
        preds.append(_conv(p, "reg_conv%d" % (lvl + 1), feat))
        deconv = upconv(p, "upconv%d" % lvl, feat)
        field = dfi(p, "dfi_%d" % lvl, preds)
        feat = nff(p, "nff_%d" % lvl, Fx[lvl], mt.warp(M[lvl], field), deconv, taps)
        if taps is not None:
            taps["warping_field_%d" % lvl] = field
    pred0 = vecint_oracle.vecint(_conv(p, "reg_conv0.1", _conv(p, "reg_conv0.0", feat)), 7)
    if taps is not None:
        taps["pred0"] = pred0
    flow = mt.warp(field, pred0) + pred0
    return mt.warp(moving, flow), flow


def train_loss(p, moving, fixed, weights=(1.0, 1.0), taps=None):
    """NCC(fixed, moved) * weights[0] + Grad3d('l2')(flow) * weights[1] ("Baseline methods/PCnet/train.py":99-126)"""
    moved, flow = pcnet_forward(p, moving, fixed, taps)
    return mt.ncc_loss(fixed, moved) * weights[0] + mt.grad3d_loss(flow) * weights[1], moved, flow


def pcnet_shapes(c, in_channel=1):
    """name -> shape of PCNet's parameters, in the reference's registration order"""
    s = {}

    def conv(name, cin, cout, k=3):
        s[name + ".weight"], s[name + ".bias"] = (cout, cin, k, k, k), (cout,)

    for enc in ("encoder_float", "encoder_fixed"):
        conv(enc + ".conv0.main", in_channel, c)
        for k, (ci, co) in zip((1, 2, 3), ((c, 2 * c), (2 * c, 4 * c), (4 * c, 8 * c))):
            conv("%s.conv%d.0" % (enc, k), ci, co)
            conv("%s.conv%d.1.block.2" % (enc, k), co, co)
    conv("conv_bottleNeck.0.main", 16 * c, 8 * c)
    conv("conv_bottleNeck.1.main", 8 * c, 8 * c)
    for lvl, cin_reg, cin_up, cout_up, C3 in ((2, 8 * c, 8 * c, 4 * c, 12 * c), (1, 12 * c, 12 * c, 2 * c, 6 * c), (0, 6 * c, 6 * c, c, 3 * c)):
        conv("reg_conv%d" % (lvl + 1), cin_reg, 3)
        s["upconv%d.upconv.weight" % lvl], s["upconv%d.upconv.bias" % lvl] = (cin_up, cout_up, 4, 4, 4), (cout_up,)
        n = 3 - lvl
        conv("dfi_%d.conv.0.main" % lvl, 3 * n, DFI_CHANNEL * n)
        conv("dfi_%d.conv.1.main" % lvl, DFI_CHANNEL * n, DFI_CHANNEL * n)
        for i in range(n):
            conv("dfi_%d.weight_conv.%d.0" % (lvl, i), DFI_CHANNEL * n, 3)
        conv("nff_%d.conv.0.main" % lvl, C3, C3)
        conv("nff_%d.conv.1.main" % lvl, C3, C3)
        conv("nff_%d.weight_conv.0" % lvl, C3, 3)
        s["nff_%d.channel_attention.fc.0.weight" % lvl] = (C3 // 8, C3)
        s["nff_%d.channel_attention.fc.2.weight" % lvl] = (C3, C3 // 8)
    conv("reg_conv0.0", 3 * c, c)
    conv("reg_conv0.1", c, 3)
    return s


FIELD_RANGE = (0.5, 4.0)      # voxels: max |w| of every level's warping field and of the integrated last prediction (a condition)
FIELD_TAPS = (("reg_conv3", "warping_field_2"), ("reg_conv2", "warping_field_1"), ("reg_conv1", "warping_field_0"), ("reg_conv0.1", "pred0"))


def make_weights(channels, moving=None, fixed=None, seed=31, in_channel=1, dtype=torch.float64):
    """seeded parameters with the reference's names, fp32-representable: He-like scales that keep activations of the order of one.
    With a pair given, each field head (reg_conv3, reg_conv2, reg_conv1, reg_conv0.1) is scaled in turn -- by a power of two,
    found by running the network in fp64 -- so that the field it closes (warping_field_2, _1, _0, the integrated pred0) has
    max |w| of about 1.5 voxels on that pair: with default initialisation the fields are small and the warps test nothing."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, shape in pcnet_shapes(channels, in_channel).items():
        t = torch.randn(shape, generator=g)
        if name.endswith(".bias"):
            t = t * 0.05
        elif ".upconv." in name:
            t = t * (1.4 / math.sqrt(8 * shape[0]))
        elif ".fc." in name:
            t = t * (1.0 / math.sqrt(shape[1]))
            if name.endswith("fc.0.weight"):
                t[0].abs_()           # hidden unit 0 is active on the (positive) maxima: with a hidden width of 1 (nff_0 at channels = 4) no gradient is all zero
        else:
            t = t * (1.4 / math.sqrt(27 * shape[1]))
        p[name] = t.float().double()
    if moving is not None:
        for head, tap in FIELD_TAPS:
            with torch.no_grad():
                taps = {}
                pcnet_forward(p, moving.double(), fixed.double(), taps)
                scale = 2.0 ** round(math.log2(1.5 / float(taps[tap].abs().max())))
                p[head + ".weight"], p[head + ".bias"] = p[head + ".weight"] * scale, p[head + ".bias"] * scale
    return {k: v.float().to(dtype) for k, v in p.items()}


GOLD_SHAPE, GOLD_CHANNELS, PAIR_SEED = (32, 48, 32), 4, 24
GOLD_SEED = 31                # the weight seed the generator's search settled on (tests/golden/REPORT_pcnet.txt)
NFF_TAPS = ("nff_2.cat", "nff_1.cat", "nff_0.cat")


@functools.lru_cache(maxsize=None)
def golden_pair(shape=GOLD_SHAPE):
    """the seeded pair of the goldens (B = 2), (moving, fixed) each (2,1,D,H,W) fp32: smilecode_amd.synth.make_pair, not stored"""
    from smilecode_amd import synth
    return tuple(torch.from_numpy(a) for a in synth.make_pair(shape, PAIR_SEED, batch=2))


@functools.lru_cache(maxsize=None)
def golden_weights(channels=GOLD_CHANNELS, shape=GOLD_SHAPE, seed=None):
    mov, fix = golden_pair(shape)
    return make_weights(channels, mov, fix, GOLD_SEED if seed is None else seed)


def net_value_and_grads(p, moving, fixed, dtype, taps=None):
    """one evaluation in ``dtype`` -> (loss, moved, flow, {name: gradient}), everything detached"""
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    loss, moved, flow = train_loss(q, moving.to(dtype), fixed.to(dtype), taps=taps)
    names = sorted(q)
    grads = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    if taps is not None:
        for k in taps:
            taps[k] = taps[k].detach()
    return loss.detach(), moved.detach(), flow.detach(), {n: (torch.zeros_like(q[n]) if g is None else g.detach()) for n, g in zip(names, grads)}


def cat_gaps(cat):
    """per (sample, channel) of a planar pooled tensor: (top1 - top2) / |top1|"""
    top = cat.flatten(2).topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) / top[..., 0].abs()


def argmax_condition(p, moving, fixed):
    """tap -> (smallest gap, ATen fp32's relative error on the tensor): THE ARGMAX CONDITION is gap >= 100 x error for every tap"""
    t64, t32 = {}, {}
    with torch.no_grad():
        pcnet_forward({k: v.double() for k, v in p.items()}, moving.double(), fixed.double(), t64)
        pcnet_forward({k: v.float() for k, v in p.items()}, moving.float(), fixed.float(), t32)
    out = {}
    for k in NFF_TAPS:
        err = float((t32[k].double() - t64[k]).abs().max()) / float(t64[k].abs().max())
        out[k] = (float(cat_gaps(t64[k]).min()), err)
    return out
