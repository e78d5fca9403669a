"""TEST INFRASTRUCTURE ONLY -- CPU oracle of the stride-2 4x4x4 transposed convolution and of the RCN / VTN baseline ("Baseline
methods/RCN/models.py"), an independent torch composition: F.conv_transpose3d(stride=2, padding=1) for the upsampling layers,
F.conv3d for both kinds of convolution, oracle/modet_torch.py's warp, ncc_loss and grad3d_loss.  Pure functions over a name ->
tensor dict, differentiable through autograd, in fp64 (the reference for every bound) or fp32 (the ATen yardstick: what the same
composition loses in single precision).

The cases of tests/test_gpu_deconv.py and tests/test_gpu_deconv_guard.py live here, so that both build the same tensors."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import modet_torch as orc

# case number of the issue's table -> (B, input grid (D, H, W), Cin, Cout, bias, slope); slope None = no activation
OP_CASES = {
    1: (2, (1, 1, 1), 8, 4, True, 0.1),         # every output voxel has a single in-range tap per axis
    2: (1, (1, 2, 3), 256, 128, True, 0.1),     # Deconv5 at channels = 8
    3: (2, (3, 4, 5), 3, 3, False, None),       # the flow upsampler
    4: (1, (2, 3, 2), 259, 64, True, 0.1),      # odd Cin tail
    5: (2, (5, 6, 7), 19, 3, False, None),      # Pred0
    6: (1, (9, 17, 33), 8, 4, True, 0.1),       # several tiles, a partial one in every axis
    7: (1, (4, 4, 4), 1, 1, True, None),        # the smallest channel counts
    # (N = B D H W input voxels; the weight gradient makes S = ceil(N / max(256, ceil(N / 256))) partial rows)
    8: (1, (9, 11, 12), 8, 8, True, 0.1),       # 4x4x8 forward tile, 3x3x2 tiles, partial in D and H; N = 1188: S = 5
    9: (2, (7, 8, 14), 20, 6, True, 0.1),       # activation with a Cout tail, chunks of 16 + 4, 4x4x4 data-gradient tiles; S = 7
    10: (1, (6, 7, 9), 35, 8, True, 0.1),       # the network's Deconv2: chunks of 16 + 16 + 3, 9 input-channel groups
    11: (1, (5, 6, 9), 24, 20, True, 0.1),      # 4x4x4 forward tile, 2x2x3 tiles with partial ones, a last chunk of 8
    12: (1, (5, 6, 9), 24, 13, True, 0.1),      # 4x4x4 forward tile with a Cout tail and an activation
    13: (1, (41, 40, 41), 2, 3, False, None),   # N = 67 240 > 65 536: splits of 263 voxels, S = 256, the last one of 175
}
MASK_BELOW = 1e-5          # |y| in fp64 below which the two precisions may take different LeakyReLU branches
MASK_CAP = 0.01            # at most this share of a case's outputs may lose its cotangent

# the variant sweep of tests/test_gpu_deconv.py: one sample of SWEEP_GRID with a bias at every (Cin, Cout, slope) of the product
SWEEP_GRID = (5, 9, 9)
SWEEP_CIN, SWEEP_COUT, SWEEP_SLOPES = (3, 8, 12, 27), (3, 4, 6, 8, 12, 13), (None, 0.1)


def sweep_spec(Cin, Cout, slope):
    """(spec, seed) of a sweep combination for spec_tensors"""
    return (1, SWEEP_GRID, Cin, Cout, True, slope), 5000 + 40 * Cin + Cout + (0 if slope is None else 20)


def out_shape(D, H, W):
    return (2 * D, 2 * H, 2 * W)


def f32_slope(slope):
    """the slope as the kernel receives it: rounded to fp32 once (0.1 is not an fp32 number), whatever the run's dtype"""
    return None if slope is None else float(torch.tensor(slope, dtype=torch.float32))


def lrelu(y, slope):
    return y if slope is None else torch.where(y > 0, y, y * f32_slope(slope))


def deconv_cl(x, w, b, slope):
    """channels-last (B,D,H,W,Cin) -> (B,2D,2H,2W,Cout): F.conv_transpose3d(stride=2, padding=1), then LeakyReLU(slope)"""
    y = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3), w, b, stride=2, padding=1)
    return lrelu(y, slope).permute(0, 2, 3, 4, 1)


def deconv_crop_cl(x, w, b, slope):
    """the reference's own form: ConvTranspose3d(4, stride=2) without padding, then the crop [1:-1] of every axis"""
    y = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3), w, b, stride=2)[:, :, 1:-1, 1:-1, 1:-1]
    return lrelu(y, slope).permute(0, 2, 3, 4, 1)


def deconv_by_rule(x, w, b):
    """the issue's index rule written out: output o receives tap k of input i = (o + 1 - k) / 2 -- no library convolution"""
    B, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    y = torch.zeros(B, 2 * D, 2 * H, 2 * W, Cout, dtype=x.dtype)
    for kd in range(4):
        for kh in range(4):
            for kw in range(4):
                t = torch.einsum("bdhwi,io->bdhwo", x, w[:, :, kd, kh, kw])
                for i_d in range(D):
                    od = 2 * i_d - 1 + kd
                    if not 0 <= od < 2 * D:
                        continue
                    for ih in range(H):
                        oh = 2 * ih - 1 + kh
                        if not 0 <= oh < 2 * H:
                            continue
                        ows = [2 * iw - 1 + kw for iw in range(W)]
                        keep = [iw for iw, ow in enumerate(ows) if 0 <= ow < 2 * W]
                        y[:, od, oh, [ows[iw] for iw in keep]] += t[:, i_d, ih, keep]
    return y if b is None else y + b


def op_value_and_grads(x, w, b, gy, slope, dtype):
    """{y, d_x, d_w, d_b} of the layer in ``dtype`` for the cotangent gy, detached, channels-last (d_b None without a bias)"""
    o = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w) + (() if b is None else (b,))]
    y = deconv_cl(o[0], o[1], None if b is None else o[2], slope)
    g = torch.autograd.grad(y, o, gy.to(dtype))
    return {"y": y.detach(), "d_x": g[0], "d_w": g[1], "d_b": None if b is None else g[2]}


@functools.lru_cache(maxsize=None)
def spec_tensors(spec, seed, kind="randn"):
    """(x, w, b, gy, masked share) of a layer (B, (D, H, W), Cin, Cout, bias, slope) that need not be in OP_CASES, as case_tensors
    and masked_share describe them"""
    B, (D, H, W), Cin, Cout, bias, slope = spec
    g = torch.Generator().manual_seed(seed)
    shapes = ((B, D, H, W, Cin), (Cin, Cout, 4, 4, 4), (Cout,), (B, 2 * D, 2 * H, 2 * W, Cout))
    if kind == "int":
        x, w, b, gy = (torch.randint(-3, 4, s, generator=g).float() for s in shapes)
        return x, w, (b if bias else None), gy, 0.0
    x, w, b, gy = (torch.randn(s, generator=g) for s in shapes)
    w, b = w * (1.0 / math.sqrt(8 * Cin)), (b * 0.1 if bias else None)
    masked = 0.0
    if slope is not None:
        y = deconv_cl(x.double(), w.double(), None if b is None else b.double(), slope)
        near = y.abs() < MASK_BELOW
        masked = float(near.double().mean())
        gy = torch.where(near, torch.zeros_like(gy), gy).contiguous()      # (near has the permuted strides of y: where() follows them)
    return x, w, b, gy, masked


def case_tensors(n, kind="randn", seed=None):
    """(x, w, b, gy) of case n in fp32; b is None for a case without a bias.  kind 'randn': unit-variance data, weights scaled by
    1/sqrt(8 Cin) (8 taps reach an output voxel), the cotangent zeroed where |y| < MASK_BELOW in fp64; 'int': integers in [-3, 3],
    every product and partial sum exactly representable in fp32"""
    return spec_tensors(OP_CASES[n], 3000 + n if seed is None else seed, kind)[:4]


def masked_share(n, seed=None):
    """the share of case n's outputs whose cotangent case_tensors zeroed (at most MASK_CAP: tests/test_cpu_rcn.py)"""
    return spec_tensors(OP_CASES[n], 3000 + n if seed is None else seed, "randn")[4]


# ------------------------------------------------------------------------------------------------ the network
DIMS = 3


def conv_names(c):
    """(name, cin, cout, stride) of the encoder's ConvBlocks"""
    out = [("encoder.conv1", 2, c, 2), ("encoder.conv2", c, 2 * c, 2)]
    for i, k in zip((3, 4, 5, 6), (2, 4, 8, 16)):
        out += [("encoder.conv%d.0" % i, k * c, 2 * k * c, 2), ("encoder.conv%d.1" % i, 2 * k * c, 2 * k * c, 1)]
    return out


def _block(p, name, x, stride):
    return F.leaky_relu(F.conv3d(x, p[name + ".main.weight"], p[name + ".main.bias"], stride=stride, padding=1), 0.1)


def _up(p, name, x, slope=None):
    y = F.conv_transpose3d(x, p[name + ".upconv.weight"], p.get(name + ".upconv.bias"), stride=2, padding=1)
    return y if slope is None else F.leaky_relu(y, slope)


def vtn_flow(p, moving, fixed, flow_multiplier=1.0, prefix=""):
    """VTN.forward(warp=False) on planar (B,1,D,H,W) images -> flow (B,3,D,H,W)"""
    q = {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)} if prefix else p
    x = torch.cat([moving, fixed], dim=1)
    feats = []
    for name, _, _, stride in conv_names(q["encoder.conv1.main.weight"].shape[0]):
        x = _block(q, name, x, stride)
        if name.endswith((".1", "conv1", "conv2")):
            feats.append(x)
    conv1, conv2, conv3, conv4, conv5, conv6 = feats
    w = F.conv3d(conv6, q["Pred6.weight"], q["Pred6.bias"], padding=1)
    w = _up(q, "Upsamp6to5", w)
    cat = torch.cat([conv5, _up(q, "Deconv5", conv6, 0.1), w], dim=1)
    for lvl, skip in ((5, conv4), (4, conv3), (3, conv2), (2, conv1)):
        w = F.conv3d(cat, q["Pred%d.weight" % lvl], q["Pred%d.bias" % lvl], padding=1)
        w = _up(q, "Upsamp%dto%d" % (lvl, lvl - 1), w)
        cat = torch.cat([skip, _up(q, "Deconv%d" % (lvl - 1), cat, 0.1), w], dim=1)
    return _up(q, "Pred0", cat) * flow_multiplier


def warp_planar(src, flow):
    """SpatialTransformer on planar (B,C,D,H,W) tensors: the oracle's warp"""
    return orc.warp(src, flow)


def vtn_forward(p, moving, fixed, flow_multiplier=1.0):
    """VTN(warp=True).forward -> (y_moved, flow), planar"""
    flow = vtn_flow(p, moving, fixed, flow_multiplier)
    return warp_planar(moving, flow), flow


def rcn_forward(p, moving, fixed, n_cascade, flow_multiplier=1.0):
    """RCN.forward -> (moved, flow, [subflows]), planar"""
    flow, moved, subflows = None, moving, []
    for i in range(n_cascade):
        w = vtn_flow(p, moved, fixed, flow_multiplier, prefix="vtn.%d." % i)
        subflows.append(w)
        flow = w if i == 0 else w + warp_planar(flow, w)
        moved = warp_planar(moving, flow)
    return moved, flow, subflows


def train_loss(p, moving, fixed, n_cascade, flow_multiplier=2.0, weights=(1.0, 1.0)):
    """NCC(moved) * weights[0] + sum over the subflows of Grad3d('l2') * weights[1] ("Baseline methods/RCN/train.py":106-130)
    -> (loss, moved, flow, subflows)"""
    if n_cascade == 0:                                      # one bare VTN(warp=True): NCC + Grad3d of its flow
        moved, flow = vtn_forward(p, moving, fixed, flow_multiplier)
        subflows = [flow]
    else:
        moved, flow, subflows = rcn_forward(p, moving, fixed, n_cascade, flow_multiplier)
    loss = orc.ncc_loss(fixed, moved) * weights[0]
    for w in subflows:
        loss = loss + orc.grad3d_loss(w) * weights[1]
    return loss, moved, flow, subflows


def vtn_shapes(c):
    """name -> shape of one VTN's parameters, in the reference's registration order"""
    s = {}
    for name, cin, cout, _ in conv_names(c):
        s[name + ".main.weight"], s[name + ".main.bias"] = (cout, cin, 3, 3, 3), (cout,)
    s["Pred6.weight"], s["Pred6.bias"] = (DIMS, 32 * c, 3, 3, 3), (DIMS,)
    s["Upsamp6to5.upconv.weight"] = (DIMS, DIMS, 4, 4, 4)
    s["Deconv5.upconv.weight"], s["Deconv5.upconv.bias"] = (32 * c, 16 * c, 4, 4, 4), (16 * c,)
    for lvl, k in ((5, 16), (4, 8), (3, 4), (2, 2)):
        cin = 2 * k * c + DIMS
        s["Pred%d.weight" % lvl], s["Pred%d.bias" % lvl] = (DIMS, cin, 3, 3, 3), (DIMS,)
        s["Upsamp%dto%d.upconv.weight" % (lvl, lvl - 1)] = (DIMS, DIMS, 4, 4, 4)
        s["Deconv%d.upconv.weight" % (lvl - 1)], s["Deconv%d.upconv.bias" % (lvl - 1)] = (cin, k * c // 2, 4, 4, 4), (k * c // 2,)
    s["Pred0.upconv.weight"] = (2 * c + DIMS, DIMS, 4, 4, 4)
    return s


def make_vtn_weights(channels, seed, pred0_scale=1.0, dtype=torch.float64):
    """seeded parameters of one VTN with the reference's names, fp32-representable: He-like scales that keep the activations of the
    order of one through the six levels, the flow heads small, Pred0 multiplied by ``pred0_scale``"""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, shape in vtn_shapes(channels).items():
        t = torch.randn(shape, generator=g)
        if name.endswith(".bias"):
            t = t * 0.05
        elif ".upconv." in name:
            t = t * (1.4 / math.sqrt(8 * shape[0]))             # 8 taps reach an output voxel
            if name.startswith(("Upsamp", "Pred0")):
                t = t * 0.5
        else:
            t = t * (1.4 / math.sqrt(27 * shape[1]))
            if name.startswith("Pred"):
                t = t * 0.3
        p[name] = t
    p["Pred0.upconv.weight"] = p["Pred0.upconv.weight"] * pred0_scale
    return {k: v.float().to(dtype) for k, v in p.items()}


SUBFLOW_RANGE = (0.5, 4.0)      # voxels: max |w| of every cascade's subflow on the golden pair (a condition, asserted on the CPU)


def make_weights(channels, n_cascade, moving=None, fixed=None, flow_multiplier=2.0, seed=23, dtype=torch.float64):
    """the parameters of RCN(n_cascade) ('vtn.<i>.' prefixes; n_cascade == 0: one bare VTN).  With a pair given, every cascade's
    Pred0 is scaled -- by a power of two, found by running the cascades in order in fp64 -- so that its subflow has max |w| of about
    1.5 voxels on that pair: with the reference's Normal(0, 1e-5) init the flows are about 1e-4 voxel and the warps test nothing."""
    out, flow, moved = {}, None, moving
    for i in range(max(n_cascade, 1)):
        p = make_vtn_weights(channels, seed + 101 * i, dtype=torch.float64)
        if moving is not None:
            with torch.no_grad():
                w = vtn_flow(p, moved.double(), fixed.double(), flow_multiplier)
                scale = 2.0 ** round(math.log2(1.5 / float(w.abs().max())))
                p["Pred0.upconv.weight"] = p["Pred0.upconv.weight"] * scale
                w = w * scale
                flow = w if i == 0 else w + warp_planar(flow, w)
                moved = warp_planar(moving.double(), flow)
        for k, v in p.items():
            out[("vtn.%d." % i if n_cascade else "") + k] = v.float().to(dtype)
    return out


GOLD_SHAPE, GOLD_CHANNELS, PAIR_SEED = (64, 64, 128), 4, 24
# the golden runs: tag -> (n_cascade (0: one bare VTN(warp=True)), flow_multiplier)
RUNS = {"vtn": (0, 1.0), "rcn": (2, 2.0)}


@functools.lru_cache(maxsize=None)
def golden_pair():
    """the seeded pair of the goldens (B = 2), (moving, fixed) each (2,1,64,64,128) fp32: smilecode_amd.synth.make_pair, not stored
    (8 MiB); tests/golden/e2e_rcn_64x64x128.npz keeps every STRIDE-th voxel of it to pin the generator"""
    from smilecode_amd import synth
    return tuple(torch.from_numpy(a) for a in synth.make_pair(GOLD_SHAPE, PAIR_SEED, batch=2))


@functools.lru_cache(maxsize=None)
def golden_weights(run, channels=GOLD_CHANNELS, shape=None):
    """the parameters of a golden run, scaled on the B = 2 golden pair (or on its corner crop of ``shape``)"""
    n, fm = RUNS[run]
    mov, fix = golden_pair()
    if shape is not None:
        mov, fix = (t[:, :, :shape[0], :shape[1], :shape[2]].contiguous() for t in (mov, fix))
    return make_weights(channels, n, mov, fix, fm)


def value_and_grads(p, moving, fixed, n_cascade, dtype, flow_multiplier=2.0, weights=(1.0, 1.0)):
    """one evaluation in ``dtype`` -> (loss, moved, flow, subflows, {name: gradient}), everything detached"""
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    loss, moved, flow, subflows = train_loss(q, moving.to(dtype), fixed.to(dtype), n_cascade, flow_multiplier, weights)
    names = sorted(q)
    grads = torch.autograd.grad(loss, [q[n] for n in names], allow_unused=True)
    return (loss.detach(), moved.detach(), flow.detach(), [w.detach() for w in subflows],
            {n: (torch.zeros_like(q[n]) if g is None else g.detach()) for n, g in zip(names, grads)})
