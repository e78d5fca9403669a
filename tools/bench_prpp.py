"""The fused operators of the PR++ family (ops.upsample_nearest_cat, ops.relu_add, ops.corr_stack, ops.compose_cross; csrc/prpp.hip)
beside their ATen compositions as "Baseline methods/PR++/models.py" writes them, on the same GPU in the same process, the sides
alternating, at the level shapes of the default network (first_channel = 8, 160 x 192 x 160): the decoder input of decoder1..4 on
the [moving; fixed] batch of two, x + relu(res) and the stack of the five blocks, the three cross-grid compositions.  For the stack
a second table has the composition on the tree's other operators (correlation3d -> to_channels_last -> two cat_channels) in ATen's
place.  Per case forward (no gradient wanted) and forward + backward: time (HIP events: median, minimum, maximum), peak allocated
memory above the inputs, the fused side's algorithmic bytes over its median time, and both sides' error against the ATen
composition in fp64 on the GPU.  The fused side is timed twice per round (aten, fused, fused_again): the ratio of its two medians
is the spread of repeated runs of the same code.  Then the PR++ train step, eager and captured, beside ModeT's.

    python tools/bench_prpp.py [--steps 30] [--shape 160,192,160] [--channels 8] [--train-steps 30] [--json profiles/bench_prpp.json]"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops  # noqa: E402
from tools import bench_layer  # noqa: E402
from tools.bench_pcnet import measure, planar  # noqa: E402


def aten_upcat(x, skip):
    return torch.cat([F.interpolate(planar(x), scale_factor=2, mode="nearest"), planar(skip)], dim=1)


def aten_relu_add(x, t):
    return planar(x) + torch.relu(planar(t))


def box3(x, pad):
    """the all-ones grouped 3x3x3 convolution with zero padding ``pad`` >= 1, as a pooling sum (any dtype)"""
    if pad > 1:
        x = F.pad(x, (pad - 1,) * 6)
    return F.avg_pool3d(x, 3, stride=1, padding=1, count_include_pad=True) * 27.0


def aten_stack(mov, fix):
    """torch.cat([x, Correlation3D(x, y), y], 1) ("Baseline methods/PR++/models.py":228-242, :278)"""
    m, f = planar(mov), planar(fix)
    D, H, W = m.shape[2:]
    pm, pf = box3(m, 1), box3(f, 3)
    corr = [(pm * pf[:, :, 2 * i:2 * i + D, 2 * j:2 * j + H, 2 * k:2 * k + W]).sum(1, keepdim=True)
            for i in range(3) for j in range(3) for k in range(3)]
    return torch.cat([m, torch.cat(corr, dim=1) / 27.0, f], dim=1)


def existing_stack(mov, fix):
    """the same rows from the operators the tree had before this family; planar view for ``measure``"""
    corr = ops.to_channels_last(ops.correlation3d(mov, fix))
    return planar(ops.cat_channels(ops.cat_channels(mov, corr), fix))


def aten_compose(src, w):
    """SpatialTransformer(w's size)(src, w) + w (":49-67, :339)"""
    flow = planar(w)
    shape = flow.shape[2:]
    grid = torch.stack(torch.meshgrid([torch.arange(0, s, device=w.device) for s in shape], indexing="ij")).unsqueeze(0).to(w.dtype)
    locs = grid + flow
    locs = torch.stack([2 * (locs[:, i] / (shape[i] - 1) - 0.5) for i in range(3)], dim=1).permute(0, 2, 3, 4, 1)[..., [2, 1, 0]]
    return F.grid_sample(planar(src), locs, align_corners=True, mode="bilinear") + flow


def cases(shape, c, steps):
    g = torch.Generator(device="cuda").manual_seed(19)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)          # noqa: E731
    grid = lambda k: tuple(s // k for s in shape)                       # noqa: E731
    name = lambda op, tag, gr: "%s,%s,%dx%dx%d" % ((op, tag) + gr)      # noqa: E731
    for k, C1, C2 in ((16, 4 * c, 4 * c), (8, 4 * c, 2 * c), (4, 4 * c, 2 * c), (2, 2 * c, c)):     # decoder1 .. decoder4, both images
        x, skip = rn(2, *grid(k), C1), rn(2, *grid(k // 2), C2)
        gy = rn(2, *grid(k // 2), C1 + C2)
        moved = 4.0 * (x.numel() + skip.numel() + gy.numel())
        yield name("upcat", "%d+%d" % (C1, C2), grid(k // 2)), measure([x, skip], [], gy, ops.upsample_nearest_cat, aten_upcat, moved, moved, steps)
        del x, skip, gy
        torch.cuda.empty_cache()
    for k, C in ((8, 4 * c), (4, 4 * c), (2, 2 * c), (1, 2 * c), (1, c)):                          # prblock1 .. prblock5
        x, t = rn(1, *grid(k), C), rn(1, *grid(k), C)
        yield name("relu_add", "C%d" % C, grid(k)), measure([x, t], [], x, ops.relu_add, aten_relu_add, 12.0 * x.numel(), 12.0 * x.numel(), steps)
        mov, fix, gy = rn(1, *grid(k), C), rn(1, *grid(k), C), rn(1, *grid(k), 2 * C + 27)
        n = float(mov.numel() // C)
        fwd, bwd = 4.0 * n * (4 * C + 27), 4.0 * n * (6 * C + 27)
        yield name("stack", "C%d" % C, grid(k)), measure([mov, fix], [], gy, ops.corr_stack, aten_stack, fwd, bwd, steps)
        yield name("stack_vs_existing_ops", "C%d" % C, grid(k)), measure([mov, fix], [], gy, ops.corr_stack, existing_stack, fwd, bwd, steps,
                                                                             ref=aten_stack)
        del x, t, mov, fix, gy
        torch.cuda.empty_cache()
    for k in (8, 4, 2):                                                                            # transformers[2], [1], [0] across grids
        src, w = 0.7 * rn(1, *grid(k), 3), 0.7 * rn(1, *grid(k // 2), 3)
        gy = rn(1, *grid(k // 2), 3)
        fwd = 4.0 * (src.numel() + 2 * w.numel())
        bwd = 4.0 * (2 * src.numel() + 3 * w.numel()) + 16.0 * src.numel()                         # + the int64 sums, written and read
        yield name("compose", "x2", grid(k // 2)), measure([src, w], [], gy, ops.compose_cross, aten_compose, fwd, bwd, steps)
        del src, w, gy
        torch.cuda.empty_cache()


def make_prpp(shape, channels):
    torch.manual_seed(24)
    m = models.PRNetplusplus(shape, first_channel=channels).cuda()
    with torch.no_grad():                       # fields of a fraction of a voxel instead of the N(0, 1e-5) identity
        for k in range(1, 6):
            getattr(m, "prblock%d" % k).flow.weight.mul_(2.0 ** 12)
    return m


def main():
    ap = bench_layer.parser("160,192,160", 8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_prpp.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_prpp.json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "channels": args.channels, "iterations": args.steps, "ops": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for name, measured in cases(shape, args.channels, args.steps):
        res["ops"][name] = measured
        print(name, json.dumps({leg: {k: measured[leg][k] for k in ("aten_over_fused_time", "fused_again_over_fused_time")}
                                for leg in ("fwd", "fwd_bwd")}), flush=True)
        save()
    if args.train_steps > 0:
        res["train_step"] = {}
        for name, make in (("prpp", lambda s: make_prpp(s, args.channels)), ("modet", bench_layer.make_modet)):
            for capture in (False, True):
                key = "%s,%s" % (name, "captured" if capture else "eager")
                try:
                    res["train_step"][key] = bench_layer.train_step_ms(make(shape), shape, args.train_steps, capture)
                except RuntimeError as e:                 # an allocation failure is a result, not a crash of the tool
                    res["train_step"][key] = {"error": str(e)[:400]}
                torch.cuda.empty_cache()
                save()
    print(json.dumps(res["train_step"] if args.train_steps > 0 else {}))
    save()


if __name__ == "__main__":
    main()
