"""The fused stride-2 convolution (ops.conv3d_s2, csrc/convs2.hip) beside ATen's F.conv3d(stride=2, padding=1) + leaky_relu(0.2) in
channels-last memory format, on the same GPU in the same process, the sides alternating -- per encoder layer of RDN with
channels = 16 at the [moving; fixed] batch of a 160x192x160 pair: forward (no gradient wanted) and forward + backward, time (HIP
events: median, minimum, maximum) and peak allocated memory above the inputs.  The fused side is timed twice per round (aten,
fused, fused_again): the ratio of its two medians is the spread of repeated runs of the same code.  The first layer's input is
the image: neither side computes a data gradient for it.  Then the RDN train step (channels = 16, one pass per level), eager and
captured, beside ModeT's.

    python tools/bench_rdn.py [--steps 30] [--shape 160,192,160] [--channels 16] [--train-steps 30] [--json profiles/bench_rdn.json]

The layer's ALGORITHMIC bytes: forward 4 (|x| + |y|); the backward reads x, d_y and y once more for the weight gradient and d_y, y
for the data gradient and writes d_x; ``achieved_gbps`` divides them by the fused side's median time.  ``error_vs_fp64``: both sides
against the same layer in ATen fp64 on the GPU, max|got - ref| / max|ref| per result."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops, synth  # noqa: E402
from smilecode_amd.engine import Trainer  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402

SLOPE = 0.2


def layer_case(B, grid, Cin, Cout, steps, x_grad):
    D, H, W = grid
    g = torch.Generator(device="cuda").manual_seed(7 + Cin)
    x = torch.randn((B, D, H, W, Cin), device="cuda", generator=g)
    w = (torch.randn((Cout, Cin, 3, 3, 3), device="cuda", generator=g) / (27 * Cin) ** 0.5).requires_grad_(True)
    b = (torch.randn(Cout, device="cuda", generator=g) * 0.1).requires_grad_(True)
    Do, Ho, Wo = ops.conv3d_s2_out_shape(D, H, W)
    gy = torch.randn((B, Do, Ho, Wo, Cout), device="cuda", generator=g)
    # LeakyReLU has a kink at 0: where |y| is within rounding of it, fp32 and fp64 can take different branches of the derivative and
    # one such element moves a gradient by 0.8 d_y times its factor.  The cotangent is zeroed there (|y| < 1e-5 in fp64: a few of
    # the millions of outputs), so that error_vs_fp64 below measures arithmetic, not the branch.
    with torch.no_grad():
        y_ref = F.leaky_relu(F.conv3d(x.permute(0, 4, 1, 2, 3).double(), w.detach().double(), b.detach().double(), stride=2, padding=1), SLOPE)
        near_kink = y_ref.permute(0, 2, 3, 4, 1).abs() < 1e-5
        gy = (gy * ~near_kink).contiguous()
        n_kink = int(near_kink.sum())
        del y_ref, near_kink
    # the same bytes as a (B,C,D,H,W) tensor in channels_last_3d memory format: what ATen's channels-last path takes
    x_nc, gy_nc = x.permute(0, 4, 1, 2, 3), gy.permute(0, 4, 1, 2, 3)
    w_cl = w.detach().contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)

    def fused(a):
        return ops.conv3d_s2(a, w, b, SLOPE)

    def aten(a):
        return F.leaky_relu(F.conv3d(a, w_cl, b, stride=2, padding=1), SLOPE)

    def fwd(fn, a):
        with torch.no_grad():
            return fn(a)

    def fwd_bwd(fn, a, c, wt):
        a = a.detach().requires_grad_(x_grad)
        return torch.autograd.grad(fn(a), ([a] if x_grad else []) + [wt, b], c)

    sides = {"aten": (lambda: fwd(aten, x_nc), lambda: fwd_bwd(aten, x_nc, gy_nc, w_cl)),
             "fused": (lambda: fwd(fused, x), lambda: fwd_bwd(fused, x, gy, w))}
    sides["fused_again"] = sides["fused"]
    nx, ny = x.numel(), gy.numel()
    algo = {"fwd": 4.0 * (nx + ny), "fwd_bwd": 4.0 * (nx + ny) + 4.0 * (nx + 2 * ny) + (4.0 * (nx + 2 * ny) if x_grad else 0.0)}
    r = {"B": B, "grid": list(grid), "Cin": Cin, "Cout": Cout, "input_bytes": 4 * nx, "output_bytes": 4 * ny, "x_grad": x_grad,
         "flop_fwd": 54.0 * Cin * Cout * (ny // Cout), "outputs_near_kink_with_zero_cotangent": n_kink}
    for leg, idx in (("fwd", 0), ("fwd_bwd", 1)):
        for _ in range(3):
            for s in sides.values():
                s[idx]()
        ts = {k: [] for k in sides}
        for _ in range(steps):
            for k, s in sides.items():
                ts[k].append(once(s[idx]))
        r[leg] = {k: stats(v) for k, v in ts.items()}
        for k in ("fused", "aten"):
            r[leg][k]["peak_bytes"] = peak_above(sides[k][idx])
        r[leg]["algorithmic_bytes"] = algo[leg]
        r[leg]["fused"]["achieved_gbps"] = algo[leg] / (r[leg]["fused"]["ms"] * 1e-3) / 1e9
        r[leg]["aten_over_fused_time"] = r[leg]["aten"]["ms"] / r[leg]["fused"]["ms"]
        r[leg]["fused_again_over_fused_time"] = r[leg]["fused_again"]["ms"] / r[leg]["fused"]["ms"]
        r[leg]["aten_over_fused_peak"] = r[leg]["aten"]["peak_bytes"] / max(r[leg]["fused"]["peak_bytes"], 1)
    gf, ga = sides["fused"][1](), sides["aten"][1]()
    # (ATen's d_x comes back as a (B,C,D,H,W) view of channels-last memory; d_w and d_b have the same shape on both sides)
    r["grad_fused_vs_aten_maxdiff_of_max"] = max(
        float((f - (a if a.shape == f.shape else a.permute(0, 2, 3, 4, 1))).abs().max() / a.abs().max()) for f, a in zip(gf, ga))
    # both sides against the same layer in ATen fp64 on this GPU: max|got - ref| / max|ref| per result
    x64 = x_nc.double().requires_grad_(x_grad)
    w64, b64 = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    y64 = F.leaky_relu(F.conv3d(x64, w64, b64, stride=2, padding=1), SLOPE)
    g64 = torch.autograd.grad(y64, ([x64] if x_grad else []) + [w64, b64], gy_nc.double())
    names = (["d_x"] if x_grad else []) + ["d_w", "d_b"]
    cl = lambda a, f: a if a.shape == f.shape else a.permute(0, 2, 3, 4, 1)      # noqa: E731
    err = lambda got, ref: float((got.double() - ref).abs().max() / ref.abs().max())      # noqa: E731
    r["error_vs_fp64"] = {"fused": {"y": err(fwd(fused, x), y64.detach().permute(0, 2, 3, 4, 1))},
                          "aten": {"y": err(fwd(aten, x_nc), y64.detach())}}
    for n, f, a, ref in zip(names, gf, ga, g64):
        r["error_vs_fp64"]["fused"][n] = err(f, cl(ref, f))
        r["error_vs_fp64"]["aten"][n] = err(a, ref)
    del x64, y64, g64
    # per-kernel times of one fused forward + backward (HIP events around each launch)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        for _ in range(5):
            sides["fused"][1]()
    finally:
        ops.set_kernel_timer(None)
    r["fused_kernels_ms"] = {k: v["ms"] / v["calls"] for k, v in timer.summary().items()}
    return r


def train_step_ms(model, shape, steps, capture, warmup=5):
    mov, fix = (torch.from_numpy(v).cuda() for v in synth.make_pair(shape, 24, 1))
    tr = Trainer(model)
    if capture:
        tr.capture(mov, fix)
    for _ in range(warmup):
        tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    return {"ms_per_step": (time.perf_counter() - t0) * 1e3 / steps, "loss": float(out[0]), "peak_allocated_bytes": torch.cuda.max_memory_allocated()}


def make_rdn(shape, channels):
    """the reference's initialisation except for the flow convolutions: Normal(0, 1e-5) leaves every field at zero, so they get
    weights that move the flow by a fraction of a voxel"""
    torch.manual_seed(24)
    m = models.RDN(shape, channels=channels).cuda()
    g = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for est in (m.est0[0], m.est1[0], m.est2[0], m.est3[0]):
            w = est.conv[4].weight
            w.copy_(torch.randn(w.shape, generator=g) * (0.3 / (27 * w.shape[1]) ** 0.5))
    return m


def make_modet(shape):
    m = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rdn.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    c = args.channels
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_rdn.json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "channels": c, "iterations": args.steps, "layers": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for i, (cin, cout) in enumerate([(1, c), (c, 2 * c), (2 * c, 4 * c), (4 * c, 8 * c)]):
        grid = tuple(s // 2 ** i for s in shape)
        res["layers"]["conv%d,%dx%dx%d,%d->%d" % ((i,) + grid + (cin, cout))] = layer_case(2, grid, cin, cout, args.steps, x_grad=i > 0)
        torch.cuda.empty_cache()
        save()
    if args.train_steps > 0:
        res["train_step"] = {}
        for name, make in (("rdn", lambda s: make_rdn(s, c)), ("modet", make_modet)):
            for capture in (False, True):
                key = "%s,%s" % (name, "captured" if capture else "eager")
                try:
                    res["train_step"][key] = train_step_ms(make(shape), shape, args.train_steps, capture)
                except RuntimeError as e:                 # a refused width or an allocation failure is a result, not a crash of the tool
                    res["train_step"][key] = {"error": str(e)[:400]}
                torch.cuda.empty_cache()
                save()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
