"""The fused stride-2 4x4x4 transposed convolution (ops.conv_transpose3d_k4s2, csrc/deconv.hip) beside ATen's F.conv_transpose3d in
the reference's own form -- stride 2 without padding, then the crop [1:-1] of every axis and leaky_relu(0.1) -- on channels-last
memory, on the same GPU in the same process, the sides alternating -- per Upsamp*, Deconv* and Pred0 layer of VTN with channels = 8
on a 192^3 pair: forward (no gradient wanted) and forward + backward, time (HIP events: median, minimum, maximum) and peak
allocated memory above the inputs, and both sides' error against the same layer in ATen fp64 on the GPU.  The fused side is timed
twice per round (aten, fused, fused_again): the ratio of its two medians is the spread of repeated runs of the same code.  Then
the RCN train step (n_cascade 2 and 10), eager and captured, beside ModeT's in the same process.

    python tools/bench_rcn.py [--steps 30] [--shape 192,192,192] [--channels 8] [--train-steps 30] [--json profiles/bench_rcn.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402
from tools.bench_rdn import make_modet, train_step_ms  # noqa: E402

SLOPE = 0.1


def layer_case(B, grid, Cin, Cout, bias, act, steps):
    D, H, W = grid
    g = torch.Generator(device="cuda").manual_seed(11 + Cin)
    x = torch.randn((B, D, H, W, Cin), device="cuda", generator=g)
    w = (torch.randn((Cin, Cout, 4, 4, 4), device="cuda", generator=g) / (8 * Cin) ** 0.5).requires_grad_(True)
    b = (torch.randn(Cout, device="cuda", generator=g) * 0.1).requires_grad_(True) if bias else None
    gy = torch.randn((B, 2 * D, 2 * H, 2 * W, Cout), device="cuda", generator=g)
    slope = SLOPE if act else None

    def ref_layer(a, wt, bt):
        y = F.conv_transpose3d(a, wt, bt, stride=2)[:, :, 1:-1, 1:-1, 1:-1]
        return F.leaky_relu(y, SLOPE) if act else y

    n_kink = 0
    if act:     # the cotangent is zeroed where fp32 and fp64 may take different branches of LeakyReLU (|y| < 1e-5 in fp64)
        with torch.no_grad():
            y_ref = ref_layer(x.permute(0, 4, 1, 2, 3).double(), w.detach().double(), b.detach().double())
            near_kink = y_ref.permute(0, 2, 3, 4, 1).abs() < 1e-5
            gy = (gy * ~near_kink).contiguous()
            n_kink = int(near_kink.sum())
            del y_ref, near_kink
    x_nc, gy_nc = x.permute(0, 4, 1, 2, 3), gy.permute(0, 4, 1, 2, 3)          # channels_last_3d views of the same bytes
    params = [w] + ([b] if bias else [])

    def fused(a):
        return ops.conv_transpose3d_k4s2(a, w, b, slope)

    def aten(a):
        return ref_layer(a, w, b)

    def fwd(fn, a):
        with torch.no_grad():
            return fn(a)

    def fwd_bwd(fn, a, c):
        a = a.detach().requires_grad_(True)
        return torch.autograd.grad(fn(a), [a] + params, c)

    sides = {"aten": (lambda: fwd(aten, x_nc), lambda: fwd_bwd(aten, x_nc, gy_nc)),
             "fused": (lambda: fwd(fused, x), lambda: fwd_bwd(fused, x, gy))}
    sides["fused_again"] = sides["fused"]
    nx, ny = x.numel(), gy.numel()
    ya = 2 if act else 1
    algo = {"fwd": 4.0 * (nx + ny), "fwd_bwd": 4.0 * (nx + ny) + 4.0 * (nx + ya * ny) + 4.0 * (nx + ya * ny)}
    r = {"B": B, "grid": list(grid), "Cin": Cin, "Cout": Cout, "bias": bias, "act": act, "input_bytes": 4 * nx, "output_bytes": 4 * ny,
         "flop_fwd": 128.0 * Cin * Cout * (nx // Cin), "outputs_near_kink_with_zero_cotangent": n_kink}
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
    x64 = x_nc.double().requires_grad_(True)
    p64 = [t.detach().double().requires_grad_(True) for t in params]
    y64 = ref_layer(x64, p64[0], p64[1] if bias else None)
    g64 = torch.autograd.grad(y64, [x64] + p64, gy_nc.double())
    names = ["d_x", "d_w"] + (["d_b"] if bias else [])
    # (the planar fp64 d_x against the fused side's channels-last one: by name, a 3x3x3 grid of 3 channels has the same shape in both)
    cl = lambda n, a: a.permute(0, 2, 3, 4, 1) if n == "d_x" else a      # noqa: E731
    err = lambda got, ref: float((got.double() - ref).abs().max() / ref.abs().max())      # noqa: E731
    r["error_vs_fp64"] = {"fused": {"y": err(fwd(fused, x), y64.detach().permute(0, 2, 3, 4, 1))},
                          "aten": {"y": err(fwd(aten, x_nc), y64.detach())}}
    for n, f, a, ref in zip(names, gf, ga, g64):
        r["error_vs_fp64"]["fused"][n] = err(f, cl(n, ref))
        r["error_vs_fp64"]["aten"][n] = err(a, ref)
    del x64, y64, g64
    timer = ops.KernelTimer()          # per-kernel times of one fused forward + backward (HIP events around each launch)
    ops.set_kernel_timer(timer)
    try:
        for _ in range(5):
            sides["fused"][1]()
    finally:
        ops.set_kernel_timer(None)
    r["fused_kernels_ms"] = {k: v["ms"] / v["calls"] for k, v in timer.summary().items()}
    return r


def vtn_layers(shape, c):
    """(name, input grid, Cin, Cout, bias, act) of every transposed convolution of VTN"""
    g = lambda k: tuple(s // k for s in shape)          # noqa: E731
    out = [("Upsamp6to5", g(64), 3, 3, False, False), ("Deconv5", g(64), 32 * c, 16 * c, True, True)]
    for lvl, k in ((5, 16), (4, 8), (3, 4), (2, 2)):
        cin = 2 * k * c + 3
        out += [("Upsamp%dto%d" % (lvl, lvl - 1), g(2 ** lvl), 3, 3, False, False),
                ("Deconv%d" % (lvl - 1), g(2 ** lvl), cin, k * c // 2, True, True)]
    return out + [("Pred0", g(2), 2 * c + 3, 3, False, False)]


def make_rcn(shape, channels, n_cascade):
    """the reference's initialisation except for Pred0: Normal(0, 1e-5) leaves every flow at zero, so it gets weights that move the
    flow by a fraction of a voxel"""
    torch.manual_seed(24)
    m = models.RCN(shape, flow_multiplier=2, channels=channels, n_cascade=n_cascade, return_subflows=True).cuda()
    g = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for v in m.vtn:
            w = v.Pred0.upconv.weight
            w.copy_(torch.randn(w.shape, generator=g) * (0.05 / (8 * w.shape[0]) ** 0.5))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shape", default="192,192,192")
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--cascades", default="2,10")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rcn.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    c = args.channels
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_rcn.json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "channels": c, "iterations": args.steps,
           "form": "plain fp32 FMA on LDS tiles (no matrix-instruction form is built)", "layers": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for name, grid, cin, cout, bias, act in vtn_layers(shape, c):
        res["layers"]["%s,%dx%dx%d,%d->%d" % ((name,) + grid + (cin, cout))] = layer_case(1, grid, cin, cout, bias, act, args.steps)
        torch.cuda.empty_cache()
        save()
    if args.train_steps > 0:
        res["train_step"] = {}
        makes = [("rcn%d" % int(n), (lambda s, n=int(n): make_rcn(s, c, n))) for n in args.cascades.split(",") if n]
        for name, make in makes + [("modet", make_modet)]:
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
