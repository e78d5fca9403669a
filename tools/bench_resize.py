"""The resize family (ops.resize, ops.flow_pyramid, csrc/resize.hip) beside the ATen composition it replaces, F.interpolate(mode=
'trilinear', align_corners=True) times the factor on a (B,3,D,H,W) view of the same bytes, on the same GPU in the same process, the
sides alternating -- on a 3-channel field of 80x96x80 (the flow of a 160x192x160 pair, where a recursive RDN stage builds its
pyramid): the single resize to 1/2 and the pyramid (1/2, 1/4, 1/8), forward (no gradient wanted) and forward + backward, time
(HIP events around synchronised work: median, minimum, maximum), peak allocated memory above the inputs, and the error of either
side against ATen fp64.  The fused pyramid is also timed beside three ops.resize calls.  Then the train step of RDNStages at
160x192x160 with channels = 16, at 1, 2 and 4 stages with levels 1111 and 4444 (unshared), beside models.RDN's one stage, eager and
captured.

    python tools/bench_resize.py [--steps 30] [--shape 80,96,80] [--train-shape 160,192,160] [--channels 16] [--train-steps 30]
                                 [--json profiles/bench_resize.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops  # noqa: E402
from tools.bench_layer import train_step_ms  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402

PYRAMID = ((2, 0.5), (4, 0.25), (8, 0.125))


def aten_resize(x_nc, size, scale):
    return scale * F.interpolate(x_nc, size=size, mode="trilinear", align_corners=True)


def measure(sides, steps):
    """sides: name -> (forward(), forward_backward()); every side timed ``steps`` times, alternating, after three warm-up rounds"""
    r = {}
    for leg, idx in (("fwd", 0), ("fwd_bwd", 1)):
        for _ in range(3):
            for s in sides.values():
                s[idx]()
        ts = {k: [] for k in sides}
        for _ in range(steps):
            for k, s in sides.items():
                ts[k].append(once(s[idx]))
        r[leg] = {k: stats(v) for k, v in ts.items()}
        for k in sides:
            if not k.endswith("_again"):
                r[leg][k]["peak_bytes"] = peak_above(sides[k][idx])
    return r


def err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def single_case(x, steps):
    """x (B,D,H,W,3) -> 0.5 * resize to S // 2"""
    size = tuple(s // 2 for s in x.shape[1:4])
    g = torch.Generator(device="cuda").manual_seed(3)
    gy = torch.randn((x.shape[0],) + size + (3,), device="cuda", generator=g)
    x_nc, gy_nc = x.permute(0, 4, 1, 2, 3), gy.permute(0, 4, 1, 2, 3)

    def fb(fn, a, c):
        a = a.detach().requires_grad_(True)
        return torch.autograd.grad(fn(a), [a], c)[0]

    def nograd(fn, a):
        with torch.no_grad():
            return fn(a)
    hip = lambda a: ops.resize(a, size, 0.5)            # noqa: E731
    aten = lambda a: aten_resize(a, size, 0.5)          # noqa: E731
    sides = {"aten": (lambda: nograd(aten, x_nc), lambda: fb(aten, x_nc, gy_nc)), "fused": (lambda: nograd(hip, x), lambda: fb(hip, x, gy))}
    sides["fused_again"] = sides["fused"]
    r = measure(sides, steps)
    x64 = x_nc.double().requires_grad_(True)
    y64 = aten(x64)
    (d64,) = torch.autograd.grad(y64, [x64], gy_nc.double())
    cl = lambda t: t.permute(0, 2, 3, 4, 1)             # noqa: E731
    r["error_vs_fp64"] = {"fused": {"out": err(nograd(hip, x), cl(y64.detach())), "d_x": err(fb(hip, x, gy), cl(d64))},
                          "aten": {"out": err(nograd(aten, x_nc), y64.detach()), "d_x": err(fb(aten, x_nc, gy_nc), d64)}}
    r["algorithmic_bytes"] = {"fwd": 4.0 * (x.numel() + gy.numel()), "fwd_bwd": 8.0 * (x.numel() + gy.numel())}
    return r


def pyramid_case(x, steps):
    sizes = ops.flow_pyramid_sizes(*x.shape[1:4])
    g = torch.Generator(device="cuda").manual_seed(4)
    gys = [torch.randn((x.shape[0],) + s + (3,), device="cuda", generator=g) for s in sizes]
    x_nc, gys_nc = x.permute(0, 4, 1, 2, 3), [t.permute(0, 4, 1, 2, 3) for t in gys]
    hip = lambda a: ops.flow_pyramid(a)                                                                 # noqa: E731
    three = lambda a: tuple(ops.resize(a, s, sc) for s, (_, sc) in zip(sizes, PYRAMID))                 # noqa: E731
    aten = lambda a: tuple(aten_resize(a, s, sc) for s, (_, sc) in zip(sizes, PYRAMID))                 # noqa: E731

    def fb(fn, a, cs):
        a = a.detach().requires_grad_(True)
        return torch.autograd.grad(fn(a), [a], cs)[0]

    def nograd(fn, a):
        with torch.no_grad():
            return fn(a)
    sides = {"aten": (lambda: nograd(aten, x_nc), lambda: fb(aten, x_nc, gys_nc)),
             "fused": (lambda: nograd(hip, x), lambda: fb(hip, x, gys)),
             "three_resize": (lambda: nograd(three, x), lambda: fb(three, x, gys))}
    sides["fused_again"] = sides["fused"]
    r = measure(sides, steps)
    x64 = x_nc.double().requires_grad_(True)
    y64 = aten(x64)
    (d64,) = torch.autograd.grad(y64, [x64], [t.double() for t in gys_nc])
    cl = lambda t: t.permute(0, 2, 3, 4, 1)             # noqa: E731
    r["error_vs_fp64"] = {}
    for name, fn, a, cs, conv in (("fused", hip, x, gys, cl), ("three_resize", three, x, gys, cl), ("aten", aten, x_nc, gys_nc, lambda t: t)):
        ys = nograd(fn, a)
        r["error_vs_fp64"][name] = {"out_worst": max(err(y, conv(w.detach())) for y, w in zip(ys, y64)), "d_x": err(fb(fn, a, cs), conv(d64))}
    r["fused_equals_three_resize_bitwise"] = all(torch.equal(p, q) for p, q in zip(nograd(hip, x), nograd(three, x)))
    nout = sum(t.numel() for t in gys)
    r["algorithmic_bytes"] = {"fwd": 4.0 * (x.numel() + nout), "fwd_bwd": 8.0 * (x.numel() + nout)}
    for leg in ("fwd", "fwd_bwd"):
        r[leg]["aten_over_fused_time"] = r[leg]["aten"]["ms"] / r[leg]["fused"]["ms"]
        r[leg]["three_resize_over_fused_time"] = r[leg]["three_resize"]["ms"] / r[leg]["fused"]["ms"]
        r[leg]["fused_again_over_fused_time"] = r[leg]["fused_again"]["ms"] / r[leg]["fused"]["ms"]
    return r


def make_net(cls, shape, channels, **kw):
    """the reference's initialisation except for the flow convolutions: Normal(0, 1e-5) leaves every field at zero, so they get
    weights that move the flow by a fraction of a voxel (tools/bench_rdn.py's)"""
    torch.manual_seed(24)
    m = cls(shape, channels=channels, **kw).cuda()
    g = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("conv.4.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * (0.3 / (27 * p.shape[1]) ** 0.5))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shape", default="80,96,80", help="the field the operators are measured on")
    ap.add_argument("--train-shape", default="160,192,160")
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--train-steps", type=int, default=30, help="0: operators only")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resize.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    tshape = tuple(int(s) for s in args.train_shape.split(","))
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_resize.json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "train_shape": list(tshape), "channels": args.channels,
           "iterations": args.steps}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    x = torch.randn((1,) + shape + (3,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    res["resize_half"] = single_case(x, args.steps)
    for leg in ("fwd", "fwd_bwd"):
        r = res["resize_half"][leg]
        r["aten_over_fused_time"] = r["aten"]["ms"] / r["fused"]["ms"]
        r["fused_again_over_fused_time"] = r["fused_again"]["ms"] / r["fused"]["ms"]
    save()
    res["pyramid"] = pyramid_case(x, args.steps)
    save()
    if args.train_steps > 0:
        res["train_step"] = {}
        nets = [("rdn,stages1,levels1111", lambda: make_net(models.RDN, tshape, args.channels))]
        for stages in (1, 2, 4):
            for lv in (1, 4):
                nets.append(("rdnstages,stages%d,levels%s" % (stages, str(lv) * 4),
                             lambda stages=stages, lv=lv: make_net(models.RDNStages, tshape, args.channels, stage_recursion=stages,
                                                                   level_recursion=[lv] * 4, return_stage_flows=True)))
        for name, make in nets:
            for capture in (False, True):
                key = "%s,%s" % (name, "captured" if capture else "eager")
                try:
                    res["train_step"][key] = train_step_ms(make(), tshape, args.train_steps, capture)
                except RuntimeError as e:                 # an allocation failure is a result, not a crash of the tool
                    res["train_step"][key] = {"error": str(e)[:400]}
                torch.cuda.empty_cache()
                save()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
