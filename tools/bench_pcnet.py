"""The fused operators of the PCNet family (ops.upsample_pow2, ops.dfi_gate, ops.nff_fuse, ops.residual_add; csrc/pcnet.hip) beside
their ATen compositions as "Baseline methods/PCnet/models.py" writes them, on the same GPU in the same process, the sides
alternating, at the shapes of the default network (channels = 16, 160 x 192 x 160): NFF at C = 16, 32 and 64 (levels 0, 1, 2), DFI
at n = 1, 2 and 3 (levels 2, 1, 0: the upsamplings into one buffer beside Upsample + cat, and the gated sum).  Per case forward (no
gradient wanted) and forward + backward: time (HIP events: median, minimum, maximum), peak allocated memory above the inputs, the
fused side's algorithmic bytes over its median time, and both sides' error against the same composition in ATen fp64 on the GPU.
The fused side is timed twice per round (aten, fused, fused_again): the ratio of its two medians is the spread of repeated runs of
the same code.  Then the PCNet train step, eager and captured, beside ModeT's.

    python tools/bench_pcnet.py [--steps 30] [--shape 160,192,160] [--channels 16] [--train-steps 30] [--json profiles/bench_pcnet.json]"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops  # noqa: E402
from tools import bench_layer  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402


def planar(t):
    return t.permute(0, 4, 1, 2, 3)


def aten_nff(t0, t1, t2, lg, W1, W2):
    """NFFBlock.forward's tail on channels_last_3d views of the same bytes"""
    wm = torch.softmax(planar(lg), dim=1)
    cat = torch.cat([planar(t0) * wm[:, 0:1], planar(t1) * wm[:, 1:2], planar(t2) * wm[:, 2:3]], dim=1)
    b, c = cat.shape[:2]
    fc = lambda v: F.linear(torch.relu(F.linear(v, W1)), W2)        # noqa: E731
    g = torch.sigmoid(fc(F.adaptive_avg_pool3d(cat, 1).view(b, c)) + fc(F.adaptive_max_pool3d(cat, 1).view(b, c)))
    return cat * g.view(b, c, 1, 1, 1)


def aten_dfi_up(*preds):
    n = len(preds)
    return torch.cat([F.interpolate(planar(p), scale_factor=2 ** (n - i), mode="trilinear", align_corners=True)
                      for i, p in enumerate(preds)], dim=1)


def fused_dfi_up(*preds):
    n = len(preds)
    B, d, h, w, _ = preds[0].shape
    f = 2 ** n
    x = torch.empty((B, f * d, f * h, f * w, 3 * n), device=preds[0].device)
    for i, p in enumerate(preds):
        x = ops.upsample_pow2(p, 2 ** (n - i), x, 3 * i)
    return x


def aten_dfi_gate(x, lg):
    out = None
    for i in range(x.shape[-1] // 3):
        term = planar(x)[:, 3 * i:3 * i + 3] * torch.sigmoid(planar(lg)[:, 3 * i:3 * i + 3])
        out = term if out is None else out + term
    return out


def measure(leaves, consts, gy, fused, aten, algo_fwd, algo_bwd, steps, ref=None):
    """``ref``: the composition evaluated in fp64 as the reference (default: ``aten`` itself).  ``leaves``: channels-last tensors both sides differentiate with respect to; ``consts``: further arguments; the ATen side
    returns a planar (B,C,D,H,W) result, compared with the fused side's channels-last one through a permuted view"""
    def fwd(fn):
        with torch.no_grad():
            return fn(*leaves, *consts)

    def fwd_bwd(fn, cot):
        ls = [t.detach().requires_grad_(True) for t in leaves]
        return torch.autograd.grad(fn(*ls, *consts), ls, cot)

    gy_p = planar(gy)
    sides = {"aten": (lambda: fwd(aten), lambda: fwd_bwd(aten, gy_p)), "fused": (lambda: fwd(fused), lambda: fwd_bwd(fused, gy))}
    sides["fused_again"] = sides["fused"]
    r = {"input_bytes": 4 * sum(t.numel() for t in leaves), "output_bytes": 4 * gy.numel()}
    for leg, idx, algo in (("fwd", 0, algo_fwd), ("fwd_bwd", 1, algo_fwd + algo_bwd)):
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
        r[leg]["algorithmic_bytes"] = algo
        r[leg]["fused"]["achieved_gbps"] = algo / (r[leg]["fused"]["ms"] * 1e-3) / 1e9
        r[leg]["aten_over_fused_time"] = r[leg]["aten"]["ms"] / r[leg]["fused"]["ms"]
        r[leg]["fused_again_over_fused_time"] = r[leg]["fused_again"]["ms"] / r[leg]["fused"]["ms"]
        r[leg]["aten_over_fused_peak"] = r[leg]["aten"]["peak_bytes"] / max(r[leg]["fused"]["peak_bytes"], 1)
    err = lambda got, want: float((got.double() - want).abs().max() / want.abs().max())      # noqa: E731
    l64 = [t.detach().double().requires_grad_(True) for t in leaves]
    y64 = (ref or aten)(*l64, *(c.double() for c in consts))
    g64 = torch.autograd.grad(y64, l64, gy_p.double())
    r["error_vs_fp64"] = {"fused": {"y": err(planar(fwd(fused)), y64.detach())}, "aten": {"y": err(fwd(aten), y64.detach())}}
    for i, (f, a, want) in enumerate(zip(sides["fused"][1](), sides["aten"][1](), g64)):
        r["error_vs_fp64"]["fused"]["d%d" % i] = err(f, want)
        r["error_vs_fp64"]["aten"]["d%d" % i] = err(a, want)
    del l64, y64, g64
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        for _ in range(5):
            sides["fused"][1]()
    finally:
        ops.set_kernel_timer(None)
    r["fused_kernels_ms"] = {k: v["ms"] / v["calls"] for k, v in timer.summary().items()}
    return r


def cases(shape, c, steps):
    g = torch.Generator(device="cuda").manual_seed(17)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)          # noqa: E731
    for lvl in (2, 1, 0):
        grid = tuple(s // 2 ** lvl for s in shape)
        C, V = c * 2 ** lvl, grid[0] * grid[1] * grid[2]
        R = 3 * C // 8
        t = [rn(1, *grid, C) for _ in range(3)]
        lg, gy = rn(1, *grid, 3), rn(1, *grid, 3 * C)
        W1, W2 = rn(R, 3 * C) / (3 * C) ** 0.5, rn(3 * C, R) / R ** 0.5
        nin = 4.0 * V * (3 * C + 3)
        # forward: pool reads the inputs, apply reads them and writes out; backward: pass A reads inputs + d_out, pass B reads both
        # and writes the four gradients
        yield "nff,C%d,%dx%dx%d" % ((C,) + grid), measure(t + [lg, W1, W2], [], gy, lambda *a: ops.nff_fuse(*a), aten_nff,
                                                            2 * nin + 4.0 * V * 3 * C, 2 * (nin + 4.0 * V * 3 * C) + nin, steps)
        torch.cuda.empty_cache()
        n = 3 - lvl
        preds = [rn(1, *(s // 2 ** (n - i) for s in grid), 3) for i in range(n)]
        x, lgd, gyd = rn(1, *grid, 3 * n), rn(1, *grid, 3 * n), rn(1, *grid, 3)
        small = 4.0 * sum(p.numel() for p in preds)
        yield "dfi_upsample,n%d,%dx%dx%d" % ((n,) + grid), measure(preds, [], x, fused_dfi_up, aten_dfi_up, small + 4.0 * x.numel(),
                                                                     small + 4.0 * x.numel(), steps)
        yield "dfi_gate,n%d,%dx%dx%d" % ((n,) + grid), measure([x, lgd], [], gyd, ops.dfi_gate, aten_dfi_gate,
                                                                 4.0 * (2 * x.numel() + gyd.numel()), 4.0 * (4 * x.numel() + gyd.numel()), steps)
        torch.cuda.empty_cache()
    a, b = rn(1, *(s // 2 for s in shape), 2 * c), rn(1, *(s // 2 for s in shape), 2 * c)
    yield "residual_add,%d" % a.numel(), measure([a, b], [], a, ops.residual_add, lambda u, v: planar(u) + planar(v), 12.0 * a.numel(),
                                                  0.0, steps)


def make_pcnet(shape, channels):
    torch.manual_seed(24)
    return models.PCNet(shape, channels=channels).cuda()


def main():
    ap = bench_layer.parser("160,192,160", 16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pcnet.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_pcnet.json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "channels": args.channels, "iterations": args.steps, "ops": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for name, measured in cases(shape, args.channels, args.steps):
        res["ops"][name] = measured
        save()
    if args.train_steps > 0:
        res["train_step"] = {}
        for name, make in (("pcnet", lambda s: make_pcnet(s, args.channels)), ("modet", bench_layer.make_modet)):
            for capture in (False, True):
                key = "%s,%s" % (name, "captured" if capture else "eager")
                try:
                    res["train_step"][key] = bench_layer.train_step_ms(make(shape), shape, args.train_steps, capture)
                except RuntimeError as e:                 # an allocation failure is a result, not a crash of the tool
                    res["train_step"][key] = {"error": str(e)[:400]}
                torch.cuda.empty_cache()
                save()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
