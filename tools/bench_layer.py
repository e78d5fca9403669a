"""What tools/bench_rdn.py and tools/bench_rcn.py share: one fused stride-2 layer beside ATen's on the same GPU in the same process,
the sides alternating, and the tool around it (arguments, the JSON under profiles/, the train steps beside ModeT's).

``layer_case``: forward (no gradient wanted) and forward + backward, time (HIP events: median, minimum, maximum) and peak allocated
memory above the inputs.  The fused side is timed twice per round (aten, fused, fused_again): the ratio of its two medians is the
spread of repeated runs of the same code.  The layer's ALGORITHMIC bytes: forward 4 (|x| + |y|); the backward reads x and d_y (and y
once more under an activation) for the weight gradient, d_y (and y) for the data gradient and writes d_x; ``achieved_gbps`` divides
them by the fused side's median time.  ``error_vs_fp64``: both sides against the same layer in ATen fp64 on the GPU, max|got - ref|
/ max|ref| per result."""
import argparse
import json
import os
import sys
import time

import torch

from smilecode_amd import models, ops, synth
from smilecode_amd.engine import Trainer
from tools.bench_mi import once, peak_above, stats


def layer_case(x, w, b, gy, fused, ref, flop_fwd, steps, act=True, x_grad=True, w_aten=None):
    """x (B,D,H,W,Cin) and the cotangent gy (B,Do,Ho,Wo,Cout) channels-last; w and b (None: no bias) leaves.  ``fused(a, w, b)``: the
    package's layer on channels-last a; ``ref(a, w, b)``: the same layer, its activation included (``act``: whether it has one), in
    ATen on a (B,C,D,H,W) view -- the ATen side on the same bytes in channels_last_3d memory format (with ``w_aten``, a leaf of its
    own in the layout ATen's channels-last path takes, for w) and, in fp64, the reference of both.  ``x_grad``: whether either side
    computes a data gradient."""
    n_kink = 0
    if act:
        # LeakyReLU has a kink at 0: where |y| is within rounding of it, fp32 and fp64 can take different branches of the derivative
        # and one such element moves a gradient by (1 - slope) d_y times its factor.  The cotangent is zeroed there (|y| < 1e-5 in
        # fp64: a few of the millions of outputs), so that error_vs_fp64 below measures arithmetic, not the branch.
        with torch.no_grad():
            y_ref = ref(x.permute(0, 4, 1, 2, 3).double(), w.detach().double(), None if b is None else b.detach().double())
            near_kink = y_ref.permute(0, 2, 3, 4, 1).abs() < 1e-5
            gy = (gy * ~near_kink).contiguous()
            n_kink = int(near_kink.sum())
            del y_ref, near_kink
    x_nc, gy_nc = x.permute(0, 4, 1, 2, 3), gy.permute(0, 4, 1, 2, 3)          # channels_last_3d views of the same bytes
    w_aten = w if w_aten is None else w_aten
    bias = [] if b is None else [b]

    def fwd(fn, a, wt):
        with torch.no_grad():
            return fn(a, wt, b)

    def fwd_bwd(fn, a, wt, c):
        a = a.detach().requires_grad_(x_grad)
        return torch.autograd.grad(fn(a, wt, b), ([a] if x_grad else []) + [wt] + bias, c)

    sides = {"aten": (lambda: fwd(ref, x_nc, w_aten), lambda: fwd_bwd(ref, x_nc, w_aten, gy_nc)),
             "fused": (lambda: fwd(fused, x, w), lambda: fwd_bwd(fused, x, w, gy))}
    sides["fused_again"] = sides["fused"]
    nx, ny = x.numel(), gy.numel()
    ya = 2 if act else 1
    algo = {"fwd": 4.0 * (nx + ny), "fwd_bwd": 4.0 * (nx + ny) + 4.0 * (nx + ya * ny) + (4.0 * (nx + ya * ny) if x_grad else 0.0)}
    r = {"B": x.shape[0], "grid": list(x.shape[1:4]), "Cin": x.shape[4], "Cout": gy.shape[4], "bias": b is not None, "act": act,
         "x_grad": x_grad, "input_bytes": 4 * nx, "output_bytes": 4 * ny, "flop_fwd": flop_fwd,
         "outputs_near_kink_with_zero_cotangent": n_kink}
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
    names = (["d_x"] if x_grad else []) + ["d_w"] + (["d_b"] if bias else [])
    # (ATen's and the fp64 d_x are (B,C,D,H,W) views: against the fused side's channels-last one by name, a 3x3x3 grid of 3 channels
    # has the same shape in both)
    cl = lambda n, a: a.permute(0, 2, 3, 4, 1) if n == "d_x" else a      # noqa: E731
    r["grad_fused_vs_aten_maxdiff_of_max"] = max(float((f - cl(n, a)).abs().max() / a.abs().max()) for n, f, a in zip(names, gf, ga))
    x64 = x_nc.double().requires_grad_(x_grad)
    p64 = [t.detach().double().requires_grad_(True) for t in [w] + bias]
    y64 = ref(x64, p64[0], p64[1] if bias else None)
    g64 = torch.autograd.grad(y64, ([x64] if x_grad else []) + p64, gy_nc.double())
    err = lambda got, want: float((got.double() - want).abs().max() / want.abs().max())      # noqa: E731
    r["error_vs_fp64"] = {"fused": {"y": err(fwd(fused, x, w), y64.detach().permute(0, 2, 3, 4, 1))},
                          "aten": {"y": err(fwd(ref, x_nc, w_aten), y64.detach())}}
    for n, f, a, want in zip(names, gf, ga, g64):
        r["error_vs_fp64"]["fused"][n] = err(f, cl(n, want))
        r["error_vs_fp64"]["aten"][n] = err(a, want)
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


def make_modet(shape):
    m = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


def parser(shape, channels):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shape", default=shape)
    ap.add_argument("--channels", type=int, default=channels)
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--json", default="")
    return ap


def run(tool, args, layers, nets, **head):
    """the tool ``tool`` (its name without .py: the JSON goes to profiles/<tool>.json unless --json names another place).
    ``layers(shape, channels, steps)`` yields (name, grid, Cin, Cout, that layer's layer_case), measuring one layer per step of the
    iteration; ``nets`` lists (name, make(shape)) of the networks whose train step is timed, eager and captured, before ModeT's;
    ``head``: further fields of the result."""
    if not torch.cuda.is_available():
        sys.exit("%s.py measures on a GPU; none is present" % tool)
    shape = tuple(int(s) for s in args.shape.split(","))
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", tool + ".json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "channels": args.channels, "iterations": args.steps, **head,
           "layers": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for name, grid, cin, cout, measured in layers(shape, args.channels, args.steps):
        res["layers"]["%s,%dx%dx%d,%d->%d" % ((name,) + grid + (cin, cout))] = measured
        torch.cuda.empty_cache()
        save()
    if args.train_steps > 0:
        res["train_step"] = {}
        for name, make in list(nets) + [("modet", make_modet)]:
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
