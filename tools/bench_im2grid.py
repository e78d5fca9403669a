"""The fused positional-encoding projection (ops.posenc_pair, csrc/posenc.hip) beside the ATen composition the reference's
PositionalEncodingLayer runs, on the same GPU in the same process, the sides alternating -- per level shape of a 160x192x160
volume (the level's fixed and warped moving features: two uses of the layer), forward (no gradient wanted) and forward +
backward: time (HIP events: median, minimum, maximum) and peak allocated memory above the inputs.  The fused side is timed
twice per round (aten, fused, fused_again): the ratio of its two medians is the spread of repeated runs of the same code.
Then the Im2Grid train step, eager and captured, beside ModeT's.

    python tools/bench_im2grid.py [--steps 30] [--shape 160,192,160] [--train-steps 30] [--json profiles/bench_im2grid.json]

The kernel's ALGORITHMIC bytes of a pair: forward 2 N (Cin + 6) 4; backward 2 N (6 + Cin) 4 for the data gradients plus
2 N (Cin + 6) 4 for the parameter gradients (x and d_y read again); ``achieved_gbps`` divides them by the median time."""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops, synth  # noqa: E402
from smilecode_amd.engine import Trainer  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402


def aten_layer(x, Wt, b, alpha):
    """what the reference's layer does to a channels-last input, in ATen: Linear, then per call three position ranges, their
    cos / sin pairs, a zero-filled (D,H,W,6) embedding filled by three slice assignments, repeated over the batch, scaled, added"""
    feat = F.linear(x, Wt, b)
    B, D, H, W, C = feat.shape
    emb = torch.zeros((D, H, W, 6), device=x.device, dtype=feat.dtype)
    for a, n in enumerate((D, H, W)):
        t = (torch.arange(n, device=x.device).float() * (math.pi / (n - 1))).unsqueeze(-1)
        pair = torch.cat((t.cos(), t.sin()), dim=-1)
        shape = [1, 1, 1, 2]
        shape[a] = n
        emb[:, :, :, 2 * a:2 * a + 2] = pair.reshape(shape)
    emb = emb[None, :, :, :, :C].repeat(B, 1, 1, 1, 1)
    return feat + alpha * emb


def layer_case(B, grid, Cin, steps):
    D, H, W = grid
    g = torch.Generator(device="cuda").manual_seed(5 + Cin)
    x1, x2 = (torch.randn((B, D, H, W, Cin), device="cuda", generator=g) for _ in range(2))
    c1, c2 = (torch.randn((B, D, H, W, 6), device="cuda", generator=g) for _ in range(2))
    Wt = (torch.randn((6, Cin), device="cuda", generator=g) / Cin ** 0.5).requires_grad_(True)
    b = torch.randn(6, device="cuda", generator=g).requires_grad_(True)
    alpha = torch.tensor([0.8], device="cuda", requires_grad=True)
    tab = ops.posenc_table(D, H, W, device="cuda")

    def fused(a, c):
        return ops.posenc_pair(a, c, Wt, b, alpha, tab)

    def aten(a, c):
        return aten_layer(a, Wt, b, alpha), aten_layer(c, Wt, b, alpha)

    def fwd(fn):
        with torch.no_grad():
            return fn(x1, x2)

    def fwd_bwd(fn):
        a, c = x1.detach().requires_grad_(True), x2.detach().requires_grad_(True)
        return torch.autograd.grad(list(fn(a, c)), [a, c, Wt, b, alpha], [c1, c2])

    sides = {"aten": (lambda: fwd(aten), lambda: fwd_bwd(aten)), "fused": (lambda: fwd(fused), lambda: fwd_bwd(fused))}
    sides["fused_again"] = sides["fused"]
    N = B * D * H * W
    algo = {"fwd": 2.0 * N * (Cin + 6) * 4, "fwd_bwd": 3 * 2.0 * N * (Cin + 6) * 4}
    r = {"voxels": N, "Cin": Cin, "input_bytes": 2 * 4 * N * Cin}
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
    r["grad_fused_vs_aten_maxdiff_of_max"] = max(float((f - a).abs().max() / a.abs().max()) for f, a in zip(gf, ga))
    return r


def train_step_ms(model, shape, steps, capture, warmup=5):
    mov, fix = (torch.from_numpy(v).cuda() for v in synth.make_pair(shape, 24, 1))
    tr = Trainer(model)
    if capture:
        tr.capture(mov, fix)
    for _ in range(warmup):
        tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    return {"ms_per_step": (time.perf_counter() - t0) * 1e3 / steps, "loss": float(out[0])}


def make_im2grid(shape):
    """seeded NON-zero projections (the reference's initial zero weights make every q equal every k: nothing to match)"""
    torch.manual_seed(24)                    # (the encoder's default initialisation draws from the global generator)
    m = models.Im2grid(shape).cuda()
    g = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for i in range(1, 6):
            pe = getattr(m, "peblock%d" % i)
            pe.proj.weight.copy_(torch.randn(pe.proj.weight.shape, generator=g) / pe.proj.weight.shape[1] ** 0.5)
            pe.proj.bias.copy_(torch.randn(6, generator=g) * 0.1)
    return m


def make_modet(shape):
    m = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(m, synth.make_weights(24))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_im2grid.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_im2grid.json")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "iterations": args.steps, "levels": {}}
    for lvl in range(1, 6):
        grid = tuple(s // 2 ** (lvl - 1) for s in shape)
        res["levels"]["level%d,%dx%dx%d,Cin=%d" % ((lvl,) + grid + (4 * 2 ** lvl,))] = layer_case(1, grid, 4 * 2 ** lvl, args.steps)
        torch.cuda.empty_cache()
    if args.train_steps > 0:
        res["train_step"] = {}
        for name, make in (("im2grid", make_im2grid), ("modet", make_modet)):
            for capture in (False, True):
                res["train_step"]["%s,%s" % (name, "captured" if capture else "eager")] = train_step_ms(make(shape), shape, args.train_steps, capture)
                torch.cuda.empty_cache()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
