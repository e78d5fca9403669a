"""The scaling-and-squaring integration (ops.vecint, csrc/vecint.hip) on its own, beside two baselines on the same GPU in the same
process, the sides alternating: (a) the composition of existing launches -- the scale, then ops.warp(v, v, add_flow=True,
flow_bound=...) nsteps times -- and (b) the ATen composition (normalised grid -> grid_sample, what the reference's VecInt runs).
Forward (no gradient wanted) and forward + backward of one integration, at 160x192x160 and 80x96x80, for bound = 1 (a field in
[-1, 1]: every backward step gathered) and bound = 0 (a field of a few voxels: every backward step scattered): time (HIP events,
median, minimum and maximum) and peak allocated memory above the field itself.  The fused and the composed side are each
timed TWICE per round (a round is aten, fused, composed, fused_again, composed_again): the ratio of the two medians of one side
is the spread of repeated runs of the same code, against which "not slower" is judged.

    python tools/bench_vecint.py [--steps 30] [--nsteps 7] [--shapes 160,192,160:80,96,80] [--train-steps 0] [--json profiles/bench_vecint.json]

--steps K: timed iterations per side after warm-up.  --train-steps K > 0 also times the captured train step (hipGraph replay +
Adam, synthetic pair and weights of seed 24) with diff=False and diff=True at the first shape, for information."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import ops  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402


def fused(w, nsteps, bound):
    return ops.vecint(w, nsteps, bound)


def composed(w, nsteps, bound):
    v = w * (1.0 / 2 ** nsteps)
    for k in range(nsteps):
        v = ops.warp(v, v, 0, True, 1 if (bound > 0 and bound * 2.0 ** (k - nsteps) <= 1.0) else 0)
    return v


class Aten:
    """the reference's VecInt on a planar field: identity grid buffer, normalisation, grid_sample(align_corners=True)"""

    def __init__(self, shape):
        vec = [torch.arange(0, s, device="cuda", dtype=torch.float32) for s in shape]
        self.grid = torch.stack(torch.meshgrid(vec, indexing="ij")).unsqueeze(0)
        self.shape = shape

    def warp(self, src, flow):
        loc = self.grid + flow
        loc = torch.stack([2 * (loc[:, i] / (self.shape[i] - 1) - 0.5) for i in range(3)], 1)
        return F.grid_sample(src, loc.permute(0, 2, 3, 4, 1)[..., [2, 1, 0]], align_corners=True, mode="bilinear")

    def __call__(self, w_planar, nsteps):
        v = w_planar * (1.0 / 2 ** nsteps)
        for _ in range(nsteps):
            v = v + self.warp(v, v)
        return v


def train_step_ms(shape, diff, steps, warmup=5):
    from smilecode_amd import models, synth
    from smilecode_amd.engine import Trainer
    model = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0, diff=diff).cuda()
    models.load_numpy_weights(model, synth.make_weights(24))
    mov, fix = (torch.from_numpy(v).cuda() for v in synth.make_pair(shape, 24, 1))
    tr = Trainer(model).capture(mov, fix)
    for _ in range(warmup):
        tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    return {"ms_per_step": (time.perf_counter() - t0) * 1e3 / steps, "loss": float(out[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--nsteps", type=int, default=7)
    ap.add_argument("--shapes", default="160,192,160:80,96,80")
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vecint.py measures on a GPU; none is present")
    shapes = [tuple(int(s) for s in sh.split(",")) for sh in args.shapes.split(":")]
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_vecint.json")
    n = args.nsteps
    res = {"device": torch.cuda.get_device_name(0), "nsteps": n, "iterations": args.steps, "cases": {}}
    for shape in shapes:
        aten = Aten(shape)
        for bound, amp in ((1.0, 1.0), (0.0, 4.0)):
            g = torch.Generator(device="cuda").manual_seed(3)
            w = torch.tanh(torch.randn((1,) + shape + (3,), device="cuda", generator=g)) * amp
            cot = torch.randn(w.shape, device="cuda", generator=g)
            w_pl, cot_pl = w.permute(0, 4, 1, 2, 3).contiguous(), cot.permute(0, 4, 1, 2, 3).contiguous()

            def fwd(fn, x, *a):
                with torch.no_grad():
                    return fn(x, *a)

            def fwd_bwd(fn, x, c, *a):
                x = x.detach().requires_grad_(True)
                (gr,) = torch.autograd.grad(fn(x, *a), [x], c)
                return gr

            f_side = (lambda: fwd(fused, w, n, bound), lambda: fwd_bwd(fused, w, cot, n, bound))
            c_side = (lambda: fwd(composed, w, n, bound), lambda: fwd_bwd(composed, w, cot, n, bound))
            # the order of a round: "fused" follows the ATen side (200 MB to 1 GB of other traffic), every later side a HIP one
            sides = {"aten": (lambda: fwd(aten, w_pl, n), lambda: fwd_bwd(aten, w_pl, cot_pl, n)),
                     "fused": f_side, "composed": c_side, "fused_again": f_side, "composed_again": c_side}
            r = {}
            for leg, idx in (("fwd", 0), ("fwd_bwd", 1)):
                for _ in range(3):
                    for s in sides.values():
                        s[idx]()
                ts = {k: [] for k in sides}
                for _ in range(args.steps):              # alternate the sides: whatever else the host does hits all of them
                    for k, s in sides.items():
                        ts[k].append(once(s[idx]))
                r[leg] = {k: stats(v) for k, v in ts.items()}
                for k in ("fused", "composed", "aten"):
                    r[leg][k]["peak_bytes"] = peak_above(sides[k][idx])
                r[leg]["composed_over_fused_time"] = r[leg]["composed"]["ms"] / r[leg]["fused"]["ms"]
                r[leg]["aten_over_fused_time"] = r[leg]["aten"]["ms"] / r[leg]["fused"]["ms"]
                r[leg]["fused_again_over_fused_time"] = r[leg]["fused_again"]["ms"] / r[leg]["fused"]["ms"]
                r[leg]["composed_again_over_composed_time"] = r[leg]["composed_again"]["ms"] / r[leg]["composed"]["ms"]
                r[leg]["composed_again_over_fused_again_time"] = r[leg]["composed_again"]["ms"] / r[leg]["fused_again"]["ms"]
            gf, gc, ga = sides["fused"][1](), sides["composed"][1](), sides["aten"][1]()
            ga = ga.permute(0, 2, 3, 4, 1)
            r["grad_fused_vs_composed_maxdiff_of_max"] = float((gf - gc).abs().max() / gc.abs().max())
            # a random field is rough: where fp32 rounding puts a sample coordinate on the other side of an integer (a kink of
            # trilinear sampling; ATen normalises and un-normalises its coordinates) single voxels differ by a second difference
            # of the field, so the ATen side is compared in the mean and by the share of elements that differ visibly
            r["grad_fused_vs_aten_meandiff_of_mean"] = float((gf - ga).abs().mean() / ga.abs().mean())
            r["grad_fused_vs_aten_share_beyond_1e-3_of_max"] = float(((gf - ga).abs() > 1e-3 * ga.abs().max()).float().mean())
            r["field_bytes"] = 4 * w.numel()
            res["cases"]["%dx%dx%d,bound=%g" % (shape + (bound,))] = r
            del gf, gc, ga, w, cot, w_pl, cot_pl
            torch.cuda.empty_cache()
        del aten
    if args.train_steps > 0:
        torch.cuda.empty_cache()
        res["train_step"] = {"shape": list(shapes[0]), "diff=False": train_step_ms(shapes[0], False, args.train_steps),
                             "diff=True": train_step_ms(shapes[0], True, args.train_steps)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
