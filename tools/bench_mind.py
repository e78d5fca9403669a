"""MIND loss forward + gradient for one argument on its own (HIP events around the calls), beside the ATen fp32 composition
(tests/mind_oracle.py mind_loss_aten: two replication pads, two dilated one-hot conv3d, avg_pool3d, min, mean, a clamp whose
bounds are read back to the host, exp) on the same GPU in the same process.

    python tools/bench_mind.py [--iters 20] [--shape 160,192,160] [--batch 1] [--json out.json]

If ATen cannot run the shape (memory, or a convolution the library refuses), the largest of the fallback shapes where it does is
timed instead and named in the output.  Achieved bytes per second are against the implementation's OWN traffic,
ops.MIND_BYTES_PER_VOXEL."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import ops  # noqa: E402
from tests import mind_oracle  # noqa: E402

FALLBACK = [(128, 160, 128), (96, 112, 96), (64, 64, 64)]


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def pair(B, shape):
    g = torch.Generator(device="cuda").manual_seed(3)
    return (torch.rand((B, 1) + shape, device="cuda", generator=g), torch.rand((B, 1) + shape, device="cuda", generator=g))


def aten_step(a, b):
    b = b.detach().requires_grad_(True)
    mind_oracle.mind_loss_aten(a, b).backward()
    return b.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    want = tuple(int(s) for s in args.shape.split(","))
    B = args.batch
    res = {"batch": B, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    a, b = pair(B, want)
    ms = timed(lambda: ops.mind_value_and_grad(a, b), args.iters)
    res["hip"] = {"shape": list(want), "ms": ms, "bytes_per_voxel": ops.MIND_BYTES_PER_VOXEL,
                  "GBps_of_own_bytes": ops.MIND_BYTES_PER_VOXEL * a.numel() / ms / 1e6}
    ms_fwd = timed(lambda: ops._mind_once(a, b, False, 1.0), args.iters)
    ms_desc = timed(lambda: ops.mind_ssc(a), args.iters)
    res["hip"].update(ms_value_only=ms_fwd, ms_descriptor=ms_desc)
    for shape in [want] + [s for s in FALLBACK if s != want]:
        a, b = pair(B, shape)
        try:
            t_aten = timed(lambda: aten_step(a, b), max(3, args.iters // 4), warm=2)
        except RuntimeError as e:
            res.setdefault("aten_failed", []).append({"shape": list(shape), "error": str(e).splitlines()[0][:200]})
            torch.cuda.empty_cache()
            continue
        t_hip = ms if shape == want else timed(lambda: ops.mind_value_and_grad(a, b), args.iters)
        res["aten"] = {"shape": list(shape), "ms": t_aten}
        res["compare"] = {"shape": list(shape), "hip_ms": t_hip, "aten_ms": t_aten, "aten_over_hip": t_aten / t_hip}
        g_hip = ops.mind_value_and_grad(a, b)[1]
        g_aten = aten_step(a, b)
        res["compare"]["grad_maxdiff_of_max"] = float((g_hip - g_aten).abs().max() / g_aten.abs().max())
        break
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
