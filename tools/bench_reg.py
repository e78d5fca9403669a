"""The flow regularisers beside Grad3d (value + weighted gradient of a channels-last flow, what a train step asks of them) on their
own, each beside the ATen fp32 composition (tests/reg_oracle.py in fp32 on a planar copy, forward + backward) on the same GPU in
the same process: time (HIP events, the sides alternating, median and spread) and peak allocated memory above the flow itself.
ops.grad3d_value_and_grad_cl is timed the same way, for information.

    python tools/bench_reg.py [--iters 20] [--shape 160,192,160] [--batch 1] [--steps 30] [--json profiles/bench_reg_<shape>.json]

--steps K > 0 also times the captured train step (hipGraph replay + Adam, synthetic pair and weights of seed 24) with the default
Grad3d and with each kind, K steps in one window after warm-up, for information; --steps 0 leaves that out.

Byte figures are the call's own: the flow read once and the gradient written once, 8 B per element = 24 B per voxel (DESIGN.md
section 4.7); the achieved rate is that count over the CALL's time (two kernels), not a kernel's share of peak."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import losses, ops  # noqa: E402
from tests import reg_oracle  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402

HBM_PEAK_GBPS = 8000.0           # MI355X, HBM3E
KINDS = ("itv", "gradient-l2", "gradient-l1", "bending")


def term(kind):
    return losses.Grad3DiTV() if kind == "itv" else losses.DisplacementRegularizer(kind)


def step_ms(shape, batch, reg, steps, warmup=5):
    """ms per captured train step with NCC and the regulariser ``reg`` (None = Grad3d('l2'))"""
    from smilecode_amd import models, synth
    from smilecode_amd.engine import Trainer
    model = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(model, synth.make_weights(24))
    mov, fix = (torch.from_numpy(v).cuda() for v in synth.make_pair(shape, 24, batch))
    tr = Trainer(model, reg=reg).capture(mov, fix)
    for _ in range(warmup):
        tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return {"ms_per_step": ms, "loss": float(out[0]), "reg": float(out[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_reg.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    B = args.batch
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         "bench_reg_%dx%dx%d.json" % shape)
    g = torch.Generator(device="cuda").manual_seed(3)
    flow = torch.randn((B,) + shape + (3,), device="cuda", generator=g)          # channels-last, a few voxels of displacement
    nvox = float(flow.numel() // 3)
    res = {"shape": list(shape), "batch": B, "device": torch.cuda.get_device_name(0), "flow_bytes": 4 * flow.numel(),
           "bytes_per_voxel": 24.0, "kinds": {}}

    def grad3d():
        return ops.grad3d_value_and_grad_cl(flow, "l2")

    for kind in KINDS:
        fn = reg_oracle.KINDS[kind]

        def hip():
            return ops.reg_value_and_grad_cl(flow, kind)

        def ref():
            # what a user does today: the planar view of the flow the step holds, the ATen expression, autograd, the gradient back
            f = flow.detach().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
            fn(f).backward()
            return f.grad.permute(0, 2, 3, 4, 1).contiguous()

        for _ in range(3):
            hip()
            grad3d()
        for _ in range(2):
            ref()
        t_hip, t_ref, t_g3 = [], [], []
        for _ in range(args.iters):                  # alternate the sides: whatever else the host does hits all of them
            t_hip.append(once(hip))
            t_ref.append(once(ref))
            t_g3.append(once(grad3d))
        r = {"hip": stats(t_hip), "aten": stats(t_ref), "grad3d_value_and_grad_cl": stats(t_g3)}
        r["hip"]["peak_bytes"], r["aten"]["peak_bytes"] = peak_above(hip), peak_above(ref)
        r["hip"]["GBps_of_own_bytes"] = 24.0 * nvox / r["hip"]["ms"] / 1e6
        r["hip"]["fraction_of_hbm_peak"] = r["hip"]["GBps_of_own_bytes"] / HBM_PEAK_GBPS
        r["aten_over_hip_time"] = r["aten"]["ms"] / r["hip"]["ms"]
        r["hip_over_grad3d_time"] = r["hip"]["ms"] / r["grad3d_value_and_grad_cl"]["ms"]
        r["aten_over_hip_peak_bytes"] = r["aten"]["peak_bytes"] / max(r["hip"]["peak_bytes"], 1)
        l_hip, g_hip = hip()
        g_ref = ref()
        r["grad_maxdiff_of_max"] = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
        r["loss_hip"] = float(l_hip)
        res["kinds"][kind] = r
        del g_hip, g_ref
        torch.cuda.empty_cache()
    if args.steps > 0:
        del flow
        torch.cuda.empty_cache()
        res["train_step"] = {"grad3d": step_ms(shape, B, None, args.steps)}
        for kind in KINDS:
            res["train_step"][kind] = step_ms(shape, B, term(kind), args.steps)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
