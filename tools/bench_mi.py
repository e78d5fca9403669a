"""The two mutual-information terms (value + gradient for y_pred, what a train step asks of them) on their own, beside the ATen
fp32 composition (tests/mi_oracle.py in fp32, forward + backward) on the same GPU in the same process: time (HIP events, the
two sides alternating, median and spread) and peak allocated memory above the two input volumes.

    python tools/bench_mi.py [--iters 20] [--shape 160,192,160] [--batch 1] [--steps 0] [--json out.json]

--steps K > 0 also times the captured train step (hipGraph replay + Adam, synthetic pair and weights of seed 24) with the NCC
term and with each of the two, K steps in one window after warm-up, for information.

FLOP and byte figures are the implementation's own, as given to ops._Guard (ops.MI_FLOP_PER_PASS, ops.MI_BYTES_PER_PASS;
DESIGN.md section 4.5): achieved rates are those counts over the CALL's time (several kernels), not a kernel's share of peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import ops  # noqa: E402
from tests import mi_oracle  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def peak_above(fn):
    """peak allocated bytes during fn() above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def stats(ts):
    ts = sorted(ts)
    return {"ms": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "runs": len(ts)}


def step_ms(shape, batch, sim, steps, warmup=5):
    """ms per captured train step with the similarity term ``sim`` (None = NCC_vxm)"""
    import time
    from smilecode_amd import models, synth
    from smilecode_amd.engine import Trainer
    model = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(model, synth.make_weights(24))
    mov, fix = (torch.from_numpy(v).cuda() for v in synth.make_pair(shape, 24, batch))
    tr = Trainer(model, sim=sim).capture(mov, fix)
    for _ in range(warmup):
        tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.train_step(mov, fix, epoch=0)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return {"ms_per_step": ms, "loss": float(out[0]), "sim": float(out[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mi.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    B = args.batch
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.rand((B, 1) + shape, device="cuda", generator=g)
    b = torch.rand((B, 1) + shape, device="cuda", generator=g)
    nv = float(a.numel())
    res = {"shape": list(shape), "batch": B, "device": torch.cuda.get_device_name(0), "volume_bytes": 4 * a.numel(),
           "flop_per_voxel": 2 * ops.MI_FLOP_PER_PASS, "bytes_per_voxel": 2 * ops.MI_BYTES_PER_PASS + 4.0}

    def aten(fn):
        def step():
            bb = b.detach().requires_grad_(True)
            fn(a, bb).backward()
            return bb.grad
        return step

    for name, hip, ref in (("mi", lambda: ops.mi_value_and_grad(a, b), aten(mi_oracle.mi_loss)),
                           ("lmi", lambda: ops.lmi_value_and_grad(a, b), aten(mi_oracle.lmi_loss))):
        r = {}
        for _ in range(3):
            hip()
        for _ in range(2):
            ref()
        t_hip, t_ref = [], []
        for _ in range(args.iters):                  # alternate the two sides: whatever else the host does hits both
            t_hip.append(once(hip))
            t_ref.append(once(ref))
        r["hip"], r["aten"] = stats(t_hip), stats(t_ref)
        r["hip"]["peak_bytes"], r["aten"]["peak_bytes"] = peak_above(hip), peak_above(ref)
        r["hip"]["GFLOPs_of_own_flop"] = res["flop_per_voxel"] * nv / r["hip"]["ms"] / 1e6
        r["hip"]["GBps_of_own_bytes"] = res["bytes_per_voxel"] * nv / r["hip"]["ms"] / 1e6
        r["aten_over_hip_time"] = r["aten"]["ms"] / r["hip"]["ms"]
        r["aten_over_hip_peak_bytes"] = r["aten"]["peak_bytes"] / max(r["hip"]["peak_bytes"], 1)
        l_hip, g_hip = hip()
        g_ref = ref()
        r["grad_maxdiff_of_max"] = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
        r["loss_hip"] = float(l_hip)
        res[name] = r
    if args.steps > 0:
        from smilecode_amd import losses
        del a, b
        torch.cuda.empty_cache()
        res["train_step"] = {name: step_ms(shape, B, sim, args.steps) for name, sim in (
            ("ncc", None), ("mi", losses.MutualInformation()), ("lmi", losses.localMutualInformation()))}
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
