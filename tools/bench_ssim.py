"""The SSIM3D term (value + gradient for img2, what a train step asks of it) on its own, beside the ATen fp32 composition
(tests/ssim_oracle.py in fp32: five dense conv3d, forward + backward) on the same GPU in the same process: time (HIP events, the
two sides alternating, median and spread) and peak allocated memory above the two input volumes.  ops.ncc_value_and_grad is
timed the same way, for information.

    python tools/bench_ssim.py [--iters 20] [--shape 160,192,160] [--batch 1] [--window 11] [--steps 0] [--json out.json]

--steps K > 0 also times the captured train step (hipGraph replay + Adam, synthetic pair and weights of seed 24) with the NCC
term and with SSIM3D, K steps in one window after warm-up, for information.

FLOP and byte figures are the implementation's own, as given to ops._Guard (ops._ssim_counts): achieved
rates are those counts over the CALL's time (three kernels), not a kernel's share of peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import ops  # noqa: E402
from tests import ssim_oracle  # noqa: E402
from tools.bench_mi import once, peak_above, stats, step_ms  # noqa: E402

HBM_PEAK_GBPS = 8000.0           # MI355X, HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ssim.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    B, w = args.batch, args.window
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.rand((B, 1) + shape, device="cuda", generator=g)
    b = torch.rand((B, 1) + shape, device="cuda", generator=g)
    nv = float(a.numel())
    flop, nbytes = ops._ssim_counts(w, False, True)
    res = {"shape": list(shape), "batch": B, "window": w, "device": torch.cuda.get_device_name(0), "volume_bytes": 4 * a.numel(),
           "flop_per_voxel": flop, "bytes_per_voxel": nbytes}

    def hip():
        return ops.ssim_value_and_grad(a, b, w)

    def ref():
        bb = b.detach().requires_grad_(True)
        ssim_oracle.ssim_loss(a, bb, w).backward()
        return bb.grad

    def ncc():
        return ops.ncc_value_and_grad(a, b)

    for _ in range(3):
        hip()
        ncc()
    for _ in range(2):
        ref()
    t_hip, t_ref, t_ncc = [], [], []
    for _ in range(args.iters):                      # alternate the sides: whatever else the host does hits all of them
        t_hip.append(once(hip))
        t_ref.append(once(ref))
        t_ncc.append(once(ncc))
    r = {"hip": stats(t_hip), "aten": stats(t_ref), "ncc_value_and_grad": stats(t_ncc)}
    r["hip"]["peak_bytes"], r["aten"]["peak_bytes"] = peak_above(hip), peak_above(ref)
    r["hip"]["GFLOPs_of_own_flop"] = flop * nv / r["hip"]["ms"] / 1e6
    r["hip"]["GBps_of_own_bytes"] = nbytes * nv / r["hip"]["ms"] / 1e6
    r["hip"]["fraction_of_hbm_peak"] = r["hip"]["GBps_of_own_bytes"] / HBM_PEAK_GBPS
    r["aten_over_hip_time"] = r["aten"]["ms"] / r["hip"]["ms"]
    r["hip_over_ncc_time"] = r["hip"]["ms"] / r["ncc_value_and_grad"]["ms"]
    r["aten_over_hip_peak_bytes"] = r["aten"]["peak_bytes"] / max(r["hip"]["peak_bytes"], 1)
    l_hip, g_hip = hip()
    g_ref = ref()
    r["grad_maxdiff_of_max"] = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
    r["loss_hip"] = float(l_hip)
    res["ssim"] = r
    if args.steps > 0:
        from smilecode_amd import losses
        del a, b, g_hip, g_ref
        torch.cuda.empty_cache()
        res["train_step"] = {name: step_ms(shape, B, sim, args.steps) for name, sim in (("ncc", None), ("ssim", losses.SSIM3D(w)))}
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
