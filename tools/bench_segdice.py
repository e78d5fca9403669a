"""The label-overlap (soft Dice) term (value + weighted gradient of a channels-last flow, what a train step asks of it) on its own,
beside the ATen fp32 composition a user writes today (one_hot -> trilinear grid_sample(align_corners=True) on the normalised grid
-> per-label sums -> 1 - mean Dice, forward + backward) on the same GPU in the same process: time (HIP events, the sides
alternating, median and spread) and peak allocated memory above the inputs.

    python tools/bench_segdice.py [--iters 20] [--shape 160,192,160] [--labels 54] [--batch 1] [--steps 30] [--json profiles/bench_segdice_<shape>.json]

--steps K > 0 also times the captured ModeT train step (hipGraph replay + Adam, synthetic pair, labels and weights of seed 24)
without and with the term, K steps in one window after warm-up; --steps 0 leaves that out.

Byte figures are the call's own, from the shapes: 44 B per voxel with a gradient; the achieved rate is that
count over the CALL's time (four kernels), not a kernel's share of peak."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import losses, ops  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402

HBM_PEAK_GBPS = 8000.0           # MI355X, HBM3E


def aten_dice(mov_lab, flow_cl, fix_lab, L):
    """the composition in fp32: (loss, d loss / d flow_cl)"""
    B, D, H, W, _ = flow_cl.shape
    f = flow_cl.detach().requires_grad_(True)
    dev = f.device
    gz, gy, gx = torch.meshgrid(torch.arange(D, device=dev, dtype=f.dtype), torch.arange(H, device=dev, dtype=f.dtype),
                                torch.arange(W, device=dev, dtype=f.dtype), indexing="ij")
    pz, py, px = gz + f[..., 0], gy + f[..., 1], gx + f[..., 2]
    grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1, 2 * pz / (D - 1) - 1], -1)       # grid_sample wants (x, y, z)
    hot = F.one_hot(mov_lab[:, 0].long(), L + 1)[..., 1:].permute(0, 4, 1, 2, 3).float()
    warped = F.grid_sample(hot, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    fixed = F.one_hot(fix_lab[:, 0].long(), L + 1)[..., 1:].permute(0, 4, 1, 2, 3).float()
    inter, p, t = (fixed * warped).sum((2, 3, 4)), warped.sum((2, 3, 4)), fixed.sum((2, 3, 4))
    loss = 1 - (2 * inter / (p + t + 1e-5)).mean()
    loss.backward()
    return loss.detach(), f.grad


def step_ms(shape, batch, seg, labels, steps, warmup=5):
    """ms per captured ModeT train step with NCC + Grad3d and the label term ``seg`` (None = without)"""
    from smilecode_amd import models, synth
    from smilecode_amd.engine import Trainer
    model = models.ModeT(shape, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1.0).cuda()
    models.load_numpy_weights(model, synth.make_weights(24))
    mov, fix = (torch.from_numpy(v).cuda() for v in synth.make_pair(shape, 24, batch))
    kw = {} if seg is None else {"labels": labels}
    tr = Trainer(model, seg=seg).capture(mov, fix, **kw)
    for _ in range(warmup):
        tr.train_step(mov, fix, epoch=0, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.train_step(mov, fix, epoch=0, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    r = {"ms_per_step": ms, "loss": float(out[0])}
    if seg is not None:
        r["seg"] = float(out[3])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--labels", type=int, default=54)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_segdice.py measures on a GPU; none is present")
    from smilecode_amd import synth
    shape = tuple(int(s) for s in args.shape.split(","))
    B, L = args.batch, args.labels
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                         "bench_segdice_%dx%dx%d.json" % shape)
    g = torch.Generator(device="cuda").manual_seed(3)
    flow = torch.randn((B,) + shape + (3,), device="cuda", generator=g)          # channels-last, a few voxels of displacement
    # the synthetic label maps hold 54 labels; a smaller L leaves the rest out of every sum, a larger one has empty labels
    mov_lab = torch.stack([torch.from_numpy(synth.make_labels(shape, 24 + i)) for i in range(B)])[:, None].cuda()
    fix_lab = torch.stack([torch.from_numpy(synth.make_labels(shape, 124 + i)) for i in range(B)])[:, None].cuda()
    if L < 54:
        mov_lab, fix_lab = (torch.where(t <= L, t, torch.zeros_like(t)) for t in (mov_lab, fix_lab))
    nvox = float(flow.numel() // 3)
    one_hot_bytes = int(L * nvox * 4)
    res = {"shape": list(shape), "batch": B, "labels": L, "device": torch.cuda.get_device_name(0), "flow_bytes": 4 * flow.numel(),
           "bytes_per_voxel": ops.SEGDICE_BYTES_PER_VOXEL, "one_hot_bytes": one_hot_bytes}

    def hip():
        return ops.seg_dice_value_and_grad_cl(flow, mov_lab, fix_lab, L)

    def sums():
        return ops.seg_dice_sums(mov_lab, flow, fix_lab, L, channels_last=True)

    def ref():
        return aten_dice(mov_lab, flow, fix_lab, L)

    for _ in range(3):
        hip()
        sums()
    for _ in range(2):
        ref()
    t_hip, t_ref, t_sums = [], [], []
    for _ in range(args.iters):                  # alternate the sides: whatever else the host does hits all of them
        t_hip.append(once(hip))
        t_ref.append(once(ref))
        t_sums.append(once(sums))
    r = {"hip": stats(t_hip), "aten": stats(t_ref), "hip_sums_only": stats(t_sums)}
    r["hip"]["peak_bytes"], r["aten"]["peak_bytes"] = peak_above(hip), peak_above(ref)
    r["hip"]["GBps_of_own_bytes"] = ops.SEGDICE_BYTES_PER_VOXEL * nvox / r["hip"]["ms"] / 1e6
    r["hip"]["fraction_of_hbm_peak"] = r["hip"]["GBps_of_own_bytes"] / HBM_PEAK_GBPS
    r["aten_over_hip_time"] = r["aten"]["ms"] / r["hip"]["ms"]
    r["aten_minus_hip_peak_bytes"] = r["aten"]["peak_bytes"] - r["hip"]["peak_bytes"]
    r["peak_saving_in_one_hot_volumes"] = r["aten_minus_hip_peak_bytes"] / one_hot_bytes
    l_hip, g_hip = hip()
    l_ref, g_ref = ref()
    r["grad_maxdiff_of_max"] = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
    r["loss_hip"], r["loss_aten"] = float(l_hip), float(l_ref)
    res.update(r)
    del g_hip, g_ref
    torch.cuda.empty_cache()
    if args.steps > 0:
        del flow
        torch.cuda.empty_cache()
        res["train_step"] = {"without": step_ms(shape, B, None, None, args.steps),
                             "with_dice": step_ms(shape, B, losses.LabelDice(L), (mov_lab, fix_lab), args.steps)}
        res["train_step"]["added_ms"] = res["train_step"]["with_dice"]["ms_per_step"] - res["train_step"]["without"]["ms_per_step"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
