"""The surface-distance evaluation (ops.surface_distances, csrc/surface.hip) on its own: two Voronoi label maps of 54 seeded points
at 160x192x160 (the second map's seeds jittered by a few voxels), HD / HD95 / ASSD of every label in one call.  Time (HIP events:
median, minimum and maximum of --steps runs after warm-up) and peak allocated memory above the two maps, workspace included.

If scipy imports, the same 54 labels are also scored ONCE on the CPU the way the reference does it (medpy's algorithm: binary
erosion plus distance_transform_edt per label and direction on the full volume), timed, and compared with the GPU's numbers; if
it does not import, that leg is omitted and the output says so.

    python tools/bench_surface.py [--steps 30] [--shape 160,192,160] [--labels 54] [--cpu-labels 54] [--json profiles/bench_surface.json]

--cpu-labels K < --labels scores only the first K labels on the CPU (its time is then reported for K labels, not extrapolated)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import _lib, ops  # noqa: E402
from tools.bench_mi import once, peak_above, stats  # noqa: E402


def voronoi(shape, seeds):
    """(D,H,W) int16 on the GPU: 1 + index of the nearest seed, one z-slab at a time"""
    D, H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    out = torch.empty(shape, dtype=torch.int16, device="cuda")
    s = seeds.cuda()
    for z in range(D):
        d = (z - s[:, 0, None, None]) ** 2 + (yy[None] - s[:, 1, None, None]) ** 2 + (xx[None] - s[:, 2, None, None]) ** 2
        out[z] = (1 + d.argmin(0)).to(torch.int16)
    return out


def cpu_reference(a, b, labels):
    """medpy's hd / hd95 / assd restated over scipy.ndimage (medpy/metric/binary.py, __surface_distances) -> (nlabels, 3), seconds"""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    fp = generate_binary_structure(3, 1)

    def sds(res, ref):
        rb, fb = res ^ binary_erosion(res, structure=fp, iterations=1), ref ^ binary_erosion(ref, structure=fp, iterations=1)
        return distance_transform_edt(~fb)[rb]
    rows, t0 = [], time.perf_counter()
    for l in labels:
        ra, rb = a == l, b == l
        ab, ba = sds(ra, rb), sds(rb, ra)
        rows.append([max(ab.max(), ba.max()), np.percentile(np.hstack((ab, ba)), 95), (ab.mean() + ba.mean()) / 2.0])
    return np.array(rows), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shape", default="160,192,160")
    ap.add_argument("--labels", type=int, default=54)
    ap.add_argument("--cpu-labels", type=int, default=-1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_surface.py measures on a GPU; none is present")
    shape = tuple(int(s) for s in args.shape.split(","))
    nl = args.labels
    out_path = args.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_surface.json")
    g = torch.Generator().manual_seed(7)
    flat = torch.randperm(shape[0] * shape[1] * shape[2], generator=g)[:nl]
    seeds = torch.stack((flat // (shape[1] * shape[2]), (flat // shape[2]) % shape[1], flat % shape[2]), 1)
    moved = torch.minimum(torch.clamp(seeds + torch.randint(-3, 4, seeds.shape, generator=g), min=0), torch.tensor(shape) - 1)
    a, b = voronoi(shape, seeds), voronoi(shape, moved)
    run = lambda: ops.surface_distances(a, b, nl)      # noqa: E731
    for _ in range(3):
        run()
    ts = [once(run) for _ in range(args.steps)]
    metrics, counts = run()
    m, c = metrics.cpu().numpy(), counts.cpu().numpy()
    both = ~np.isnan(m[:, 0])
    res = {"device": torch.cuda.get_device_name(0), "shape": list(shape), "labels": nl, "labels_in_both_maps": int(both.sum()),
           "surface_distances": dict(stats(ts), peak_bytes=peak_above(run)),
           "workspace_bytes": int(_lib.load().modet_surface_ws_bytes(*shape, nl)), "map_bytes": 2 * a.numel(),
           "border_voxels": int(c[:, 2:4].sum()),
           "mean_hd": float(m[both, 0].mean()), "mean_hd95": float(m[both, 1].mean()), "mean_assd": float(m[both, 2].mean())}
    try:
        import scipy
    except ImportError:
        scipy = None
        res["cpu_scipy"] = "omitted: scipy does not import on this host"
    if scipy is not None:
        k = nl if args.cpu_labels < 0 else min(args.cpu_labels, nl)
        labels = [l for l in range(1, k + 1) if both[l - 1]]
        ref, sec = cpu_reference(a.cpu().numpy(), b.cpu().numpy(), labels)
        got = m[[l - 1 for l in labels], :3]
        res["cpu_scipy"] = {"scipy": scipy.__version__, "labels_scored": len(labels), "seconds": sec, "runs": 1,
                            "includes": "per label: 2 masks, 4 erosions, 2 distance_transform_edt, percentile; maps already on the host",
                            "cpu_over_gpu_time": sec * 1e3 / res["surface_distances"]["ms"] if len(labels) == int(both.sum()) else None,
                            "max_rel_diff_gpu_vs_scipy": float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
