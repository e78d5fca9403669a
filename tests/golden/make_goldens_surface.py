"""Writes tests/golden/op_surface.npz and REPORT_surface.txt: a few small label-map pairs with the surface distances the
reference's hd_val / hd95_val / assd_val (Baseline methods/RDN/utils.py:94-116) get for them.

Those functions call medpy's metric.hd, metric.hd95 and metric.assd.  medpy is NOT installed where these goldens were made, so
its algorithm (medpy/metric/binary.py, __surface_distances: border = mask ^ binary_erosion(mask, generate_binary_structure(3, 1)),
distances = distance_transform_edt(~other_border)[border]) is restated below over scipy.ndimage, the library medpy itself
calls.  Run from the repository root:  python tests/golden/make_goldens_surface.py"""
import os
import sys

import numpy as np
import scipy
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import surface_oracle as so  # noqa: E402  (the label maps only)


def surface_distances(result, reference):
    footprint = generate_binary_structure(result.ndim, 1)
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=None)
    return dt[result_border]


def per_label(a, b, label, percentile):
    ra, rb = a == label, b == label
    counts = [int(ra.sum()), int(rb.sum()), 0, 0, -1, -1, -1]
    fp = generate_binary_structure(3, 1)
    counts[2] = int((ra ^ binary_erosion(ra, structure=fp)).sum())
    counts[3] = int((rb ^ binary_erosion(rb, structure=fp)).sum())
    if counts[0] == 0 or counts[1] == 0:               # medpy raises here; the ABI reports NaN and which side is empty
        return [np.nan] * 5, counts
    ab, ba = surface_distances(ra, rb), surface_distances(rb, ra)
    both = np.hstack((ab, ba))
    sq = np.sort(np.rint(both * both).astype(np.int64))
    n = len(sq)
    vi = (n - 1) * (percentile / 100.0)
    k = min(int(np.floor(vi)), n - 1)
    counts[4:] = [int(sq[-1]), int(sq[k]), int(sq[min(k + 1, n - 1)])]
    hd = max(ab.max(), ba.max())                                           # metric.hd
    hdq = np.percentile(both, percentile)                                  # metric.hd95 (percentile = 95)
    asd_ab, asd_ba = ab.mean(), ba.mean()                                  # metric.asd
    return [hd, hdq, np.mean((asd_ab, asd_ba)), asd_ab, asd_ba], counts    # metric.assd


def main():
    cases = {}
    for tag in ("5x6x7", "4x5x67", "9x13x35"):
        shape, nl, seed = so.VORONOI[tag]
        a, b = so.voronoi_pair(shape, nl, seed)
        cases["voronoi " + tag] = (a, b, nl, 95.0)
    a, b = so.voronoi_pair((17, 20, 23), 6, 21)
    cases["voronoi 17x20x23 q50"] = (a, b, 6, 50.0)
    con = so.constructed()
    for tag in ("interior hole", "two components", "label 2 in A only, label 3 in B only", "values outside 1..nlabels",
                "opposite corners", "integer virtual index"):
        cases[tag] = con[tag] + (95.0,)
    out, lines = {}, ["goldens of tests/golden/op_surface.npz", "",
                      "medpy is NOT installed on the machine these were made on: its algorithm (medpy/metric/binary.py: hd, hd95,",
                      "assd over __surface_distances) is restated in make_goldens_surface.py over scipy.ndimage %s" % scipy.__version__,
                      "(binary_erosion + distance_transform_edt, the calls medpy makes), numpy %s." % np.__version__, "",
                      "per case: shape, nlabels, percentile, labels present in both maps, mean hd / hdq / assd over them", ""]
    for tag, (a, b, nl, q) in cases.items():
        rows = [per_label(a, b, l, q) for l in range(1, nl + 1)]
        m, c = np.array([r[0] for r in rows], np.float64), np.array([r[1] for r in rows], np.int64)
        out[tag + ".a"], out[tag + ".b"] = a.astype(np.int16), b.astype(np.int16)
        out[tag + ".nlabels"], out[tag + ".percentile"] = np.int64(nl), np.float64(q)
        out[tag + ".metrics"], out[tag + ".counts"] = m, c
        ok = ~np.isnan(m[:, 0])
        lines.append("%-40s %-10s nlabels %2d q %5.1f present %2d  hd %.6f hdq %.6f assd %.6f" % (
            tag, "x".join(map(str, a.shape)), nl, q, int(ok.sum()), *(m[ok, k].mean() if ok.any() else float("nan") for k in range(3))))
    np.savez_compressed(os.path.join(HERE, "op_surface.npz"), **out)
    lines.append("")
    lines.append("op_surface.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "op_surface.npz")))
    with open(os.path.join(HERE, "REPORT_surface.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
