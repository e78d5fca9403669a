"""The surface-distance semantics of include/modet_hip_surface.h restated in numpy, sharing no algorithm with the kernels (no
distance transform, no histogram): the border by shifted comparisons on a zero-padded mask, ALL PAIRS of int64 squared distances
between the two border point sets, np.percentile, fp64 means.  Plus the label maps the tests run on: Voronoi maps of seeded
points, which hold every label by construction, and the constructed cases."""
import numpy as np

COLUMNS = ("hd", "hdq", "assd", "asd_ab", "asd_ba")
COUNTS = ("n_a", "n_b", "nborder_a", "nborder_b", "hd2", "q_lo2", "q_hi2")


def border_points(mask):
    """(n, 3) int64 coordinates of the voxels of ``mask`` with a 6-neighbour outside it (the volume's outside counts)"""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    c = m[1:-1, 1:-1, 1:-1]
    inner = (c & m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[1:-1, 1:-1, :-2]
             & m[1:-1, 1:-1, 2:])
    return np.argwhere(c & ~inner).astype(np.int64)


def nearest_d2(src, dst, block=2048):
    """for every point of ``src`` the smallest squared distance to a point of ``dst`` (int64, all pairs, in blocks of rows)"""
    out = np.empty(len(src), dtype=np.int64)
    for i in range(0, len(src), block):
        d = src[i:i + block, None, :] - dst[None, :, :]
        out[i:i + block] = (d * d).sum(-1).min(1)
    return out


def label_metrics(a, b, label, percentile=95.0):
    """-> (metrics (5,) float64, counts (7,) int64) of one label"""
    ma, mb = np.asarray(a) == label, np.asarray(b) == label
    pa, pb = border_points(ma), border_points(mb)
    counts = np.array([ma.sum(), mb.sum(), len(pa), len(pb), -1, -1, -1], dtype=np.int64)
    if counts[0] == 0 or counts[1] == 0:
        return np.full(5, np.nan), counts
    ab, ba = nearest_d2(pa, pb), nearest_d2(pb, pa)
    both = np.sort(np.hstack((ab, ba)))
    n = len(both)
    q = float(np.float32(percentile))                       # the C ABI takes a float
    vi = (n - 1) * (q / 100.0)
    k_lo = min(int(np.floor(vi)), n - 1)
    k_hi = min(k_lo + 1, n - 1)
    counts[4:] = (both[-1], both[k_lo], both[k_hi])
    asd_ab, asd_ba = np.sqrt(ab.astype(np.float64)).mean(), np.sqrt(ba.astype(np.float64)).mean()
    hdq = np.percentile(np.hstack((np.sqrt(ab.astype(np.float64)), np.sqrt(ba.astype(np.float64)))), q)
    return np.array([np.sqrt(np.float64(both[-1])), hdq, (asd_ab + asd_ba) / 2.0, asd_ab, asd_ba]), counts


def surface_distances(a, b, nlabels, percentile=95.0):
    """-> (metrics (nlabels, 5) float64, counts (nlabels, 7) int64), the layout of ops.surface_distances"""
    rows = [label_metrics(a, b, l, percentile) for l in range(1, nlabels + 1)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


# ------------------------------------------------------------------------------------------------ label maps
def voronoi(shape, seeds):
    """int16 map: voxel -> 1 + index of the nearest seed (ties to the lower index); seeds are distinct voxels, so every label occurs"""
    zz, yy, xx = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    p = np.stack((zz, yy, xx), -1).reshape(-1, 1, 3).astype(np.int64)
    d = ((p - seeds[None].astype(np.int64)) ** 2).sum(-1)
    return (1 + d.argmin(1)).reshape(shape).astype(np.int16)


def voronoi_pair(shape, nlabels, seed):
    """two Voronoi maps with ``nlabels`` labels each: distinct seed voxels, and the same seeds jittered by up to one voxel (kept
    distinct and inside the volume) for the second map"""
    g = np.random.default_rng([int(seed), 17])
    nvox = int(np.prod(shape))
    assert nlabels <= nvox
    flat = g.choice(nvox, size=nlabels, replace=False)
    seeds = np.stack(np.unravel_index(flat, shape), -1)
    for _ in range(100):
        moved = np.clip(seeds + g.integers(-1, 2, seeds.shape), 0, np.array(shape) - 1)
        if len(np.unique(moved, axis=0)) == nlabels:
            break
    else:
        moved = seeds
    return voronoi(shape, seeds), voronoi(shape, moved)


# tag -> (shape, nlabels, seed): what each shape is for is said in tests/test_gpu_surface.py
VORONOI = {
    "5x6x7": ((5, 6, 7), 4, 1), "4x5x67": ((4, 5, 67), 5, 2), "3x4x300": ((3, 4, 300), 6, 3), "9x13x35": ((9, 13, 35), 7, 4),
    "1x1x9": ((1, 1, 9), 2, 5), "1x8x8": ((1, 8, 8), 3, 6), "40x48x40": ((40, 48, 40), 8, 7),
}


def constructed():
    """tag -> (a, b, nlabels): the cases built by hand"""
    c = {}
    full = np.ones((4, 5, 6), np.int16)
    part = full.copy(); part[:, :, 4:] = 0
    c["one label fills the volume"] = (full, part, 1)
    a, _ = voronoi_pair((6, 7, 9), 3, 11)
    c["identical maps"] = (a, a.copy(), 3)
    p, q = np.zeros((3, 4, 5), np.int16), np.zeros((3, 4, 5), np.int16)
    p[0, 0, 0] = 1; q[2, 3, 4] = 1
    c["opposite corners"] = (p, q, 1)
    h = np.zeros((9, 9, 11), np.int16); h[1:8, 1:8, 1:10] = 2
    hb = h.copy(); h[3:6, 3:6, 4:7] = 0; hb[4, 4, 5] = 0
    c["interior hole"] = (h, hb, 2)
    t = np.zeros((6, 8, 20), np.int16); t[1:4, 1:4, 1:5] = 1; t[2:5, 3:7, 14:19] = 1
    tb = np.zeros_like(t); tb[1:5, 2:6, 3:16] = 1
    c["two components"] = (t, tb, 1)
    a, b = (m.copy() for m in voronoi_pair((7, 8, 9), 4, 12))
    b[b == 2] = 1; a[a == 3] = 4
    c["label 2 in A only, label 3 in B only"] = (a, b, 4)
    a, b = (m.copy() for m in voronoi_pair((7, 8, 9), 6, 13))
    a[a == 5] = -3; b[b == 5] = 300; a[a == 6] = 32767; b[b == 6] = -32768
    c["values outside 1..nlabels"] = (a, b, 4)
    a, b = voronoi_pair((8, 9, 10), 5, 14)
    c["nlabels=1 of 5"] = (a, b, 1)
    a, b = voronoi_pair((8, 9, 10), 3, 15)
    c["nlabels=54, most absent"] = ((a * 17).astype(np.int16), (b * 17).astype(np.int16), 54)
    two_a, two_b = np.zeros((2, 3, 4), np.int16), np.zeros((2, 3, 4), np.int16)
    two_a[0, 1, 1] = 1; two_b[1, 2, 3] = 1
    c["two border voxels in all"] = (two_a, two_b, 1)
    # 6 + 15 = 21 border voxels: (n - 1) * 0.95 = 19 and (n - 1) * 0.5 = 10 are integers
    ra, rb = np.zeros((3, 4, 9), np.int16), np.zeros((3, 4, 9), np.int16)
    ra[1, 1, 1:7] = 1; rb[0, 3, 0:8] = 1; rb[2, 0, 1:8] = 1
    c["integer virtual index"] = (ra, rb, 1)
    return c


def labels_above_the_lds_table():
    """labels on both sides of 1024 (the kernels count labels up to there in LDS first): 1, 1024, 1025 and 3000 of nlabels 3000"""
    a, b = voronoi_pair((6, 10, 12), 4, 16)
    remap = np.array([0, 1, 1024, 1025, 3000], np.int16)
    return remap[a], remap[b], 3000
