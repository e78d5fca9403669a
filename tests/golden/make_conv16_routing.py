"""Records tests/golden/conv16_routing.npz: which kernel family libmodet_hip.so routes each bf16-STORAGE 3x3x3 convolution to
(modet_conv3d_bf16_kernel_family: 1 = tiled, 2 = z-march), and the exact values of the size queries that must follow the same
route, over make_conv_routing.py's volumes.  Host-only (no GPU needed): the three queries are plain host arithmetic, no
occupancy query, so their values are recorded, not just zero / non-zero.

A deliberate change of the routing policy or of a buffer layout is the ONLY reason to rerun this script.
tests/test_cpu.py::test_conv16_routing_matches_the_recorded_table compares the library with the table entry by entry, so a
refactor of the dispatch code is checked against the table as recorded BEFORE it, never against a fresh recording.

    python tests/golden/make_conv16_routing.py          # writes conv16_routing.npz beside this file
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_conv_routing import VOLUMES  # noqa: E402  (the same grid of volumes as the fp32 table)

CHANNELS = [4, 8, 12, 16, 24, 32, 48, 64, 96, 128]
PASSES = [0, 1, 2]              # forward, data gradient, weight gradient
X_BF16 = [0, 1]                 # the activation (forward, weight gradient) / the data gradient's output is fp32 | bf16


def table(L):
    """the routing of library L over the grid: family int8 [volume, Cin, Cout, pass, x_bf16]; byte counts int64"""
    nv, nc = len(VOLUMES), len(CHANNELS)
    t = {"family": np.zeros((nv, nc, nc, len(PASSES), len(X_BF16)), np.int8),
         "stats_bytes": np.zeros((nv, nc, nc), np.int64),
         "bwd_weight_ws_bytes": np.zeros((nv, nc, nc), np.int64),
         "ws_bytes": np.zeros((nc, nc), np.int64)}
    for ii, ci in enumerate(CHANNELS):
        for io, co in enumerate(CHANNELS):
            t["ws_bytes"][ii, io] = L.modet_conv3d_bf16_ws_bytes(ci, co)
            for iv, (B, D, H, W) in enumerate(VOLUMES):
                a = (B, D, H, W, ci, co)
                for p in PASSES:
                    for xb in X_BF16:
                        t["family"][iv, ii, io, p, xb] = L.modet_conv3d_bf16_kernel_family(*a, p, xb)
                t["stats_bytes"][iv, ii, io] = L.modet_conv3d_bf16_stats_bytes(*a)
                t["bwd_weight_ws_bytes"][iv, ii, io] = L.modet_conv3d_bf16_bwd_weight_ws_bytes(*a)
    return t


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(os.path.dirname(here)))
    from smilecode_amd import _lib
    out = os.path.join(here, "conv16_routing.npz")
    np.savez_compressed(out, **table(_lib.load()))
    print("wrote", out)
