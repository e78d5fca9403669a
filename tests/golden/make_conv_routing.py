"""Records tests/golden/conv_routing.npz: which kernel family libmodet_hip.so routes each fp32 3x3x3 convolution to, and
the size / capability queries that must follow the same route, over a fixed grid of shapes.  Host-only (no GPU needed).

A deliberate change of the routing policy is the ONLY reason to rerun this script.  The table pins the policy:
tests/test_cpu.py::test_conv_routing_matches_the_recorded_table compares the library with it entry by entry, so a
refactor of the dispatch code is checked against the table as recorded BEFORE it, never against a fresh recording.

    python tests/golden/make_conv_routing.py            # writes conv_routing.npz beside this file
"""
import os
import sys

import numpy as np

VOLUMES = [(1, 8, 8, 8), (1, 10, 12, 10), (2, 10, 12, 10), (1, 16, 16, 16), (1, 20, 24, 20), (2, 20, 24, 20), (1, 32, 48, 32),
           (2, 32, 48, 32), (1, 40, 48, 40), (2, 40, 48, 40), (1, 64, 64, 64), (1, 80, 96, 80), (2, 80, 96, 80),
           (1, 160, 192, 160), (2, 160, 192, 160), (2, 160, 192, 224), (4, 160, 192, 224), (1, 12, 20, 7), (3, 33, 17, 65)]
CHANNELS = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128]
PASSES = [0, 1, 2]              # forward, data gradient, weight gradient
VARIANTS = [0, 1, 2, 3]         # plain, fused LeakyReLU, normalised input, fused statistics


def table(L):
    """the routing of library L over the grid: int8 arrays indexed [volume, Cin, Cout(, pass, variant)]"""
    nv, nc = len(VOLUMES), len(CHANNELS)
    t = {"family": np.zeros((nv, nc, nc, len(PASSES), len(VARIANTS)), np.int8)}
    # the *_bytes queries only as zero / non-zero: their values for the exact-f32 family depend on an occupancy query
    for name in ("wgrad_normin_ok", "wgrad_defers_operands", "stats_nonzero", "normin_stats_nonzero", "dgrad_instats_nonzero"):
        t[name] = np.zeros((nv, nc, nc), np.int8)
    for iv, (B, D, H, W) in enumerate(VOLUMES):
        for ii, ci in enumerate(CHANNELS):
            for io, co in enumerate(CHANNELS):
                a = (B, D, H, W, ci, co)
                for p in PASSES:
                    for v in VARIANTS:
                        t["family"][iv, ii, io, p, v] = L.modet_conv3d_kernel_family_v(*a, p, v)
                t["wgrad_normin_ok"][iv, ii, io] = L.modet_conv3d_bwd_weight_normin_ok(*a)
                t["wgrad_defers_operands"][iv, ii, io] = L.modet_conv3d_wgrad_defers_operands(*a)
                t["stats_nonzero"][iv, ii, io] = L.modet_conv3d_stats_bytes(*a) != 0
                t["normin_stats_nonzero"][iv, ii, io] = L.modet_conv3d_normin_stats_bytes(*a) != 0
                t["dgrad_instats_nonzero"][iv, ii, io] = L.modet_conv3d_bwd_data_instats_bytes(*a) != 0
    return t


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(os.path.dirname(here)))
    from smilecode_amd import _lib
    out = os.path.join(here, "conv_routing.npz")
    np.savez_compressed(out, **table(_lib.load()))
    print("wrote", out)
