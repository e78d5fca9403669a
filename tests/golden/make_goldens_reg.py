"""Golden vectors for the flow regularisers of include/modet_hip_reg.h, generated in fp64 by the REFERENCE's own classes (Baseline
methods/RCN/losses.py:203-268, Grad3DiTV and DisplacementRegularizer) and compared with the restatement of tests/reg_oracle.py.
The reference tree is needed only here:

    SMILECODE_REFERENCE=<root of the reference tree> python tests/golden/make_goldens_reg.py

Per case the file holds the flow ``<case>.f`` (float32, planar (B,C,D,H,W), as the kernels take it), the kinds it holds under
``<case>.kinds`` and per kind the value and the gradient (float64) under ``<case>.<kind>.{loss,grad}``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("SMILECODE_REFERENCE")
if not REF:
    sys.exit("set SMILECODE_REFERENCE to the root of the reference tree")
sys.path.insert(0, os.path.join(REF, "Baseline methods", "RCN"))
import losses as ref_losses  # noqa: E402  (the reference)
from tests import reg_oracle  # noqa: E402

ALL = ("itv", "gradient-l2", "gradient-l1", "bending")


def cases():
    """(tag, flow, kinds)"""
    g = np.random.default_rng(11)
    n = lambda *s: g.normal(0.0, 1.0, s).astype(np.float32)      # noqa: E731
    yield "noise2x3x5x5x5", n(2, 3, 5, 5, 5), ALL                # bending's minimum: one point per channel, every voxel in the shell
    yield "noise1x3x6x7x9", n(1, 3, 6, 7, 9), ALL
    yield "noise1x3x9x9x9", n(1, 3, 9, 9, 9), ALL                # the first shape with a voxel at least 4 from every face
    z, y, x = np.meshgrid(np.arange(8.0), np.arange(10.0), np.arange(37.0), indexing="ij")
    smooth = np.stack([2.0 * np.sin(0.31 * x + 0.7 * c) * np.cos(0.23 * y - 0.4 * c) + 0.8 * np.sin(0.45 * z + 0.17 * x + c)
                       for c in range(3)])[None]
    yield "smooth1x3x8x10x37", (smooth + 0.05 * 2.0 * g.normal(0.0, 1.0, smooth.shape)).astype(np.float32), ALL
    slab = n(1, 3, 7, 8, 9)
    slab[:, :, 2:6, 3:7, 1:5] = np.float32(0.75)                 # an exactly constant 4 x 4 x 4 block: differences of exactly 0
    yield "slab1x3x7x8x9", slab, ALL
    yield "zero1x3x6x6x6", np.zeros((1, 3, 6, 6, 6), np.float32), ALL
    yield "itv2x2x2x3x4", n(2, 2, 2, 3, 4), ("itv",)             # two channels, at iTV's minimum sizes
    yield "itv1x1x4x5x6", n(1, 1, 4, 5, 6), ("itv",)


def reference(kind):
    if kind == "itv":
        return ref_losses.Grad3DiTV()
    return ref_losses.DisplacementRegularizer(kind)


out, REPORT = {}, []
for tag, f_np, kinds in cases():
    out[tag + ".f"], out[tag + ".kinds"] = f_np, np.array(kinds)
    for kind in kinds:
        f = torch.from_numpy(f_np).double().requires_grad_(True)
        lv = reference(kind)(f, None)
        (gf,) = torch.autograd.grad(lv, [f])
        k = "%s.%s" % (tag, kind)
        out[k + ".loss"], out[k + ".grad"] = np.array(float(lv.detach())), gf.numpy()
        lo_, go = reg_oracle.value_and_grad(reg_oracle.KINDS[kind], f, torch.float64)
        REPORT.append("%s: |restatement - reference| loss %.3e (loss %.6e), gradient %.3e (max %.3e)" % (
            k, abs(float(lo_) - float(lv.detach())), float(lv.detach()), float((go - gf).abs().max()), float(gf.abs().max())))

np.savez_compressed(os.path.join(HERE, "op_reg.npz"), **out)
with open(os.path.join(HERE, "REPORT_reg.txt"), "w") as fh:
    fh.write("\n".join(REPORT) + "\n")
print("\n".join(REPORT))
print("op_reg.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "op_reg.npz")))
