"""Golden vectors for the SSIM3D loss, generated in fp64 by the REFERENCE's own class (Baseline methods/RCN/losses.py:103-126,
SSIM3D) and compared with the restatement of tests/ssim_oracle.py.  The reference tree is needed only here:

    SMILECODE_REFERENCE=<root of the reference tree> python tests/golden/make_goldens_ssim.py

Per case the file holds the two images (float32, as the kernels take them) and per window the value and both gradients (float64)
under ``<case>.w<window>.{loss,da,db}``; ``<case>.windows`` lists the windows.  Every case has the window 11; the small ones
also shorter ones, and ``tiny3x5x7`` has every axis shorter than the window."""
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
from smilecode_amd import synth  # noqa: E402
from tests import ssim_oracle  # noqa: E402


def cases():
    """(tag, a = img1, b = img2, windows)"""
    yield ("pair16",) + synth.make_pair((16, 16, 16), 24) + ((11,),)
    g = np.random.default_rng(7)
    u = lambda lo, hi, *s: g.uniform(lo, hi, (s[0], 1) + s[1:]).astype(np.float32)      # noqa: E731
    yield "noise2x6x10x14", u(-0.2, 1.2, 2, 6, 10, 14), u(-0.2, 1.2, 2, 6, 10, 14), (11, 3, 5, 7)
    yield "tiny3x5x7", u(0, 1, 1, 3, 5, 7), u(0, 1, 1, 3, 5, 7), (11, 3, 5, 7)           # every axis shorter than the window
    yield "one1x1x1", u(0, 1, 1, 1, 1, 1), u(0, 1, 1, 1, 1, 1), (11, 3)
    yield "wide6x7x9", u(-0.3, 2.3, 1, 6, 7, 9), u(-0.3, 2.3, 1, 6, 7, 9), (11, 5)


out, REPORT = {}, []
for tag, a_np, b_np, windows in cases():
    out[tag + ".a"], out[tag + ".b"], out[tag + ".windows"] = a_np, b_np, np.array(windows)
    for w in windows:
        a = torch.from_numpy(a_np).double().requires_grad_(True)
        b = torch.from_numpy(b_np).double().requires_grad_(True)
        lv = ref_losses.SSIM3D(window_size=w)(a, b)
        ga, gb = torch.autograd.grad(lv, [a, b])
        k = "%s.w%d" % (tag, w)
        out[k + ".loss"], out[k + ".da"], out[k + ".db"] = np.array(float(lv.detach())), ga.numpy(), gb.numpy()
        lo_, gao, gbo = ssim_oracle.value_and_grads(ssim_oracle.ssim_loss, a, b, torch.float64, window_size=w)
        REPORT.append("%s: |restatement - reference| loss %.3e (loss %.6e), gradient %.3e (max %.3e)" % (
            k, abs(float(lo_) - float(lv.detach())), float(lv.detach()), max(float((gao - ga).abs().max()), float((gbo - gb).abs().max())),
            max(float(ga.abs().max()), float(gb.abs().max()))))

np.savez_compressed(os.path.join(HERE, "op_ssim.npz"), **out)
with open(os.path.join(HERE, "REPORT_ssim.txt"), "w") as f:
    f.write("\n".join(REPORT) + "\n")
print("\n".join(REPORT))
print("op_ssim.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "op_ssim.npz")))
