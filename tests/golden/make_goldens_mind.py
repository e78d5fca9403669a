"""Golden vectors for the MIND-SSC loss, generated in fp64 by the REFERENCE's own class (Baseline methods/RCN/losses.py:333-399,
MIND_loss) and compared with the gather-form restatement of tests/mind_oracle.py.  The reference tree is needed only here:

    SMILECODE_REFERENCE=<root of the reference tree> python tests/golden/make_goldens_mind.py

Two quirks of the reference: it calls .cuda() on its shift kernels (Tensor.cuda is patched to the identity) and builds them in
the default dtype (set to float64 for the run).  Per case the file holds the two images (float32, as the kernels take them),
the loss, both gradients and the first image's descriptor, all float64; the descriptor on the z planes listed beside it (all of
them but for the largest case, where the two border planes at the low end, an inner one and the last one keep the file below 1 MiB)."""
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
from tests import mind_oracle  # noqa: E402


def cases():
    yield ("pair16",) + synth.make_pair((16, 16, 16), 24)
    yield ("pair12x20x28",) + synth.make_pair((12, 20, 28), 31)
    g = np.random.default_rng(5)
    yield "noise2x10x12x14", g.uniform(0, 1, (2, 1, 10, 12, 14)).astype(np.float32), g.uniform(0, 1, (2, 1, 10, 12, 14)).astype(np.float32)
    yield "tiny3x4x5", g.uniform(0, 1, (1, 1, 3, 4, 5)).astype(np.float32), g.uniform(0, 1, (1, 1, 3, 4, 5)).astype(np.float32)


out, REPORT = {}, []
_cuda, _dtype = torch.Tensor.cuda, torch.get_default_dtype()
torch.Tensor.cuda = lambda self, *a, **k: self
torch.set_default_dtype(torch.float64)
try:
    ref = ref_losses.MIND_loss()
    for tag, a_np, b_np in cases():
        a = torch.from_numpy(a_np).double().requires_grad_(True)
        b = torch.from_numpy(b_np).double().requires_grad_(True)
        lv = ref(a, b)
        ga, gb = torch.autograd.grad(lv, [a, b])
        desc = ref.MINDSSC(a.detach())
        out[tag + ".a"], out[tag + ".b"] = a_np, b_np
        zs = np.array([0, 1, 6, 11] if tag == "pair12x20x28" else range(a_np.shape[2]))
        out[tag + ".loss"], out[tag + ".da"], out[tag + ".db"] = np.array(float(lv.detach())), ga.numpy(), gb.numpy()
        out[tag + ".mind_a"], out[tag + ".mind_a_z"] = desc.numpy()[:, :, zs], zs
        lo, gao, gbo = mind_oracle.value_and_grads(mind_oracle.mind_loss, a, b, torch.float64)
        do = mind_oracle.mind_ssc(a.detach())
        REPORT.append("%s: |restatement - reference| loss %.3e (loss %.6e), gradient %.3e (max %.3e), descriptor %.3e" % (
            tag, abs(float(lo) - float(lv)), float(lv), max(float((gao - ga).abs().max()), float((gbo - gb).abs().max())),
            float(ga.abs().max()), float((do - desc).abs().max())))
finally:
    torch.Tensor.cuda = _cuda
    torch.set_default_dtype(_dtype)

np.savez_compressed(os.path.join(HERE, "op_mind.npz"), **out)
with open(os.path.join(HERE, "REPORT_mind.txt"), "w") as f:
    f.write("\n".join(REPORT) + "\n")
print("\n".join(REPORT))
print("op_mind.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "op_mind.npz")))
