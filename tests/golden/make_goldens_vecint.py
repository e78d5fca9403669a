"""Golden vectors for the velocity-field integration of include/modet_hip_vecint.h, generated in fp64 on the CPU by the
REFERENCE's own class (ModeT/models.py:70-87, VecInt over its SpatialTransformer: normalised grid -> grid_sample) and compared
with the restatement of tests/vecint_oracle.py.  The reference tree is needed only here:

    SMILECODE_REFERENCE=<root of the reference tree> python tests/golden/make_goldens_vecint.py

Per golden case of vecint_oracle.CASES the file holds the output ``<case>.out`` and the gradient ``<case>.grad`` (float64, planar
(B,3,D,H,W)) for the seeded cotangent; the fields themselves are rebuilt from their seeds (vecint_oracle.case_field).  The
report also lists, for every case, the kink margin and the fp32 coordinate error (vecint_oracle.margin_and_coord_error)."""
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
sys.path.insert(0, os.path.join(REF, "ModeT"))
import models as ref_models  # noqa: E402  (the reference)
from tests import vecint_oracle as vo  # noqa: E402

out, REPORT = {}, []
for tag, (kind, B, shape, amp, nsteps, seed, golden) in vo.CASES.items():
    w = vo.case_field(tag)
    margin, e_coord = vo.margin_and_coord_error(w, nsteps)
    line = "%s: margin %.3e, e_coord %.3e (ratio %.1f)" % (tag, margin, e_coord, margin / max(e_coord, 1e-300))
    if golden:
        ref = ref_models.VecInt(shape, nsteps).double()
        wr = w.clone().requires_grad_(True)
        o = ref(wr)
        (g,) = torch.autograd.grad(o, [wr], vo.cotangent(o.shape))
        out[tag + ".out"], out[tag + ".grad"] = o.detach().numpy(), g.numpy()
        o2, g2 = vo.value_and_grad(w, nsteps, torch.float64)
        line += "; |restatement - reference| out %.3e (max %.3e), gradient %.3e (max %.3e)" % (
            float((o2 - o.detach()).abs().max()), float(o.detach().abs().max()), float((g2 - g).abs().max()), float(g.abs().max()))
    REPORT.append(line)

np.savez_compressed(os.path.join(HERE, "op_vecint.npz"), **out)
with open(os.path.join(HERE, "REPORT_vecint.txt"), "w") as fh:
    fh.write("\n".join(REPORT) + "\n")
print("\n".join(REPORT))
print("op_vecint.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "op_vecint.npz")))
