"""Golden vectors for the RDN network, from the REAL reference ("Baseline methods/RDN/models.py" and losses.py) -- build
container only.

    python tests/golden/make_goldens_rdn.py <checkout of the reference>

Imports the reference files read-only (never copied, never shipped), runs RDN (levels [2,1,1,2]) and RDN_diff (levels [1,1,1,1])
with channels = 4 on the CPU in fp64 at 32 x 48 x 32, for B = 1 and B = 2, and writes
    tests/golden/e2e_rdn_32x48x32.npz    the seeded pair; per run y_moved, flow_out and the stage field (every STRIDE-th element),
                                         the loss NCC(y_moved) + Grad3d(stage field) as the reference's train loop forms it at one
                                         stage, and the reference's gradients of the encoder tensors, est0 and every bias (golden_tensor)
    tests/golden/rdn_state_dict.json     the state-dict keys and shapes of both classes
    tests/golden/REPORT_rdn.txt          max|oracle - reference| per quantity (tests/rdn_oracle.py in fp64)
Weights: tests/rdn_oracle.py make_weights (seeded, not stored)."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
from smilecode_amd import synth  # noqa: E402
from tests import rdn_oracle as orc  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Baseline methods", "RDN", "models.py")):
    sys.exit("usage: make_goldens_rdn.py <checkout of the reference (ZAX130/SmileCode)>")
REF = os.path.join(sys.argv[1], "Baseline methods", "RDN") + os.sep


def _load(name):
    spec = importlib.util.spec_from_file_location("rdn_ref_" + name, REF + name + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, ref_losses = _load("models"), _load("losses")
torch.set_num_threads(8)
LINES = []
SHAPE, STRIDE, PAIR_SEED, CHANNELS = (32, 48, 32), 101, 24, 4


def report(name, a, b):
    err, mag = float((a.detach().double() - b.detach().double()).abs().max()), float(b.detach().double().abs().max())
    LINES.append("%s\t%.6e\t%.6e" % (name, err, mag))
    return err


def ncc_ref(y_true, y_pred):
    """the reference's NCC_vxm hard-codes .to('cuda') and fp32 ones: patched for the call (as make_goldens.py does)"""
    orig, ones = torch.Tensor.to, torch.ones

    def to(self, *a, **k):
        return orig(self, *tuple("cpu" if (isinstance(x, str) and x == "cuda") else x for x in a), **k)

    torch.Tensor.to = to
    torch.ones = lambda *a, **k: ones(*a, **{**k, "dtype": y_true.dtype})
    try:
        return ref_losses.NCC_vxm()(y_true, y_pred)
    finally:
        torch.Tensor.to, torch.ones = orig, ones


def golden_tensor(n, B):
    """the parameters whose reference gradient is stored: the encoder, est0 and every bias.  The largest of them, the 13 824
    numbers of encoder.conv3.main.weight, are stored for the B = 2 runs only: fp64 gradients do not compress, and with all four
    copies the file would pass 1 MiB (the B = 1 runs compare that tensor with the oracle, which REPORT_rdn.txt ties to the
    reference at 1e-17)"""
    if n == "encoder.conv3.main.weight" and B == 1:
        return False
    return n.startswith("encoder.") or n.startswith("est0.") or n.endswith(".bias")


def e2e():
    p = orc.make_weights(channels=CHANNELS)
    mov2, fix2 = (torch.from_numpy(a) for a in synth.make_pair(SHAPE, PAIR_SEED, batch=2))
    out = {"shape": np.array(SHAPE), "stride": np.array(STRIDE), "moving": mov2.numpy(), "fixed": fix2.numpy(),
           "weights_seed": np.array(11), "channels": np.array(CHANNELS)}
    shapes = {}
    for run, (levels, diff) in orc.RUNS.items():
        cls = ref.RDN_diff if diff else ref.RDN
        for B in (1, 2):
            m = cls(SHAPE, channels=CHANNELS, stage_recursion=1, level_recursion=list(levels))
            shapes.setdefault(cls.__name__, {k: list(v.shape) for k, v in m.state_dict().items()})
            sd = m.state_dict()
            for n, v in p.items():
                assert tuple(sd[n].shape) == tuple(v.shape), n
                sd[n] = v.float()
            m.load_state_dict(sd)
            m = m.double()
            mov, fix = mov2[:B].double(), fix2[:B].double()
            y_ref, f_ref, s_ref = m(mov, fix)
            sim, reg = ncc_ref(fix, y_ref), ref_losses.Grad3d(penalty="l2")(s_ref, fix)
            loss = sim + reg
            params = dict(m.named_parameters())
            assert sorted(params) == sorted(p)
            kept = sorted(n for n in params if golden_tensor(n, B))
            g_ref = dict(zip(kept, torch.autograd.grad(loss, [params[n] for n in kept])))
            ol, osim, oreg, oy, oflow, os_, og = orc.value_and_grads(p, mov, fix, torch.float64, levels, diff)
            tag = "%s.B%d" % (run, B)
            for name, o_, r_ in (("flow_out", oflow, f_ref), ("y_moved", oy, y_ref), ("stage", os_, s_ref), ("loss", ol, loss)):
                report("e2e[%s] %s" % (tag, name), o_, r_)
            for name, r_ in (("flow_out", f_ref), ("y_moved", y_ref), ("stage", s_ref)):
                out["%s.%s" % (tag, name)] = np.ascontiguousarray(r_.detach().numpy().reshape(-1)[::STRIDE])
                out["%s.%s_absmax" % (tag, name)] = np.array(float(r_.abs().max()))
            out[tag + ".loss"] = np.array([float(loss), float(sim), float(reg)])
            for n in kept:
                report("e2e[%s] grad %s" % (tag, n), og[n], g_ref[n])
                out["%s.grad.%s" % (tag, n)] = g_ref[n].detach().numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "e2e_rdn_32x48x32.npz"), **out)
    with open(os.path.join(HERE, "rdn_state_dict.json"), "w") as f:
        json.dump(shapes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    e2e()
    with open(os.path.join(HERE, "REPORT_rdn.txt"), "w") as f:
        f.write("# tests/rdn_oracle.py (fp64) against the reference's RDN / RDN_diff in .double(), channels = 4, one stage: quantity <TAB> "
                "max|oracle - reference| <TAB> max|reference|\n# rdn: levels [2,1,1,2]; rdn_diff: levels [1,1,1,1], 7 integration steps; "
                "'stage' is the third output (the stage flow / the composed velocity)\n")
        f.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))
    for n in ("e2e_rdn_32x48x32.npz", "rdn_state_dict.json", "REPORT_rdn.txt"):
        print(n, os.path.getsize(os.path.join(HERE, n)))
