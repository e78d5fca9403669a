"""Golden vectors for the RCN / VTN network, from the REAL reference ("Baseline methods/RCN/models.py" and losses.py) -- build
container only.

    python tests/golden/make_goldens_rcn.py <checkout of the reference>

Imports the reference files read-only (never copied, never shipped), runs VTN(warp=True) and RCN(n_cascade=2, flow_multiplier=2)
with channels = 4 on the CPU in fp64 at 64 x 64 x 128 (the smallest legal size: a 1 x 1 x 2 grid at conv6), for B = 1 and B = 2,
and writes
    tests/golden/e2e_rcn_64x64x128.npz   per run moved, flow and every subflow (every STRIDE-th element), the loss NCC(moved) +
                                         sum of Grad3d('l2') over the subflows as the reference's train loop forms it, and the
                                         reference's gradients of every bias, every Upsamp*.upconv.weight, Deconv1.upconv.weight,
                                         Pred0.upconv.weight and encoder.conv1.main.weight; every STRIDE-th voxel of the seeded pair
    tests/golden/rcn_state_dict.json     the state-dict keys and shapes of VTN, RCN and RCN_test
    tests/golden/REPORT_rcn.txt          max|oracle - reference| per quantity (tests/rcn_oracle.py in fp64) and max |w| per subflow
Weights: tests/rcn_oracle.py golden_weights (seeded, not stored).  The pair: smilecode_amd.synth.make_pair (seeded, not stored)."""
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
from tests import rcn_oracle as orc  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Baseline methods", "RCN", "models.py")):
    sys.exit("usage: make_goldens_rcn.py <checkout of the reference (ZAX130/SmileCode)>")
REF = os.path.join(sys.argv[1], "Baseline methods", "RCN") + os.sep


def _load(name):
    spec = importlib.util.spec_from_file_location("rcn_ref_" + name, REF + name + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, ref_losses = _load("models"), _load("losses")
torch.set_num_threads(8)
LINES = []
SHAPE, STRIDE, CHANNELS = orc.GOLD_SHAPE, 997, orc.GOLD_CHANNELS


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


def golden_tensor(n):
    """the parameters whose reference gradient is stored; the others come from the oracle in fp64 at test time"""
    tail = n.split("vtn.")[-1].split(".", 1)[-1] if n.startswith("vtn.") else n
    return (n.endswith(".bias") or (tail.startswith("Upsamp") and tail.endswith("upconv.weight"))
            or tail in ("Deconv1.upconv.weight", "Pred0.upconv.weight", "encoder.conv1.main.weight"))


def e2e():
    mov2, fix2 = orc.golden_pair()
    out = {"shape": np.array(SHAPE), "stride": np.array(STRIDE), "channels": np.array(CHANNELS),
           "moving": mov2.numpy().reshape(-1)[::STRIDE].copy(), "fixed": fix2.numpy().reshape(-1)[::STRIDE].copy(),
           "pair_sum": np.array([float(mov2.double().sum()), float(fix2.double().sum())])}
    shapes = {}
    for cls, kw in ((ref.VTN, {}), (ref.RCN, {"n_cascade": 2}), (ref.RCN_test, {"n_cascade": 2})):
        shapes[cls.__name__] = {k: list(v.shape) for k, v in cls(SHAPE, channels=CHANNELS, **kw).state_dict().items()}
    for run, (n_cascade, fm) in orc.RUNS.items():
        p = orc.golden_weights(run)
        for B in (1, 2):
            m = ref.RCN(SHAPE, flow_multiplier=fm, channels=CHANNELS, n_cascade=n_cascade) if n_cascade else \
                ref.VTN(SHAPE, flow_multiplier=fm, channels=CHANNELS, warp=True)
            sd = m.state_dict()
            for n, v in p.items():
                assert tuple(sd[n].shape) == tuple(v.shape), n
                sd[n] = v.float()
            m.load_state_dict(sd)
            m = m.double()
            mov, fix = mov2[:B].double(), fix2[:B].double()
            res = m(mov, fix)
            moved, flow, subs = res[0], res[1], (list(res[2:]) if n_cascade else [res[1]])
            loss = ncc_ref(fix, moved)
            for w in subs:
                loss = loss + ref_losses.Grad3d(penalty="l2")(w, fix)
            params = dict(m.named_parameters())
            assert sorted(params) == sorted(p)
            kept = sorted(n for n in params if golden_tensor(n))
            g_ref = dict(zip(kept, torch.autograd.grad(loss, [params[n] for n in kept])))
            ol, omoved, oflow, osubs, og = orc.value_and_grads(p, mov, fix, n_cascade, torch.float64, fm)
            tag = "%s.B%d" % (run, B)
            named = [("flow", oflow, flow), ("moved", omoved, moved), ("loss", ol, loss)]
            named += [("subflow%d" % i, o_, r_) for i, (o_, r_) in enumerate(zip(osubs, subs))]
            for name, o_, r_ in named:
                report("e2e[%s] %s" % (tag, name), o_, r_)
                if name != "loss":
                    out["%s.%s" % (tag, name)] = np.ascontiguousarray(r_.detach().numpy().reshape(-1)[::STRIDE])
                    out["%s.%s_absmax" % (tag, name)] = np.array(float(r_.abs().max()))
            for i, w in enumerate(subs):
                amax = float(w.abs().max())
                assert orc.SUBFLOW_RANGE[0] <= amax <= orc.SUBFLOW_RANGE[1], (tag, i, amax)
                LINES.append("range[%s] max|subflow%d| (voxels, condition %g..%g)\t%.6e\t%.6e" % ((tag, i) + orc.SUBFLOW_RANGE + (0.0, amax)))
            out[tag + ".loss"] = np.array([float(loss)])
            for n in kept:
                report("e2e[%s] grad %s" % (tag, n), og[n], g_ref[n])
                out["%s.grad.%s" % (tag, n)] = g_ref[n].detach().numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "e2e_rcn_64x64x128.npz"), **out)
    with open(os.path.join(HERE, "rcn_state_dict.json"), "w") as f:
        json.dump(shapes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    e2e()
    with open(os.path.join(HERE, "REPORT_rcn.txt"), "w") as f:
        f.write("# tests/rcn_oracle.py (fp64) against the reference's VTN(warp=True) and RCN(n_cascade=2, flow_multiplier=2) in .double(), "
                "channels = 4, 64 x 64 x 128: quantity <TAB> max|oracle - reference| <TAB> max|reference|\n")
        f.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))
    for n in ("e2e_rcn_64x64x128.npz", "rcn_state_dict.json", "REPORT_rcn.txt"):
        print(n, os.path.getsize(os.path.join(HERE, n)))
