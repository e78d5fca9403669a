"""Golden vectors for RDN with recursive stages and its weight-shared forms, from the REAL reference ("Baseline methods/RDN/
models.py" and losses.py) -- build container only.

    python tests/golden/make_goldens_rdn_stages.py <checkout of the reference>

Imports the reference files read-only (never copied, never shipped), runs the four runs of tests/rdn_stages_oracle.py RUNS (RDN at
two stages, RDN_share at three, RDN_diff and RDN_diff_share at two) with channels = 4 on the CPU in fp64 at 32 x 48 x 32, for B = 1
and B = 2, and writes
    tests/golden/e2e_rdn_stages_32x48x32.npz   per run y_moved, flow_out and every stage field (every STRIDE-th element), the loss
                                               NCC(y_moved) + sum of Grad3d(stage field) as the reference's train loop forms it, and
                                               the reference's gradients of a subset of the parameters (golden_tensor)
    tests/golden/rdn_stages_state_dict.json    the state-dict keys and shapes of RDN and RDN_diff at two stages, RDN_share, RDN_diff_share
    tests/golden/REPORT_rdn_stages.txt         max|oracle - reference| per quantity (tests/rdn_stages_oracle.py in fp64)
The pair is that of tests/golden/e2e_rdn_32x48x32.npz (smilecode_amd.synth.make_pair, seeded, not stored again).  Weights:
tests/rdn_stages_oracle.py make_weights (seeded, not stored)."""
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
from tests import rdn_stages_oracle as orc  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Baseline methods", "RDN", "models.py")):
    sys.exit("usage: make_goldens_rdn_stages.py <checkout of the reference (ZAX130/SmileCode)>")
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
    """the reference's NCC_vxm hard-codes .to('cuda') and fp32 ones: patched for the call (as make_goldens_rdn.py does)"""
    orig, ones = torch.Tensor.to, torch.ones

    def to(self, *a, **k):
        return orig(self, *tuple("cpu" if (isinstance(x, str) and x == "cuda") else x for x in a), **k)

    torch.Tensor.to = to
    torch.ones = lambda *a, **k: ones(*a, **{**k, "dtype": y_true.dtype})
    try:
        return ref_losses.NCC_vxm()(y_true, y_pred)
    finally:
        torch.Tensor.to, torch.ones = orig, ones


def golden_tensor(n, stages):
    """the parameters whose reference gradient is stored: the two finest encoder layers, the LAST stage's (or the shared) level-0
    and level-3 flow convolutions and every bias.  fp64 gradients do not compress and eight runs share the file's 1 MiB; every
    other tensor is compared with the oracle, which REPORT_rdn_stages.txt ties to the reference."""
    if n.endswith(".bias"):
        return True
    if n.startswith("encoder.conv0.") or n.startswith("encoder.conv1."):
        return True
    last = n.split(".")[1] in ("conv", str(stages - 1))                          # estL.conv.* (shared) or estL.<last stage>.conv.*
    return n.endswith(".conv.4.weight") and n[:4] in ("est0", "est3") and last


def e2e():
    mov2, fix2 = (torch.from_numpy(a) for a in synth.make_pair(SHAPE, PAIR_SEED, batch=2))
    stored = np.load(os.path.join(HERE, "e2e_rdn_32x48x32.npz"))               # the tests read the pair from there
    assert np.array_equal(stored["moving"], mov2.numpy()) and np.array_equal(stored["fixed"], fix2.numpy())
    out = {"shape": np.array(SHAPE), "stride": np.array(STRIDE), "pair_seed": np.array(PAIR_SEED), "weights_seed": np.array(11),
           "channels": np.array(CHANNELS)}
    shapes = {}
    for run, (cls_name, stages, levels, diff, share) in orc.RUNS.items():
        cls = getattr(ref, cls_name)
        p = orc.make_weights(stages, share, channels=CHANNELS)
        for B in (1, 2):
            m = cls(SHAPE, channels=CHANNELS, stage_recursion=stages, level_recursion=list(levels))
            shapes.setdefault(cls.__name__, {k: list(v.shape) for k, v in m.state_dict().items()})
            sd = m.state_dict()
            for n, v in p.items():
                assert tuple(sd[n].shape) == tuple(v.shape), n
                sd[n] = v.float()
            m.load_state_dict(sd)
            m = m.double()
            mov, fix = mov2[:B].double(), fix2[:B].double()
            outs = m(mov, fix)
            y_ref, f_ref, s_ref = outs[0], outs[1], list(outs[2:])
            assert len(s_ref) == stages
            sim = ncc_ref(fix, y_ref)
            reg = sum(ref_losses.Grad3d(penalty="l2")(s, fix) for s in s_ref)
            loss = sim + reg
            params = dict(m.named_parameters())
            assert sorted(params) == sorted(p)
            kept = sorted(n for n in params if golden_tensor(n, stages))
            g_ref = dict(zip(kept, torch.autograd.grad(loss, [params[n] for n in kept])))
            ol, osim, oreg, oy, oflow, ofields, og = orc.value_and_grads(p, mov, fix, torch.float64, stages, levels, diff, share)
            tag = "%s.B%d" % (run, B)
            named = [("flow_out", oflow, f_ref), ("y_moved", oy, y_ref)] + [("stage%d" % i, ofields[i], s_ref[i]) for i in range(stages)]
            for name, o_, r_ in named + [("loss", ol, loss)]:
                report("e2e[%s] %s" % (tag, name), o_, r_)
            for name, _, r_ in named:
                out["%s.%s" % (tag, name)] = np.ascontiguousarray(r_.detach().numpy().reshape(-1)[::STRIDE])
                out["%s.%s_absmax" % (tag, name)] = np.array(float(r_.abs().max()))
            out[tag + ".loss"] = np.array([float(loss), float(sim), float(reg)])
            for n in kept:
                report("e2e[%s] grad %s" % (tag, n), og[n], g_ref[n])
                out["%s.grad.%s" % (tag, n)] = g_ref[n].detach().numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "e2e_rdn_stages_32x48x32.npz"), **out)
    with open(os.path.join(HERE, "rdn_stages_state_dict.json"), "w") as f:
        json.dump(shapes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    e2e()
    with open(os.path.join(HERE, "REPORT_rdn_stages.txt"), "w") as f:
        f.write("# tests/rdn_stages_oracle.py (fp64) against the reference's RDN / RDN_share / RDN_diff / RDN_diff_share in .double(), "
                "channels = 4: quantity <TAB> max|oracle - reference| <TAB> max|reference|\n# rdn_s2: RDN, 2 stages, levels [1,1,1,2]; "
                "share_s3: RDN_share, 3 stages, [1,1,1,1]; diff_s2: RDN_diff, 2 stages, [1,1,1,1]; diff_share_s2: RDN_diff_share, 2 "
                "stages, [1,1,2,1]; 'stageN' is output 2 + N (the stage flow / the composed velocity)\n")
        f.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))
    for n in ("e2e_rdn_stages_32x48x32.npz", "rdn_stages_state_dict.json", "REPORT_rdn_stages.txt"):
        print(n, os.path.getsize(os.path.join(HERE, n)))
