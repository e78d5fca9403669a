"""Golden vectors for the PCNet network, from the REAL reference ("Baseline methods/PCnet/models.py" and losses.py) -- build
container only.

    python tests/golden/make_goldens_pcnet.py <checkout of the reference>

Imports the reference files read-only (never copied, never shipped), runs PCNet(channels = 4) on the CPU in fp64 at 32 x 48 x 32
(a 4 x 6 x 4 grid at level 3), for B = 1 and B = 2, and writes
    tests/golden/e2e_pcnet_32x48x32.npz   per run moved, flow, the three warping fields and the integrated last prediction (every
                                          STRIDE-th element), the loss NCC(moved) + Grad3d('l2')(flow) as the reference's train
                                          loop forms it, and the reference's gradients of every bias, every fc weight, every
                                          weight_conv / reg_conv weight and both encoders' first convolution; every STRIDE-th voxel
                                          of the seeded pair
    tests/golden/pcnet_state_dict.json    the state-dict keys and shapes of PCNet(channels = 4) here and of the default width at 16^3
    tests/golden/REPORT_pcnet.txt         max|oracle - reference| per quantity (tests/pcnet_oracle.py in fp64), max |w| per field,
                                          and per NFF block the smallest argmax gap beside ATen fp32's error on the pooled tensor
Weights: tests/pcnet_oracle.py golden_weights (seeded, not stored); the seed is the first from SEED_FROM on whose run meets THE
ARGMAX CONDITION (every pooled channel's two largest values differ by at least 100 x the fp32 error of that tensor), measured on
the reference itself through a forward hook on nff_k.channel_attention.  The pair: smilecode_amd.synth.make_pair (seeded, not stored)."""
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
from tests import pcnet_oracle as orc  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Baseline methods", "PCnet", "models.py")):
    sys.exit("usage: make_goldens_pcnet.py <checkout of the reference (ZAX130/SmileCode)>")
REF = os.path.join(sys.argv[1], "Baseline methods", "PCnet") + os.sep


def _load(name):
    spec = importlib.util.spec_from_file_location("pcnet_ref_" + name, REF + name + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, ref_losses = _load("models"), _load("losses")
torch.set_num_threads(8)
LINES = []
SHAPE, STRIDE, CHANNELS, SEED_FROM = orc.GOLD_SHAPE, 211, orc.GOLD_CHANNELS, 31


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
    return (n.endswith(".bias") or ".fc." in n or ".weight_conv." in n or n.startswith("reg_conv")
            or n in ("encoder_float.conv0.main.weight", "encoder_fixed.conv0.main.weight"))


def reference(p, dtype):
    m = ref.PCNet(SHAPE, channels=CHANNELS)
    sd = m.state_dict()
    for n, v in p.items():
        assert tuple(sd[n].shape) == tuple(v.shape), n
        sd[n] = v.float()
    m.load_state_dict(sd)
    return m.to(dtype)


def run_reference(m, mov, fix):
    """-> (moved, flow, the tensors each nff_k.channel_attention pooled, the fields) of one forward of the reference"""
    pooled, fields, hooks = {}, {}, []
    for k in (2, 1, 0):
        hooks.append(getattr(m, "nff_%d" % k).channel_attention.register_forward_hook(
            lambda mod, inp, out, k=k: pooled.__setitem__("nff_%d.cat" % k, inp[0].detach())))
        hooks.append(getattr(m, "dfi_%d" % k).register_forward_hook(
            lambda mod, inp, out, k=k: fields.__setitem__("warping_field_%d" % k, out)))
    calls = []
    hooks.append(m.integrate.register_forward_hook(lambda mod, inp, out: calls.append(out)))
    moved, flow = m(mov, fix)
    for h in hooks:
        h.remove()
    fields["pred0"] = calls[-1]
    return moved, flow, pooled, fields


def condition(p, mov, fix):
    """tap -> (smallest gap in the reference's fp64 run, the fp32 run's relative error on that tensor)"""
    with torch.no_grad():
        p64 = run_reference(reference(p, torch.float64), mov.double(), fix.double())[2]
        p32 = run_reference(reference(p, torch.float32), mov.float(), fix.float())[2]
    return {k: (float(orc.cat_gaps(p64[k]).min()), float((p32[k].double() - p64[k]).abs().max()) / float(p64[k].abs().max()))
            for k in orc.NFF_TAPS}


def e2e():
    mov2, fix2 = orc.golden_pair()
    seed = SEED_FROM
    while True:
        p = orc.make_weights(CHANNELS, mov2, fix2, seed)
        cond = {B: condition(p, mov2[:B], fix2[:B]) for B in (1, 2)}
        ok = all(g >= 100.0 * e for c in cond.values() for g, e in c.values())
        LINES.append("# weight seed %d: %s" % (seed, "meets the argmax condition" if ok else "does not meet the argmax condition"))
        if ok:
            break
        seed += 1
    assert seed == orc.GOLD_SEED, "tests/pcnet_oracle.py GOLD_SEED must be %d" % seed
    for B, c in cond.items():
        for k, (g, e) in c.items():
            LINES.append("gap[B%d] %s min (top1 - top2) / |top1| <TAB> ATen fp32 relative error\t%.6e\t%.6e" % (B, k, g, e))
    out = {"shape": np.array(SHAPE), "stride": np.array(STRIDE), "channels": np.array(CHANNELS), "seed": np.array(seed),
           "moving": mov2.numpy().reshape(-1)[::STRIDE].copy(), "fixed": fix2.numpy().reshape(-1)[::STRIDE].copy(),
           "pair_sum": np.array([float(mov2.double().sum()), float(fix2.double().sum())])}
    shapes = {"PCNet(%s, channels=%d)" % ("x".join(map(str, SHAPE)), CHANNELS): {k: list(v.shape) for k, v in ref.PCNet(SHAPE, channels=CHANNELS).state_dict().items()},
              "PCNet(16x16x16, channels=16)": {k: list(v.shape) for k, v in ref.PCNet((16, 16, 16)).state_dict().items()}}
    for B in (1, 2):
        m = reference(p, torch.float64)
        mov, fix = mov2[:B].double(), fix2[:B].double()
        moved, flow, pooled, fields = run_reference(m, mov, fix)
        loss = ncc_ref(fix, moved) + ref_losses.Grad3d(penalty="l2")(flow, fix)
        params = dict(m.named_parameters())
        assert sorted(params) == sorted(p)
        kept = sorted(n for n in params if golden_tensor(n))
        g_ref = dict(zip(kept, torch.autograd.grad(loss, [params[n] for n in kept])))
        taps = {}
        ol, omoved, oflow, og = orc.net_value_and_grads(p, mov, fix, torch.float64, taps)
        tag = "B%d" % B
        named = [("flow", oflow, flow), ("moved", omoved, moved), ("loss", ol, loss)]
        named += [(k, taps[k], v) for k, v in fields.items()] + [(k, taps[k], v) for k, v in pooled.items()]
        for name, o_, r_ in named:
            report("e2e[%s] %s" % (tag, name), o_, r_)
            if name != "loss" and not name.endswith(".cat"):
                out["%s.%s" % (tag, name)] = np.ascontiguousarray(r_.detach().numpy().reshape(-1)[::STRIDE])
                out["%s.%s_absmax" % (tag, name)] = np.array(float(r_.abs().max()))
        for k, w in fields.items():
            amax = float(w.abs().max())
            assert orc.FIELD_RANGE[0] <= amax <= orc.FIELD_RANGE[1], (tag, k, amax)
            LINES.append("range[%s] max|%s| (voxels, condition %g..%g)\t%.6e\t%.6e" % ((tag, k) + orc.FIELD_RANGE + (0.0, amax)))
        out[tag + ".loss"] = np.array([float(loss)])
        for n in kept:
            report("e2e[%s] grad %s" % (tag, n), og[n], g_ref[n])
            out["%s.grad.%s" % (tag, n)] = g_ref[n].detach().numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "e2e_pcnet_32x48x32.npz"), **out)
    with open(os.path.join(HERE, "pcnet_state_dict.json"), "w") as f:
        json.dump(shapes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    e2e()
    with open(os.path.join(HERE, "REPORT_pcnet.txt"), "w") as f:
        f.write("# tests/pcnet_oracle.py (fp64) against the reference's PCNet(channels = 4) in .double(), 32 x 48 x 32: "
                "quantity <TAB> max|oracle - reference| <TAB> max|reference|\n")
        f.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))
    for n in ("e2e_pcnet_32x48x32.npz", "pcnet_state_dict.json", "REPORT_pcnet.txt"):
        print(n, os.path.getsize(os.path.join(HERE, n)))
