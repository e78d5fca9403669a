"""Golden vectors for the PR++ network, from the REAL reference ("Baseline methods/PR++/models.py" and losses.py) -- build
container only.

    python tests/golden/make_goldens_prpp.py <checkout of the reference>

Imports the reference files read-only (never copied, never shipped; Correlation3D's constructor calls .cuda(): mapped to a no-op
here, as make_goldens_corr3d.py does), runs PRNetplusplus(first_channel = 4) on the CPU in fp64 at 32 x 48 x 32 (a 4 x 6 x 4 grid
at 1/8), for B = 1 and B = 2, and writes
    tests/golden/e2e_prpp_32x48x32.npz    per run moved and flow (every STRIDE-th element), the loss NCC(moved) + Grad3d('l2')(flow)
                                          as the reference's train loop forms it, and the reference's gradients of every bias and
                                          of every weight tensor of at most SMALL numbers; those of at most MID numbers for B = 2
                                          only (fp64 gradients do not compress; the others are compared with the oracle, which
                                          the report ties to the reference); every STRIDE-th voxel of the seeded pair
    tests/golden/prpp_state_dict.json     the state-dict keys and shapes of PRNetplusplus(first_channel = 4) here and of the
                                          default width at 16^3, from the reference's own class
    tests/golden/REPORT_prpp.txt          max|oracle - reference| per output and per gradient (ALL parameters), max |w| per
                                          block, and per composition the share of samples with a corner outside the coarse grid
Weights: tests/prpp_oracle.py golden_weights (seeded, not stored); the seed is the first from SEED_FROM on for which the REFERENCE
alone -- forward hooks on its five blocks -- has every block's max |w| inside FIELD_RANGE (voxels of the block's own grid) AND
every composition's share of samples with a corner outside the coarse grid below SHARE_MAX (and above 0 somewhere), for B = 1 and
B = 2.  On the 8 x 12 x 8 grid of block 2 a sub-voxel field of random sign already puts about 1 - (7/8)(11/12)(7/8) = 30 % of the
samples across a face, so most seeds that meet the range miss the share: the report lists every seed tried.  The pair: smilecode_amd.synth.make_pair (seeded, not stored)."""
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
from tests import prpp_oracle as orc  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Baseline methods", "PR++", "models.py")):
    sys.exit("usage: make_goldens_prpp.py <checkout of the reference (ZAX130/SmileCode)>")
REF = os.path.join(sys.argv[1], "Baseline methods", "PR++") + os.sep
torch.Tensor.cuda = lambda self, *a, **k: self             # no GPU in the build container


def _load(name):
    spec = importlib.util.spec_from_file_location("prpp_ref_" + name, REF + name + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, ref_losses = _load("models"), _load("losses")
torch.set_num_threads(8)
LINES = []
SHAPE, STRIDE, CHANNELS, SEED_FROM = orc.GOLD_SHAPE, 211, orc.GOLD_CHANNELS, 31
SMALL, MID = 2048, 7000
SHARE_MAX = 0.25


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


def golden_tensor(n, numel, B):
    """the parameters whose reference gradient is stored (module docstring)"""
    return n.endswith(".bias") or numel <= SMALL or (B == 2 and numel <= MID)


def reference(p, dtype):
    m = ref.PRNetplusplus(SHAPE, first_channel=CHANNELS)
    sd = m.state_dict()
    for n, v in p.items():
        assert tuple(sd[n].shape) == tuple(v.shape), n
        sd[n] = v.float()
    m.load_state_dict(sd)
    m = m.to(dtype)
    for k in orc.LEVELS:
        blk = getattr(m, "prblock%d" % k)
        blk.corr.w = blk.corr.w.to(dtype)         # a plain attribute, not a buffer: .to() does not reach it
    return m


def run_reference(m, mov, fix):
    """-> (moved, flow, {level: the block's field w}) of one forward of the reference"""
    fields, hooks = {}, []
    for k in orc.LEVELS:
        hooks.append(getattr(m, "prblock%d" % k).register_forward_hook(lambda mod, inp, out, k=k: fields.__setitem__(k, out)))
    moved, flow = m(mov, fix)
    for h in hooks:
        h.remove()
    return moved, flow, fields


def coarse_shape(k):
    """the grid of the flow that block k's field is composed with: 1/8, 1/4, 1/2, 1 for k = 2 .. 5"""
    f = {2: 8, 3: 4, 4: 2, 5: 1}[k]
    return tuple(s // f for s in SHAPE)


def condition(p, mov, fix):
    """level -> (max |w|, share of the composition's samples with a corner outside) on the reference's own fp64 run"""
    with torch.no_grad():
        fields = run_reference(reference(p, torch.float64), mov.double(), fix.double())[2]
    return {k: (float(w.abs().max()), orc.outside_share(orc.to_cl(w), coarse_shape(k)) if k > 1 else 0.0) for k, w in fields.items()}


def e2e():
    mov2, fix2 = orc.golden_pair()
    seed = SEED_FROM
    while True:
        p = orc.make_weights(CHANNELS, mov2, fix2, seed)
        cond = {B: condition(p, mov2[:B], fix2[:B]) for B in (1, 2)}
        in_range = all(orc.FIELD_RANGE[0] <= a <= orc.FIELD_RANGE[1] for c in cond.values() for a, _ in c.values())
        worst = max(s for c in cond.values() for k, (_, s) in c.items() if k > 1)
        LINES.append("# weight seed %d: %s; largest outside share %.3f (%s %g)" % (
            seed, "meets the field range" if in_range else "does not meet the field range", worst,
            "below" if worst < SHARE_MAX else "not below", SHARE_MAX))
        if in_range and 0.0 < worst < SHARE_MAX:
            break
        seed += 1
    assert seed == orc.GOLD_SEED, "tests/prpp_oracle.py GOLD_SEED must be %d" % seed
    for B, c in cond.items():
        for k, (a, share) in c.items():
            LINES.append("range[B%d] max|w%d| (voxels of its own grid, condition %g..%g)\t%.6e\t%.6e" % ((B, k) + orc.FIELD_RANGE + (0.0, a)))
            if k > 1:
                LINES.append("outside[B%d] composition %d: share of samples with a corner outside the coarse grid %s\t%.6e\t%.6e"
                             % (B, k, "x".join(map(str, coarse_shape(k))), 0.0, share))
    shares = [s for c in cond.values() for k, (_, s) in c.items() if k > 1]
    assert max(shares) > 0.0 and max(shares) < SHARE_MAX, shares
    out = {"shape": np.array(SHAPE), "stride": np.array(STRIDE), "channels": np.array(CHANNELS), "seed": np.array(seed),
           "moving": mov2.numpy().reshape(-1)[::STRIDE].copy(), "fixed": fix2.numpy().reshape(-1)[::STRIDE].copy(),
           "pair_sum": np.array([float(mov2.double().sum()), float(fix2.double().sum())])}
    shapes = {"PRNetplusplus(%s, first_channel=%d)" % ("x".join(map(str, SHAPE)), CHANNELS):
              {k: list(v.shape) for k, v in ref.PRNetplusplus(SHAPE, first_channel=CHANNELS).state_dict().items()},
              "PRNetplusplus(16x16x16, first_channel=8)": {k: list(v.shape) for k, v in ref.PRNetplusplus((16, 16, 16)).state_dict().items()}}
    for B in (1, 2):
        m = reference(p, torch.float64)
        mov, fix = mov2[:B].double(), fix2[:B].double()
        moved, flow, fields = run_reference(m, mov, fix)
        loss = ncc_ref(moved, fix) + ref_losses.Grad3d(penalty="l2")(flow, fix)
        params = dict(m.named_parameters())
        assert sorted(params) == sorted(p)
        names = sorted(params)
        g_ref = dict(zip(names, torch.autograd.grad(loss, [params[n] for n in names])))
        taps = {}
        ol, omoved, oflow, og = orc.net_value_and_grads(p, mov, fix, torch.float64, taps)
        tag = "B%d" % B
        named = [("flow", oflow, flow), ("moved", omoved, moved), ("loss", ol, loss)] + [("w%d" % k, taps["w%d" % k], w) for k, w in fields.items()]
        for name, o_, r_ in named:
            report("e2e[%s] %s" % (tag, name), o_, r_)
            if name in ("flow", "moved"):
                out["%s.%s" % (tag, name)] = np.ascontiguousarray(r_.detach().numpy().reshape(-1)[::STRIDE])
                out["%s.%s_absmax" % (tag, name)] = np.array(float(r_.abs().max()))
        for k, w in fields.items():
            out["%s.w%d_absmax" % (tag, k)] = np.array(float(w.abs().max()))
        out[tag + ".loss"] = np.array([float(loss)])
        for n in names:
            report("e2e[%s] grad %s" % (tag, n), og[n], g_ref[n])
            if golden_tensor(n, g_ref[n].numel(), B):
                out["%s.grad.%s" % (tag, n)] = g_ref[n].detach().numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "e2e_prpp_32x48x32.npz"), **out)
    with open(os.path.join(HERE, "prpp_state_dict.json"), "w") as f:
        json.dump(shapes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    e2e()
    with open(os.path.join(HERE, "REPORT_prpp.txt"), "w") as f:
        f.write("# tests/prpp_oracle.py (fp64) against the reference's PRNetplusplus(first_channel = 4) in .double(), 32 x 48 x 32: "
                "quantity <TAB> max|oracle - reference| <TAB> max|reference|\n")
        f.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))
    for n in ("e2e_prpp_32x48x32.npz", "prpp_state_dict.json", "REPORT_prpp.txt"):
        print(n, os.path.getsize(os.path.join(HERE, n)))
