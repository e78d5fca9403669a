"""Golden vectors for the Im2Grid network and its positional-encoding layer, from the REAL reference
("Baseline methods/Im2Grid/models.py" and losses.py) -- build container only.

    python tests/golden/make_goldens_im2grid.py <checkout of the reference>

Imports the reference files read-only (never copied, never shipped), runs them on the CPU in fp64 on seeded inputs and writes
    tests/golden/op_posenc.npz               per case: inputs, y, d_W, d_b, d_alpha (pair and single form)
    tests/golden/op_posenc_dx.npz            per case: d_x of both uses (a file of its own: see op_posenc below)
    tests/golden/e2e_im2grid_32x48x32.npz    the seeded pair, y_moved, flow, loss and the gradients of the fifteen peblock tensors,
                                             for B = 1 and B = 2 (weights: tests/im2grid_oracle.py make_weights, NON-zero, alpha != 1)
    tests/golden/im2grid_state_dict.json     the reference's state-dict keys and shapes
    tests/golden/REPORT_im2grid.txt          max|oracle - reference| per quantity (tests/im2grid_oracle.py in fp64)
The reference forms its embedding in fp32 even in a .double() model (pos.type(torch.FloatTensor)); the oracle forms it in fp64.
Everything that depends on the embedding therefore deviates by about 1e-7 relative, not 1e-15: the report records it."""
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
from tests import im2grid_oracle as orc  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "Baseline methods", "Im2Grid", "models.py")):
    sys.exit("usage: make_goldens_im2grid.py <checkout of the reference (ZAX130/SmileCode)>")
REF = os.path.join(sys.argv[1], "Baseline methods", "Im2Grid") + os.sep


def _load(name):
    spec = importlib.util.spec_from_file_location("im2grid_ref_" + name, REF + name + ".py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref, ref_losses = _load("models"), _load("losses")
torch.set_num_threads(8)
LINES = []


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


# ----------------------------------------------------------------------------- the layer
CASES = (("b2_2x3x5_c8", 2, (2, 3, 5), 8), ("b1_7x6x19_c16", 1, (7, 6, 19), 16), ("b1_3x5x17_c32", 1, (3, 5, 17), 32),
         ("b2_4x7x9_c64", 2, (4, 7, 9), 64), ("b1_2x3x4_c128", 1, (2, 3, 4), 128))


def op_posenc():
    out = {}
    for tag, B, shape, Cin in CASES:
        rng = np.random.default_rng(500 + Cin)
        f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))      # noqa: E731  (the fixture stores fp32 inputs)
        x1, x2 = (f32(rng.standard_normal((B,) + shape + (Cin,))) for _ in range(2))
        gy1, gy2 = (f32(rng.standard_normal((B,) + shape + (6,))) for _ in range(2))
        Wt = f32(rng.standard_normal((6, Cin)) / np.sqrt(Cin))
        b, alpha = f32(rng.standard_normal(6) * 0.3), f32([0.75 + 0.01 * Cin])
        layer = ref.PositionalEncodingLayer(Cin).double()
        with torch.no_grad():
            layer.proj.weight.copy_(Wt)
            layer.proj.bias.copy_(b)
            layer.alpha.copy_(alpha)
        prm = [layer.proj.weight, layer.proj.bias, layer.alpha]
        a1, a2 = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
        y1, y2 = layer(a1.permute(0, 4, 1, 2, 3)), layer(a2.permute(0, 4, 1, 2, 3))         # the reference takes (B,C,H,W,T)
        dx1, dW1, db1, da1 = torch.autograd.grad(y1, [a1] + prm, gy1.double(), retain_graph=True)
        dx2, dW2, db2, da2 = torch.autograd.grad(y2, [a2] + prm, gy2.double())
        # the oracle on the same numbers
        o = [t.double().requires_grad_(True) for t in (x1, x2, Wt, b, alpha)]
        oy1, oy2 = orc.posenc_cl(o[0], o[2], o[3], o[4]), orc.posenc_cl(o[1], o[2], o[3], o[4])
        og = torch.autograd.grad([oy1, oy2], o, [gy1.double(), gy2.double()])
        for name, got, want in (("y", torch.stack((oy1, oy2)), torch.stack((y1, y2))), ("d_x", torch.stack(og[:2]), torch.stack((dx1, dx2))),
                                ("d_W", og[2], dW1 + dW2), ("d_b", og[3], db1 + db2), ("d_alpha", og[4], da1 + da2)):
            report("op[%s] %s" % (tag, name), got, want)
        for n, v in (("x1", x1), ("x2", x2), ("gy1", gy1), ("gy2", gy2), ("Wt", Wt), ("b", b), ("alpha", alpha)):
            out["%s.%s" % (tag, n)] = v.numpy()
        for n, v in (("y1", y1), ("y2", y2), ("dx1", dx1), ("dx2", dx2), ("dW", dW1 + dW2), ("db", db1 + db2), ("dalpha", da1 + da2),
                     ("dW_single", dW1), ("db_single", db1), ("dalpha_single", da1)):
            out["%s.%s" % (tag, n)] = v.detach().numpy().astype(np.float64)
    # two files: the fp64 data gradients alone are 0.9 MB of incompressible numbers, and a committed file stays below 1 MiB
    is_dx = lambda k: k.endswith(".dx1") or k.endswith(".dx2")      # noqa: E731
    np.savez_compressed(os.path.join(HERE, "op_posenc.npz"), **{k: v for k, v in out.items() if not is_dx(k)})
    np.savez_compressed(os.path.join(HERE, "op_posenc_dx.npz"), **{k: v for k, v in out.items() if is_dx(k)})


# ----------------------------------------------------------------------------- end to end
SHAPE, STRIDE, PAIR_SEED = (32, 48, 32), 11, 24


def e2e():
    p = orc.make_weights()
    mov2, fix2 = (torch.from_numpy(a) for a in synth.make_pair(SHAPE, PAIR_SEED, batch=2))
    out = {"shape": np.array(SHAPE), "stride": np.array(STRIDE), "moving": mov2.numpy(), "fixed": fix2.numpy()}
    for n, v in p.items():
        if n.startswith("peblock"):
            out["weight." + n] = v.float().numpy()
    out["weights_seed"] = np.array(7)
    sd_shapes = None
    for B in (1, 2):
        m = ref.Im2grid(SHAPE)
        if sd_shapes is None:
            sd_shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
        sd = m.state_dict()
        for n, v in p.items():
            assert tuple(sd[n].shape) == tuple(v.shape), n
            sd[n] = v.float()
        m.load_state_dict(sd)
        m = m.double()
        mov, fix = mov2[:B].double(), fix2[:B].double()
        y_ref, f_ref = m(mov, fix)
        sim, reg = ncc_ref(fix, y_ref), ref_losses.Grad3d(penalty="l2")(f_ref, fix)
        loss = sim + reg
        params = dict(m.named_parameters())
        small = sorted(n for n in params if n.startswith("peblock"))
        g_ref = dict(zip(small, torch.autograd.grad(loss, [params[n] for n in small])))
        ol, osim, oreg, oy, oflow, og = orc.value_and_grads(p, mov, fix, torch.float64)
        tag = "B%d" % B
        report("e2e[%s] flow" % tag, oflow, f_ref)
        report("e2e[%s] y_moved" % tag, oy, y_ref)
        report("e2e[%s] loss" % tag, ol, loss)
        out[tag + ".flow"] = np.ascontiguousarray(f_ref.detach().numpy().reshape(-1)[::STRIDE])
        out[tag + ".y_moved"] = np.ascontiguousarray(y_ref.detach().numpy().reshape(-1)[::STRIDE])
        out[tag + ".flow_absmax"] = np.array(float(f_ref.abs().max()))
        out[tag + ".y_absmax"] = np.array(float(y_ref.abs().max()))
        out[tag + ".loss"] = np.array([float(loss), float(sim), float(reg)])
        for n in small:
            report("e2e[%s] grad %s" % (tag, n), og[n], g_ref[n])
            out["%s.grad.%s" % (tag, n)] = g_ref[n].detach().numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "e2e_im2grid_32x48x32.npz"), **out)
    with open(os.path.join(HERE, "im2grid_state_dict.json"), "w") as f:
        json.dump(sd_shapes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    op_posenc()
    e2e()
    with open(os.path.join(HERE, "REPORT_im2grid.txt"), "w") as f:
        f.write("# tests/im2grid_oracle.py (fp64) against the reference's Im2Grid in .double(): quantity <TAB> max|oracle - reference| "
                "<TAB> max|reference|\n"
                "# The reference forms its position embedding in fp32 even here (pos.type(torch.FloatTensor)), the oracle in fp64: y, "
                "d_alpha and everything\n# end to end carry that ~1e-7 relative deviation; d_x, d_W and d_b do not depend on the "
                "embedding and agree to fp64 rounding.\n")
        f.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))
    for n in ("op_posenc.npz", "op_posenc_dx.npz", "e2e_im2grid_32x48x32.npz", "im2grid_state_dict.json", "REPORT_im2grid.txt"):
        print(n, os.path.getsize(os.path.join(HERE, n)))
