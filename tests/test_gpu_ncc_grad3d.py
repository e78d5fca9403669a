"""-m gpu: NCC (the z-march kernels of windows 3 / 5 / 7 / 9 and the general box path) and Grad3d (l1 / l2, planar and
channels-last) of csrc/losses.hip against fp64, per op: the two loss terms of every benchmarked step.

The parity bound is not a chosen number (as in tests/test_gpu_ssim.py): every case is also evaluated with oracle/modet_torch.py
in fp32 on the CPU, the ATen composition (five dense all-ones conv3d for NCC, sliced differences for Grad3d), whose own error
against fp64 is measured; the HIP result has to stay within A = 4 times the LARGEST such error over its group's cases, per
quantity -- loss: relative (and never below 2^-23, one ulp of the stored fp32 scalar, which ATen can hit exactly on a whole group
by luck); gradients: max|g - g64| over all voxels / max|g64|.  The groups: ``ncc_march`` (cubic windows 3, 5, 7, 9), ``ncc_box``
(every other window), ``grad3d``.  The errors of every case and the bounds are in the report.

The fp64 reference is the dense oracle on the same fp32-rounded inputs, the reference's recorded results for the windows of
tests/golden/op_ncc_windows.npz, and for the two plan* volumes (2.0 M and 4.4 M voxels, too large for 729-tap convolutions in a
test) the separable restatement of tests/ncc_oracle.py, which tests/test_cpu_ncc.py holds to the dense oracle; those two add no
ATen sample and are asserted against the group's bound like every other case.  tests/ncc_oracle.py lists the z-march cases with
what each reaches: ragged tiles in both directions, exact tiles, several z chunks with a short last one, chunks longer than the
window (the ring's replacement order when zc != win), axes shorter than the half-window, batch offsets, the benchmark's synthetic
pairs (two thirds exact zeros: cc is a small number over the 1e-5 epsilon) and unnormalised intensities.  The Grad3d shapes
include two above 524 288 elements, where the kernel's grid of 2048 workgroups starts to loop."""
import functools

import numpy as np
import pytest
import torch

from oracle import modet_torch as orc
from tests import ncc_oracle
from tests.util import gold, note_many

pytestmark = pytest.mark.gpu

A = 4.0
ULP = 2.0 ** -23
SCALE = 0.37
NCC_Q = ("loss", "grad_true", "grad_pred")
G3D_Q = ("loss", "grad")
GROUPS = {"ncc_march": NCC_Q, "ncc_box": NCC_Q, "grad3d": G3D_Q}
# a measured quantity that is held to another quantity's bound
BASE = {"grad_pred_scaled": "grad_pred", "loss_cl": "loss", "grad_cl": "grad", "grad_cl_scaled": "grad"}

BOX_GOLDEN = ([4, 4, 4], [5, 3, 7], [11, 11, 11], [2, 6, 3], [6, 9, 9], [9, 9, 5], [1, 1, 1])
BOX_SYNTH = {"pair13x27x35": ([4, 4, 4], [5, 3, 7], [11, 11, 11]), "noise40x80x100": ([4, 4, 4], [2, 6, 3])}
G3D_SHAPES = (((1, 3, 2, 2, 2), ("l1", "l2")), ((2, 3, 7, 9, 11), ("l1", "l2")), ((2, 3, 12, 20, 28), ("l1", "l2")),
              ((1, 3, 3, 2, 65), ("l1", "l2")), ((1, 3, 57, 56, 58), ("l1", "l2")), ((2, 3, 40, 48, 50), ("l2",)))
# The one case whose fp64 value and gradients are exactly 0: with a window of one voxel every "sum" is the voxel itself, the
# variances and the covariance cancel exactly in any precision (the reference's and ATen fp32's results are exact zeros), and
# only exact zeros are within a relative bound.  Every other case must have a reference that is not zero.
ZERO_REFERENCE = ("ncc[golden14x22x19_B2.1x1x1]",)
G3D_LOOP = 2048 * 256                        # grad3d_kernel's grid cap x its workgroup: more elements than this and threads loop


def _wtag(w):
    return "w%d" % w if isinstance(w, int) else "x".join(map(str, w))


def _ratio(err, top):
    """err / top; against a reference that is exactly 0 only an exact 0 is within a relative bound (ZERO_REFERENCE)"""
    return 0.0 if err == 0.0 else (err / top if top > 0.0 else float("inf"))


def _rel(got, ref):
    """max|got - ref| / max|ref|"""
    return _ratio(float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max()), float(ref.abs().max()))


def _ncc_errors(loss, da, db, ref):
    l64, da64, db64 = ref
    return {"loss": _ratio(abs(float(loss.detach()) - float(l64)), abs(float(l64))), "grad_true": _rel(da, da64), "grad_pred": _rel(db, db64)}


def _ncc_hip(fn, a, b, w, ref, march):
    """the HIP errors of one (volumes, window) and the names of the bit identities that do not hold"""
    from smilecode_amd import ops
    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    a0, b0 = ad.detach(), bd.detach()
    loss = fn(ad, bd, w)
    da, db = torch.autograd.grad(loss, [ad, bd])
    assert loss.shape == () and da.shape == a.shape and db.shape == b.shape
    hip, off = _ncc_errors(loss, da, db, ref), []
    if not all(bool(torch.isfinite(t).all()) for t in (loss, da, db)):
        off.append("finite")

    def same(name, *pairs):
        if not all(torch.equal(x, y) for x, y in pairs):
            off.append(name)

    # each argument alone and neither: the same value bits, the same gradient bits
    l_a = fn(ad, b0, w)
    (da1,) = torch.autograd.grad(l_a, [ad])
    l_b = fn(a0, bd, w)
    (db1,) = torch.autograd.grad(l_b, [bd])
    same("value, y_true alone", (l_a, loss))
    same("value, y_pred alone", (l_b, loss))
    same("value, no gradient", (fn(a0, b0, w), loss))
    same("d y_true alone", (da1, da))
    same("d y_pred alone", (db1, db))
    l2 = fn(ad, bd, w)
    same("second evaluation", (l2, loss), *zip(torch.autograd.grad(l2, [ad, bd]), (da, db)))
    if march:
        l1, g1 = ops.ncc_value_and_grad(a0, b0, w, 1.0)
        same("ncc_value_and_grad at weight 1", (l1, loss), (g1, db))
        ls, gs = ops.ncc_value_and_grad(a0, b0, w, SCALE)                 # the term's weight scales the gradient, not the value
        same("ncc_value_and_grad value at weight 0.37", (ls, loss))
        hip["grad_pred_scaled"] = _rel(gs, SCALE * ref[2])
    return hip, off


def _march(out):
    from smilecode_amd import ops
    for tag in ncc_oracle.MARCH_CASES:
        a, b, windows, dense = ncc_oracle.march_inputs(tag)
        for w in windows:
            ref = ncc_oracle.value_and_grads(orc.ncc_loss if dense else ncc_oracle.ncc_loss, a, b, torch.float64, win=w)
            aten = _ncc_errors(*ncc_oracle.value_and_grads(orc.ncc_loss, a, b, torch.float32, win=w), ref) if dense else None
            hip, off = _ncc_hip(ops.ncc_loss, a, b, w, ref, True)
            out["ncc_march"][f"ncc[{tag}.{_wtag(w)}]"] = {"aten": aten, "hip": hip, "off": off, "ref_top": [float(r.abs().max()) for r in ref]}


def _box_inputs(tag):
    if tag == "noise40x80x100":
        return ncc_oracle.noise_pair((40, 80, 100), 1)
    a, b, _, _ = ncc_oracle.march_inputs(tag)
    return a, b


def _box(out):
    from smilecode_amd import losses

    def fn(a, b, w):
        return losses.NCC_vxm(win=w)(a, b)

    g = gold("op_ncc_windows.npz")
    cases = []
    for w in BOX_GOLDEN:
        k = "ncc[%s]" % _wtag(w)
        a, b = torch.from_numpy(g[k + ".a"]), torch.from_numpy(g[k + ".b"])
        assert a.dtype == torch.float32 and tuple(a.shape) == (2, 1, 14, 22, 19)
        ref = tuple(torch.from_numpy(np.ascontiguousarray(g[f"{k}.{q}"])).double() for q in ("val", "da", "db"))
        cases.append(("golden14x22x19_B2", a, b, w, ref))
    for tag, windows in BOX_SYNTH.items():
        a, b = _box_inputs(tag)
        cases += [(tag, a, b, w, ncc_oracle.value_and_grads(orc.ncc_loss, a, b, torch.float64, win=w)) for w in windows]
    for tag, a, b, w, ref in cases:
        aten = _ncc_errors(*ncc_oracle.value_and_grads(orc.ncc_loss, a, b, torch.float32, win=w), ref)
        hip, off = _ncc_hip(fn, a, b, w, ref, False)
        out["ncc_box"][f"ncc[{tag}.{_wtag(w)}]"] = {"aten": aten, "hip": hip, "off": off, "ref_top": [float(r.abs().max()) for r in ref]}


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _flows():
    """(tag, planar flow on the host, penalties): standard normal flows, and one smooth flow of amplitude 0.5"""
    for shape, pens in G3D_SHAPES:
        gen = torch.Generator().manual_seed(sum(shape))
        yield "randn" + "x".join(map(str, shape)), torch.randn(shape, generator=gen), pens
    z, y, x = torch.meshgrid(torch.arange(12.0), torch.arange(20.0), torch.arange(28.0), indexing="ij")
    smooth = torch.stack([torch.stack([0.5 * torch.sin(0.31 * x + 0.7 * c + n) * torch.cos(0.23 * y - 0.4 * c) * torch.cos(0.45 * z + 0.17 * x + c)
                                       for c in range(3)]) for n in range(2)])
    yield "smooth2x3x12x20x28", smooth.float().contiguous(), ("l1", "l2")


def _g3d_errors(loss, grad, ref):
    l64, g64 = ref
    return {"loss": _ratio(abs(float(loss.detach()) - float(l64)), abs(float(l64))), "grad": _rel(grad, g64)}


def _g3d_oracle(f, pen, dtype):
    f = f.detach().cpu().to(dtype).requires_grad_(True)
    loss = orc.grad3d_loss(f, pen)
    return loss.detach(), torch.autograd.grad(loss, [f])[0]


def _grad3d(out):
    from smilecode_amd import ops
    for tag, f, pens in _flows():
        for pen in pens:
            ref = _g3d_oracle(f, pen, torch.float64)
            aten = _g3d_errors(*_g3d_oracle(f, pen, torch.float32), ref)
            fd = f.cuda().requires_grad_(True)
            loss = ops.grad3d_loss(fd, pen)
            (grad,) = torch.autograd.grad(loss, [fd])
            assert loss.shape == () and grad.shape == f.shape
            hip, off = _g3d_errors(loss, grad, ref), []
            f_cl = _cl(fd.detach())
            l_cl, g_cl = ops.grad3d_value_and_grad_cl(f_cl, pen, 1.0)
            l_s, g_s = ops.grad3d_value_and_grad_cl(f_cl, pen, SCALE)
            assert g_cl.shape == f_cl.shape == g_s.shape
            hip["loss_cl"] = _g3d_errors(l_cl, g_cl.permute(0, 4, 1, 2, 3), ref)["loss"]
            hip["grad_cl"] = _rel(g_cl.permute(0, 4, 1, 2, 3), ref[1])
            hip["grad_cl_scaled"] = _rel(g_s.permute(0, 4, 1, 2, 3), SCALE * ref[1])
            l2 = ops.grad3d_loss(fd, pen)
            (grad2,) = torch.autograd.grad(l2, [fd])
            l_cl2, g_cl2 = ops.grad3d_value_and_grad_cl(f_cl, pen, 1.0)
            for name, ok in (("channels-last gradient == planar", torch.equal(g_cl.permute(0, 4, 1, 2, 3), grad)),
                             ("channels-last value == planar", torch.equal(l_cl, loss)),
                             ("value at weight 0.37", torch.equal(l_s, loss)),
                             ("value, no gradient", torch.equal(ops.grad3d_loss(fd.detach(), pen), loss)),
                             ("second evaluation, planar", torch.equal(l2, loss) and torch.equal(grad2, grad)),
                             ("second evaluation, channels-last", torch.equal(l_cl2, l_cl) and torch.equal(g_cl2, g_cl))):
                if not ok:
                    off.append(name)
            out["grad3d"][f"grad3d[{tag}.{pen}]"] = {"aten": aten, "hip": hip, "off": off, "ref_top": [float(r.abs().max()) for r in ref]}


@functools.lru_cache(maxsize=None)
def _run():
    try:
        return _measure()
    except BaseException as e:                  # measured once: the tests that follow fail with the same error, at once
        return e


def _measured():
    m = _run()
    if isinstance(m, BaseException):
        raise m
    return m


def _measure():
    """group -> case -> {"aten": errors of ATen fp32 on the CPU (None: no sample), "hip": errors of the HIP path, "off": the bit
    identities that do not hold}, errors against fp64: loss relative, gradients max|err| over all voxels / max|g64|"""
    out = {g: {} for g in GROUPS}
    _march(out)
    _box(out)
    _grad3d(out)
    rep = {}
    for cases in out.values():
        for key, r in cases.items():
            for who in ("aten", "hip"):
                for q, v in (r[who] or {}).items():
                    rep[f"{key}.{q}.e_{who}"] = v if np.isfinite(v) else 1e30
                    print(f"{key} {q}: {who} {v:.3e}")
    note_many(rep)
    return out


def _bound(group, quantity):
    worst = max(r["aten"][quantity] for r in _measured()[group].values() if r["aten"] is not None)
    return max(A * worst, ULP) if quantity == "loss" else A * worst


def test_every_case_of_the_tables_is_measured():
    m = _measured()
    assert len(m["ncc_march"]) == 21 and sum(r["aten"] is None for r in m["ncc_march"].values()) == 2
    assert len(m["ncc_box"]) == 7 + 3 + 2 and len(m["grad3d"]) == 5 * 2 + 1 + 2
    assert all(r["aten"] is not None for g in ("ncc_box", "grad3d") for r in m[g].values())
    for w in (3, 5, 7, 9):
        assert sum(k.endswith(".w%d]" % w) for k in m["ncc_march"]) >= 3, w
    looping = [f for _, f, _ in _flows() if f.numel() > G3D_LOOP]
    assert [tuple(f.shape) for f in looping] == [(1, 3, 57, 56, 58), (2, 3, 40, 48, 50)]
    assert 40 * 80 * 100 > 1024 * 256                    # ncc_cc_kernel's grid cap x its workgroup
    # no reference is zero (a relative error would say nothing), but for the one-voxel window, where all of it is
    zero = sorted(k for cases in m.values() for k, r in cases.items() if min(r["ref_top"]) == 0.0)
    assert zero == sorted(ZERO_REFERENCE) and all(max(m["ncc_box"][k]["ref_top"]) == 0.0 for k in zero)


@pytest.mark.parametrize("group,quantity", [(g, q) for g, qs in GROUPS.items() for q in qs])
def test_parity_with_fp64_within_four_times_aten_fp32(group, quantity):
    m = _measured()[group]
    bound = _bound(group, quantity)
    note_many({f"{group}.bound.{quantity}": bound})
    print(f"{group}: bound for {quantity}: {bound:.3e}")
    assert 0.0 < bound < float("inf")
    seen = {(k, q): v for k, r in m.items() for q, v in r["hip"].items() if BASE.get(q, q) == quantity}
    assert len(seen) >= len(m)
    worst = max(seen, key=seen.get)
    note_many({f"{group}.worst_e_hip.{quantity}": seen[worst]})
    print(f"{group}: HIP's worst {quantity}: {seen[worst]:.3e} ({worst[0]} {worst[1]})")
    bad = {k: v for k, v in seen.items() if not v <= bound}
    assert not bad, f"{group} {quantity}: HIP error beyond {A:g} x the largest ATen fp32 error ({bound:.3e}): {bad}"


@pytest.mark.parametrize("group", list(GROUPS))
def test_values_and_gradients_are_the_same_bits_however_they_are_asked_for(group):
    """NCC: both arguments, either one or neither requiring a gradient, a second evaluation, and ops.ncc_value_and_grad (its
    gradient at weight 1; its value at any weight).  Grad3d: planar against channels-last, with and without a gradient, a second
    evaluation, the value at any weight"""
    off = {k: r["off"] for k, r in _measured()[group].items() if r["off"]}
    assert not off, off


@pytest.mark.parametrize("shape", [(1, 3, 2, 2, 2), (2, 3, 7, 9, 11)])
def test_zero_flow_has_no_loss_and_no_gradient(shape):
    from smilecode_amd import ops
    for pen in ("l1", "l2"):
        f = torch.zeros(shape, device="cuda").requires_grad_(True)
        loss = ops.grad3d_loss(f, pen)
        (grad,) = torch.autograd.grad(loss, [f])
        l_cl, g_cl = ops.grad3d_value_and_grad_cl(_cl(f.detach()), pen, 1.0)
        for l, g in ((loss, grad), (l_cl, g_cl)):
            assert float(l.detach()) == 0.0 and g.numel() == f.numel() and not bool(g.any()), pen
