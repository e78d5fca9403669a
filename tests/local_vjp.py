"""Host-only helper of the local-VJP tests: oracle.modet_torch.modet_forward + the train loss cut into SEGMENTS along the
oracle's taps.  One segment = one differentiable op of the path as the product runs it (an encoder group, a feature warp, a
projection pair, an attention, a CWM, a flow composition, the image warp, the loss).  For each segment: the fp64 input tensors
of the oracle's own run, one cotangent per output (d loss / d output of the full fp64 train loss as far as it arrives through
that output) and a closure that recomputes the segment from given inputs in their dtype.  With inputs AND cotangent taken from
the fp64 run a segment's vector-Jacobian product inherits nothing: its error against fp64 is the error this op adds.

Cotangents.  The oracle runs once, with its encoder's level features replaced by fresh leaves (what ModeT.stage_cuts and
test_stage_gradients_vs_oracle do): one backward pass from the loss gives the total gradient at every tensor behind the cut
and, at the leaves, the HEADS' share of d loss / d M_n, F_n; a second backward pass from the encoder's real outputs, seeded with
the leaves' gradients, gives the totals inside the encoder (at the pooled tensor entering a level, at the first block's output).
That is what an encoder group's three outputs receive in the product: features <- heads, pooled <- everything deeper.

Taps.  The cut needs the pooled tensor entering an encoder level (enc{M,F}.{lvl}.0), the final flow and y_moved from the
oracle; the upsampled 2 * flow entering a composition needs none, the upsampling being part of the composition's segment.

tests/test_cpu.py checks the cut by the chain rule (sum of the consumers' local VJPs == end-to-end autograd.grad, per cut
tensor and per parameter) and the coverage by name."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import modet_torch as orc

CWM_LEVELS = (3, 4, 5)
# oracle taps that lie INSIDE a segment (a group's first ConvInsBlock) and the ones that are another tap under a second name
INTERIOR_TAPS = tuple(f"enc{t}.{lvl}.1" for t in "MF" for lvl in range(5))


class Segment:
    """name; kind / level (what the HIP side dispatches on); inputs: name -> fp64 tensor (names are the cut tensors' canonical
    names, shared between the segments that consume one); scored: the inputs whose gradient is compared; params: name -> fp64
    tensor; cots: one fp64 cotangent per output; fn(inputs, params) -> tuple of outputs, in the dtype it is given; out_names"""

    def __init__(self, name, kind, level, inputs, scored, params, cots, fn, out_names):
        self.name, self.kind, self.level = name, kind, level
        self.inputs, self.scored, self.params, self.cots, self.fn, self.out_names = inputs, tuple(scored), params, list(cots), fn, out_names
        assert len(self.cots) == len(out_names)

    def rounded(self):
        """the same segment with inputs and cotangents rounded ONCE to fp32 (kept as fp32 tensors; every evaluation, fp64
        included, starts from these values, so input rounding is charged to nobody).  Parameters are fp32 values already."""
        return Segment(self.name, self.kind, self.level, {n: t.float() for n, t in self.inputs.items()}, self.scored, self.params,
                       [c.float() for c in self.cots], self.fn, self.out_names)

    def run(self, dtype, inputs=None, cots=None):
        """evaluate in ``dtype`` on the CPU: (outputs, {"d.<input>" / parameter name: gradient}) for the given inputs (default:
        the segment's own) under the given cotangents (default: the segment's own)"""
        src = self.inputs if inputs is None else inputs
        ins = {n: src[n].detach().to(dtype).requires_grad_(n in self.scored) for n in self.inputs}
        p = {n: t.detach().to(dtype).requires_grad_(True) for n, t in self.params.items()}
        outs = self.fn(ins, p)
        cts = [c.detach().to(dtype) for c in (self.cots if cots is None else cots)]
        names = ["d." + n for n in self.scored] + list(p)
        g = torch.autograd.grad(list(outs), [ins[n] for n in self.scored] + list(p.values()), cts)
        return [o.detach() for o in outs], {n: gi.detach() for n, gi in zip(names, g)}


def _conv_params(p, *blocks):
    return {f"{b}.{s}": p[f"{b}.{s}"] for b in blocks for s in (("main.weight", "main.bias") if not b.endswith("conv.2") else ("weight", "bias"))}


def oracle_taps(w, mov, fix, heads, head_dim, scale, cut=False):
    """one fp64 run of the oracle's forward + train loss with taps -> (p, taps, loss, real): ``cut``: the encoder's outputs
    are replaced by leaves (taps M_n / F_n are the leaves, ``real`` = {"M": [...], "F": [...]} the encoder's own outputs)"""
    p = {n: torch.as_tensor(v).double().requires_grad_(True) for n, v in w.items()}
    mov, fix = torch.as_tensor(mov).double(), torch.as_tensor(fix).double()
    taps, real, enc = {}, {}, orc.encoder

    def cut_encoder(p_, x, taps_=None, tag=""):
        real[tag] = enc(p_, x, taps_, tag)
        return [o.detach().requires_grad_(True) for o in real[tag]]
    if cut:
        orc.encoder = cut_encoder
    try:
        y, flow = orc.modet_forward(p, mov, fix, tuple(heads), head_dim, scale, taps=taps)
    finally:
        orc.encoder = enc
    loss = orc.ncc_loss(fix, y) + orc.grad3d_loss(flow)
    return p, taps, loss, real


def segments(w, mov, fix, heads=(8, 4, 2, 1, 1), head_dim=6, scale=1.0):
    """the list of Segments of one case (w: name -> fp32 array, mov / fix: (B,1,D,H,W) arrays) and the fp64 loss"""
    heads = tuple(heads)
    sc = scale if scale else head_dim ** -0.5
    p, taps, loss, real = oracle_taps(w, mov, fix, heads, head_dim, scale, cut=True)
    mov, fix = torch.as_tensor(mov).double(), torch.as_tensor(fix).double()
    B = mov.shape[0]
    # ---- pass 1: from the loss to everything behind the cut
    behind = ["y_moved", "flow"] + [f"flow{n}" for n in (2, 3, 4, 5)] + [f"w{n}" for n in (1, 2, 3, 4)] + \
        [f"mdt{n}" for n in CWM_LEVELS] + [f"{s}{n}" for n in range(1, 6) for s in ("q", "k", "M", "F")] + [f"Mw{n}" for n in range(1, 5)]
    g = dict(zip(behind, torch.autograd.grad(loss, [taps[n] for n in behind], retain_graph=True)))
    g["mdt1"], g["mdt2"], g["w5"] = g["w1"], g["w2"], g["flow5"]
    # ---- pass 2: from the encoder's real outputs, seeded with the leaves' gradients, into the encoder
    inside = [f"enc{t}.{lvl}.0" for lvl in range(5) for t in "MF"]
    outs = [real[t][i] for i in range(5) for t in "MF"]
    seeds = [g[f"{t}{i + 1}"] for i in range(5) for t in "MF"]
    g.update(zip(inside, torch.autograd.grad(outs, [taps[n] for n in inside], seeds)))
    v = {n: t.detach() for n, t in taps.items()}
    pd = {n: t.detach() for n, t in p.items()}

    def cat(name):                                  # the [moving; fixed] batch of an encoder tap / of its gradient
        return torch.cat([v["encM." + name], v["encF." + name]], 0), torch.cat([g["encM." + name], g["encF." + name]], 0)

    segs = []

    def add(name, kind, level, inputs, scored, params, cots, fn, out_names):
        segs.append(Segment(name, kind, level, inputs, scored, params, [c.detach() for c in cots], fn, out_names))

    # ---- loss, image warp
    add("loss", "loss", 0, {"y_moved": v["y_moved"], "flow": v["flow"], "fixed": fix}, ("y_moved", "flow"), {}, [torch.ones((), dtype=torch.float64)],
        lambda i, q: (orc.ncc_loss(i["fixed"], i["y_moved"]) + orc.grad3d_loss(i["flow"]),), ("loss",))
    add("image_warp", "image_warp", 0, {"moving": mov, "flow": v["flow"]}, ("flow",), {}, [g["y_moved"]],
        lambda i, q: (orc.warp(i["moving"], i["flow"]),), ("y_moved",))
    # ---- per level, fine to coarse (the order the backward pass reaches them)
    for n in (1, 2, 3, 4, 5):
        h = heads[5 - n]
        if n <= 4:
            fin, wn, out = f"flow{n + 1}", f"w{n}", ("flow" if n == 1 else f"flow{n}")
            if n == 1:
                def comp(i, q, fin=fin, wn=wn):
                    return (orc.warp(i[fin], i[wn]) + i[wn],)
            elif n == 2:
                def comp(i, q, fin=fin, wn=wn):
                    return (orc.upsample2(2 * (orc.warp(i[fin], i[wn]) + i[wn])),)
            else:
                def comp(i, q, fin=fin, wn=wn):
                    return (orc.warp(orc.upsample2(2 * i[fin]), i[wn]) + i[wn],)
            add(f"compose{n}", "compose", n, {fin: v[fin], wn: v[wn]}, (fin, wn), {}, [g[out]], comp, (out,))
        if n in CWM_LEVELS:
            blocks = [f"cwm{n}.conv.{i}" for i in range(3)]
            add(f"cwm{n}", "cwm", n, {f"mdt{n}": v[f"mdt{n}"]}, (f"mdt{n}",), _conv_params(pd, *blocks), [g[f"w{n}"]],
                lambda i, q, n=n, h=h: (orc.cwm(q, f"cwm{n}", i[f"mdt{n}"], h),), (f"w{n}",))
        add(f"attention{n}", "attention", n, {f"q{n}": v[f"q{n}"], f"k{n}": v[f"k{n}"]}, (f"q{n}", f"k{n}"),
            {f"mdt{n}.rpb": pd[f"mdt{n}.rpb"]}, [g[f"mdt{n}"]],
            lambda i, q, n=n, h=h: (orc.mode_transformer(i[f"q{n}"], i[f"k{n}"], q[f"mdt{n}.rpb"], h, sc),), (f"mdt{n}",))
        mw = f"Mw{n}" if n <= 4 else "M5"
        pj = {f"projblock{n}.{s}": pd[f"projblock{n}.{s}"] for s in ("proj.weight", "proj.bias", "norm.weight", "norm.bias")}
        add(f"projection{n}", "projection", n, {f"F{n}": v[f"F{n}"], mw: v[mw]}, (f"F{n}", mw), pj, [g[f"q{n}"], g[f"k{n}"]],
            lambda i, q, n=n, mw=mw: (orc.projection(q, f"projblock{n}", i[f"F{n}"]), orc.projection(q, f"projblock{n}", i[mw])),
            (f"q{n}", f"k{n}"))
        if n <= 4:
            fin = f"flow{n + 1}"
            add(f"feature_warp{n}", "feature_warp", n, {f"M{n}": v[f"M{n}"], fin: v[fin]}, (f"M{n}", fin), {}, [g[f"Mw{n}"]],
                lambda i, q, n=n, fin=fin: (orc.warp(i[f"M{n}"], i[fin]),), (f"Mw{n}",))
    # ---- encoder, coarse to fine, moving and fixed as one batch of 2B, cut where Encoder.forward_pair cuts it
    x4, _ = cat("4.0")
    add("encoder4", "encoder_last", 4, {"enc.4.0": x4}, ("enc.4.0",), _conv_params(pd, "encoder.conv4.1", "encoder.conv4.2"),
        [torch.cat([g["M5"], g["F5"]], 0)],
        lambda i, q: (orc.conv_ins_block(q, "encoder.conv4.2", orc.conv_ins_block(q, "encoder.conv4.1", i["enc.4.0"])),), ("MF5",))
    for L in (3, 2, 1, 0):
        xin, _ = cat(f"{L}.0")
        _, gpool = cat(f"{L + 1}.0")

        def group(i, q, L=L):
            y = orc.conv_ins_block(q, f"encoder.conv{L}.2", orc.conv_ins_block(q, f"encoder.conv{L}.1", i[f"enc.{L}.0"]))
            return F.avg_pool3d(y, 2), y[:B], y[B:]
        add(f"encoder{L}", "encoder_group", L, {f"enc.{L}.0": xin}, (f"enc.{L}.0",),
            _conv_params(pd, f"encoder.conv{L}.1", f"encoder.conv{L}.2"), [gpool, g[f"M{L + 1}"], g[f"F{L + 1}"]], group,
            (f"enc.{L + 1}.0", f"M{L + 1}", f"F{L + 1}"))
    _, g00 = cat("0.0")
    add("encoder0.0", "encoder_first", 0, {"images": torch.cat([mov, fix], 0)}, (), _conv_params(pd, "encoder.conv0.0"), [g00],
        lambda i, q: (orc.conv_block(q, "encoder.conv0.0", i["images"]),), ("enc.0.0",))
    return segs, float(loss.detach())


def consumed_taps(segs):
    """the oracle tap names the segments' inputs stand for ("enc.L.0" = the [moving; fixed] batch of encM.L.0 and encF.L.0)"""
    out = set()
    for s in segs:
        for n in s.inputs:
            out.update((f"encM.{n[4:]}", f"encF.{n[4:]}") if n.startswith("enc.") else (n,))
    return out


# taps that are another tap's tensor under a second name (asserted by identity in tests/test_cpu.py) -> the name the segments use
ALIASES = {"mdt1": "w1", "mdt2": "w2", "w5": "flow5"}
ALIASES.update({f"enc{t}.{lvl}.2": f"{t}{lvl + 1}" for t in "MF" for lvl in range(5)})
