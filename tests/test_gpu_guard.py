"""-m gpu: WHERE the kernels read and write (the parity tests pin WHAT they compute).  Every caller-supplied tensor sits between
guard bands (tests/guard.py), every allocation of the package is guarded and poisoned, and the library is reached through a
recording proxy.  Per case: no band is damaged (an out-of-bounds write), every floating result is finite (an out-of-bounds or
uninitialised read whose value is used becomes NaN), the results equal an unguarded run, and a second guarded run whose bands
and poison are 0x00 instead of 0xFF gives the same bits (a stray read that a comparison or a select swallowed).

No tolerance here is tuned: comparisons are bit-equality, except the ops of ATOMIC below, whose d_src is scattered with float
atomics; those reuse the tolerance of the existing test named beside them."""
import contextlib
import ctypes

import pytest
import torch

from tests import guard
from tests.guard_family import Maker
from tests.util import note_many

pytestmark = pytest.mark.gpu

SEEN = {"a": [], "b": [], "c": [], "e": []}   # section -> the proxies' (entry point, [class of each pointer argument]) records
RAN = set()                                   # (section, case) whose guarded run is in SEEN: the coverage test runs the rest itself

# The float-atomic scatter (csrc/warp.hip scatter_add: atomicAdd(float*)) is the library's only order-dependent sum: reached by
# modet_warp_bwd and modet_warp_bwd_acc when they produce d_src.  result name -> (relative tolerance of max|ref|, its origin)
ATOMIC = {
    "warp_atomic.d_src": (2e-6, "test_warp_backward_deterministic_mode / test_warp_backward_by_destination_tiles: 2e-6 of max"),
}


@pytest.fixture
def px(monkeypatch):
    from smilecode_amd import _lib
    p = guard.LibProxy(_lib.load())
    monkeypatch.setattr(_lib, "_lib", p)
    guard.release()
    yield p
    guard.release()
    torch.cuda.empty_cache()


def G(seed):
    return torch.Generator().manual_seed(seed)


def R(gen, *shape, s=1.0):
    return torch.randn(*shape, generator=gen) * s


def _run(case, mode, px, section):
    """one run of a case (a generator function of ``g``, the function that puts a host tensor on the GPU: it yields a dict of
    results after the forward and one after the backward).  mode None: plain tensors and allocations; 0xFF / 0x00: everything
    guarded with that canary, bands checked at every yield."""
    g, ctx = Maker(mode), (contextlib.nullcontext() if mode is None else guard.GuardedAlloc(canary=mode))
    n0, outs = len(px.records), {}
    with ctx:
        for stage, named in enumerate(case(g)):
            torch.cuda.synchronize()
            if mode is not None:
                bands = guard.check()
                assert not bands, "after %s: %s" % (("the forward", "the backward")[min(stage, 1)], guard.describe(bands))
            for k, v in named.items():
                if v is not None:
                    assert k not in outs
                    outs[k] = v.detach().clone()
    if mode == 0xFF:
        SEEN[section].extend(px.records[n0:])
    del px.records[n0:]
    guard.release()
    return outs


def _same(a, b, what, tag):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        tol = ATOMIC.get(tag + "." + k)
        if tol is None:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), "%s: %s differs (%s): max |diff| %.3e" % (
                tag, k, what, float((a[k].double() - b[k].double()).abs().max()))
        else:
            err, ref = float((a[k] - b[k]).abs().max()), float(b[k].abs().max())
            assert err <= tol[0] * ref, "%s: %s differs (%s) beyond the float-atomic noise: %.3e of max" % (tag, k, what, err / ref)


def run_guarded(case, px, tag, section="a"):
    """the four assertions of a case; returns the guarded results"""
    plain = _run(case, None, px, section)
    first = _run(case, 0xFF, px, section)
    for k, v in first.items():
        if v.dtype.is_floating_point:
            assert bool(torch.isfinite(v).all()), "%s: %s is not finite in the guarded run (a read of a band or of poison)" % (tag, k)
    _same(first, plain, "guarded vs unguarded", tag)
    second = _run(case, 0x00, px, section)
    _same(second, first, "0x00 vs 0xFF bands and poison", tag)
    return first


def _grads(outs, inputs, cots):
    """torch.autograd.grad over the inputs that want one -> {d_<name>: grad}"""
    names = [n for n, t in inputs.items() if t is not None and t.requires_grad]
    gs = torch.autograd.grad(outs, [inputs[n] for n in names], cots, allow_unused=True)
    return {"d_" + n: gi for n, gi in zip(names, gs)}


# ------------------------------------------------------------------------------------------------ (a) the per-op table
def _ops():
    from smilecode_amd import ops
    return ops


def conv_case(cin, cout, shape, B, form="conv", act=False, x_act=False, x_grad=True, xs=1.0):
    """form: conv (ops.conv3d) | stats (conv3d_with_stats) | ins (conv3d_instnorm_lrelu)"""
    def case(g):
        ops, gen = _ops(), G(3)
        x = g(R(gen, B, *shape, cin, s=xs)).requires_grad_(x_grad)
        w = g(R(gen, cout, cin, 3, 3, 3, s=0.2)).requires_grad_(True)
        b = g(R(gen, cout)).requires_grad_(True)
        if form == "conv":
            y, st = ops.conv3d(x, w, b, act, x_act), None
        elif form == "stats":
            y, st = ops.conv3d_with_stats(x, w, b, x_act)
        else:
            y, st = ops.conv3d_instnorm_lrelu(x, w, b, 1e-5, x_act), None
        yield {"y": y, "stats": st}
        yield _grads([y], {"x": x, "w": w, "b": b}, [g(R(gen, *y.shape))])
    return case


def raw_conv_case(cin, cout, shape, B):
    """the raw calls: conv3d_forward, conv3d_backward_data (with and without max |d_y|), conv3d_backward_weight (plain, y_act, amax)"""
    def case(g):
        ops, gen = _ops(), G(4)
        x = g(R(gen, B, *shape, cin))
        w, b = g(R(gen, cout, cin, 3, 3, 3, s=0.2)), g(R(gen, cout))
        y = ops.conv3d_forward(x, w, b, True)
        y2 = ops.conv3d_forward(x, w, None, False, x_act=True)
        yield {"y": y, "y2": y2}
        dy = g(R(gen, *y.shape))
        amax = g(dy.abs().max().reshape(1).expand(ops.AMAX_FLOATS).contiguous())
        out = {"dx": ops.conv3d_backward_data(dy, w, cin), "dx_amax": ops.conv3d_backward_data(dy, w, cin, amax=amax)}
        out["dw"], out["db"] = ops.conv3d_backward_weight(x, dy, True)
        out["dw_nb"], _ = ops.conv3d_backward_weight(x, dy, False)
        if (cin, cout) == (1, 4):                     # (the only configuration with the fused LeakyReLU' form: the first encoder block)
            out["dw_act"], out["db_act"] = ops.conv3d_backward_weight(x, dy, True, y_act=y)
        out["dw_amax"], out["db_amax"] = ops.conv3d_backward_weight(x, dy, True, amax=amax)
        yield out
    return case


def chain_case(c0, c1, c2, shape, B, grad=True, want_stats=True):
    """conv3d_with_stats -> lazy_instnorm_conv3d (-> instnorm_stats + conv3d_forward_normin without gradients)"""
    def case(g):
        ops, gen = _ops(), G(5)
        x = g(R(gen, B, *shape, c0)).requires_grad_(grad)
        p = [g(t).requires_grad_(grad) for t in (R(gen, c1, c0, 3, 3, 3, s=0.2), R(gen, c1), R(gen, c2, c1, 3, 3, 3, s=0.2), R(gen, c2))]
        with (contextlib.nullcontext() if grad else torch.no_grad()):
            raw, st = ops.conv3d_with_stats(x, p[0], p[1])
            z, zst = ops.lazy_instnorm_conv3d(raw, st, p[2], p[3], want_stats=want_stats)
        with torch.no_grad():                                          # (no epilogue statistics: one statistics pass)
            z2, _ = ops.lazy_instnorm_conv3d(raw.detach(), None, p[2].detach(), p[3].detach(), want_stats=False)
        yield {"raw": raw, "st": st, "z": z, "zst": zst, "z2": z2}
        if grad:
            yield _grads([z], {"x": x, "w1": p[0], "b1": p[1], "w2": p[2], "b2": p[3]}, [g(R(gen, *z.shape))])
    return case


def normin_case(cin, cout, shape, B):
    def case(g):
        ops, gen = _ops(), G(6)
        x = g(R(gen, B, *shape, cin) + 0.5)
        w, b = g(R(gen, cout, cin, 3, 3, 3, s=0.2)), g(R(gen, cout))
        mean, rstd = ops.instnorm_stats(x)
        z, zst = ops.conv3d_forward_normin(x, mean, rstd, w, b, cout % 4 == 0)
        yield {"mean": mean, "rstd": rstd, "z": z, "zst": zst}
        dz = g(R(gen, *z.shape))
        if _lib().load().modet_conv3d_bwd_weight_normin_ok(B, *shape, cin, cout):
            amax = g(dz.abs().max().reshape(1).expand(ops.AMAX_FLOATS).contiguous())
            dw, db = ops.conv3d_backward_weight(x, dz, True, amax=amax, norm=(mean, rstd))
            yield {"dw": dw, "db": db}
    return case


def _lib():
    from smilecode_amd import _lib as m
    return m


def elementwise_case(name, C, shape, B):
    """instnorm_lrelu | avgpool2 | pool_tee | pool_tee_split | in_pool_split | upsample2 | to_cl | to_ncdhw"""
    def case(g):
        ops, gen = _ops(), G(7)
        if name == "to_cl":
            x = g(R(gen, B, C, *shape)).requires_grad_(True)
        else:
            x = g(R(gen, B, *shape, C) + 0.3).requires_grad_(True)
        if name == "instnorm_lrelu":
            outs = [ops.instnorm_lrelu(x)]
        elif name == "avgpool2":
            outs = [ops.avgpool2(x)]
        elif name == "pool_tee":
            outs = list(ops.pool_tee(x))
        elif name == "pool_tee_split":
            outs = list(ops.pool_tee_split(x, B // 2))
        elif name == "in_pool_split":
            outs = list(ops.instnorm_lrelu_pool_tee_split(x, None, B // 2))
        elif name == "upsample2":
            outs = [ops.upsample2(x, 2.0)]
        elif name == "to_cl":
            outs = [ops.to_channels_last(x)]
        else:
            outs = [ops.to_ncdhw(x)]
        yield {"out%d" % i: o for i, o in enumerate(outs)}
        yield _grads(outs, {"x": x}, [g(R(gen, *o.shape)) for o in outs])
    return case


def proj_case(cin, dim, n, pair):
    def case(g):
        ops, gen = _ops(), G(8)
        xs = [g(R(gen, 1, 1, 1, n, cin)).requires_grad_(True) for _ in range(2 if pair else 1)]
        Wt, b, ga, be = (g(t).requires_grad_(True) for t in (R(gen, dim, cin, s=0.3), R(gen, dim), 1 + 0.1 * R(gen, dim), R(gen, dim)))
        ys = list(ops.proj_ln_pair(xs[0], xs[1], Wt, b, ga, be)) if pair else [ops.proj_ln(xs[0], Wt, b, ga, be)]
        yield {"y%d" % i: y for i, y in enumerate(ys)}
        ins = {"W": Wt, "b": b, "gamma": ga, "beta": be}
        ins.update({"x%d" % i: x for i, x in enumerate(xs)})
        yield _grads(ys, ins, [g(R(gen, *y.shape)) for y in ys])
    return case


def na_case(heads, hd, shape, B):
    def case(g):
        ops, gen = _ops(), G(9)
        q, k = (g(R(gen, B, *shape, heads * hd)).requires_grad_(True) for _ in range(2))
        rpb = g(R(gen, heads, 3, 3, 3, s=0.5)).requires_grad_(True)
        out = ops.neighbourhood_attention(q, k, rpb, heads, 0.7)
        with torch.no_grad():
            out_ng = ops.neighbourhood_attention(q, k, rpb, heads, 0.7)          # (no lse)
        yield {"out": out, "out_ng": out_ng}
        yield _grads([out], {"q": q, "k": k, "rpb": rpb}, [g(R(gen, *out.shape))])
    return case


def level_attn_case(cin, heads, shape, B, with_flow, src16, tee=False):
    """level_attention_bf16: modet_warp_fwd_t, proj_ln_fwd_t, na_fwd_t / na_bwd_t, proj_ln_bwd_pair_t, the tile warp backward"""
    def case(g):
        ops, gen = _ops(), G(10)
        dim = heads * 6
        F_, M_ = R(gen, B, *shape, cin), R(gen, B, *shape, cin)
        if src16:                        # fp32 handles (one element, expanded, never read) that carry the bf16 features
            F, M = (g(torch.zeros(1)).expand(B, *shape, cin).requires_grad_(True) for _ in range(2))
            F.data16, M.data16 = g(F_.bfloat16()), g(M_.bfloat16())
        else:
            F, M = g(F_).requires_grad_(True), g(M_).requires_grad_(True)
        flow = g(R(gen, B, *shape, 3, s=1.5)).requires_grad_(True) if with_flow else None
        Wt, b, ga, be = (g(t).requires_grad_(True) for t in (R(gen, dim, cin, s=0.3), R(gen, dim), 1 + 0.1 * R(gen, dim), R(gen, dim)))
        rpb = g(R(gen, heads, 3, 3, 3, s=0.5)).requires_grad_(True)
        res = ops.level_attention_bf16(F, M, flow, Wt, b, ga, be, rpb, heads, 0.7, tee=tee)
        outs = list(res) if isinstance(res, tuple) else [res]
        yield {"out": outs[0]}
        ins = {"F": F, "M": M, "flow": flow, "W": Wt, "b": b, "gamma": ga, "beta": be, "rpb": rpb}
        yield _grads(outs, ins, [g(R(gen, *o.shape)) for o in outs])
    return case


def corr_case(C, shape, B):
    def case(g):
        ops, gen = _ops(), G(11)
        mov, fix = (g(R(gen, B, *shape, C)).requires_grad_(True) for _ in range(2))
        corr = ops.correlation3d(mov, fix)
        yield {"corr": corr}
        yield _grads([corr], {"mov": mov, "fix": fix}, [g(R(gen, *corr.shape))])
    return case


def warp_case(C, shape, B, amp, mode=0, add_flow=False, flow_bound=0, src_grad=True, tee=False, det=False, tiles=True):
    def case(g):
        ops, gen = _ops(), G(12)
        src = g(R(gen, B, *shape, C)).requires_grad_(src_grad and mode == 0)
        fl = R(gen, B, *shape, 3, s=amp)
        if flow_bound:
            fl = fl.clamp(-1, 1)
            fl[:, 0, 0, :4] = torch.tensor([[1.0, -1.0, 0.0], [-1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])   # the promise's boundary
        flow = g(fl).requires_grad_(mode == 0)
        prev_d, prev_t = ops.set_deterministic(det), ops.WARP_TILES
        ops.WARP_TILES = tiles
        try:
            outs = list(ops.warp_tee(src, flow)) if tee else [ops.warp(src, flow, mode, add_flow, flow_bound)]
            yield {"out": outs[0]}
            if mode == 0:
                yield _grads(outs, {"src": src, "flow": flow}, [g(R(gen, *o.shape)) for o in outs])
        finally:
            ops.set_deterministic(prev_d)
            ops.WARP_TILES = prev_t
    return case


def cwm_case(heads, n):
    def case(g):
        ops, gen = _ops(), G(13)
        x, lg = g(R(gen, 1, n, heads * 3)).requires_grad_(True), g(R(gen, 1, n, heads)).requires_grad_(True)
        out = ops.cwm_tail(x, lg)
        yield {"out": out}
        yield _grads([out], {"x": x, "logits": lg}, [g(R(gen, *out.shape))])
    return case


def loss_case(kind, shape, B, win=9):
    def case(g):
        ops, gen = _ops(), G(14)
        if kind in ("ncc", "ncc_first", "ncc_vg"):
            a, b = g(torch.rand(B, 1, *shape, generator=gen)), g(torch.rand(B, 1, *shape, generator=gen))
            if kind == "ncc_vg":
                loss, d = ops.ncc_value_and_grad(a, b, win, 0.37)
                yield {"loss": loss, "d": d}
                return
            a.requires_grad_(True)
            b.requires_grad_(kind == "ncc")
            loss = ops.ncc_loss(a, b, win)
            yield {"loss": loss}
            yield _grads([loss], {"a": a, "b": b}, [g(torch.tensor(1.7))])
        elif kind in ("grad3d_l1", "grad3d_l2"):
            f = g(R(gen, B, 3, *shape)).requires_grad_(True)
            loss = ops.grad3d_loss(f, kind[-2:])
            yield {"loss": loss}
            yield _grads([loss], {"f": f}, [g(torch.tensor(0.6))])
        else:
            f = g(R(gen, B, *shape, 3))
            loss, d = ops.grad3d_value_and_grad_cl(f, kind[-2:], 0.37)
            yield {"loss": loss, "d": d}
    return case


def adam_case(n):
    def case(g):
        ops, gen = _ops(), G(15)
        p, gr, m = g(R(gen, n)), g(R(gen, n)), g(R(gen, n, s=0.1))
        v = g(R(gen, n).abs() * 0.01)
        vmax = g(R(gen, n).abs() * 0.01)
        ops.adam_amsgrad_step_(p, gr, m, v, vmax, 1e-3, 3, grad_scale=0.5)
        yield {"p": p, "m": m, "v": v, "vmax": vmax}
    return case


def eval_case(shape, B):
    def case(g):
        from smilecode_amd import synth
        ops, gen = _ops(), G(16)
        flow = g(R(gen, B, *shape, 3, s=2.0))
        counts, det = ops.jacdet_nonpos_count(flow, want_det=True)
        counts2, _ = ops.jacdet_nonpos_count(flow)
        lm, lf = g(torch.from_numpy(synth.make_labels(shape, 24))), g(torch.from_numpy(synth.make_labels(shape, 25)))
        f1 = g(R(gen, 1, *shape, 3, s=2.0))
        warped, c = ops.label_warp_counts(lm, f1, lf, 54)
        _, c2 = ops.label_warp_counts(lm, f1, lf, 54, want_warped=False)
        yield {"jac_counts": counts, "det": det, "jac_counts2": counts2, "warped": warped, "counts": c, "counts2": c2}
    return case


def bf16_case(name, cin, cout, shape, B):
    """cast | raw (conv3d_bf16_forward / _backward_data / _backward_weight) | pair (conv_ins_pair_bf16) | pair_split | pair_split16"""
    def case(g):
        ops, gen = _ops(), G(17)
        if name == "cast":
            x = g(R(gen, 1000))                              # (the library takes multiples of 8 and refuses the rest)
            y = ops.cast_bf16(x, True)
            yield {"y": y.float(), "back": ops.cast_bf16(y, False)}
            return
        x_ = R(gen, B, *shape, cin)
        ws = [R(gen, cout, cin, 3, 3, 3, s=0.2), R(gen, cout), R(gen, cout, cout, 3, 3, 3, s=0.2), R(gen, cout)]
        if name == "raw":
            w, b = g(ws[0]), g(ws[1])
            outs = {}
            for tag, x in (("32", g(x_)), ("16", g(x_.bfloat16()))):
                y, st = ops.conv3d_bf16_forward(x, w, b)
                y_ns, _ = ops.conv3d_bf16_forward(x, w, b, want_stats=False)
                dy = g(R(G(18), *y.shape).bfloat16())
                dw, db = ops.conv3d_bf16_backward_weight(x, dy)
                # (the statistics buffer is not compared raw: its last 64 rows per sample are scratch of the CONSUMING
                #  modet_instnorm_lrelu_fwd_stats_bf16, which the conv does not write -- include/modet_hip.h beside
                #  modet_conv3d_bf16_stats_bytes; the pair cases below consume the buffer through the InstanceNorm)
                outs.update({"y" + tag: y.float(), "y_ns" + tag: y_ns.float(), "dw" + tag: dw, "db" + tag: db,
                             "dx" + tag: ops.conv3d_bf16_backward_data(dy, w, cin, tag == "16").float()})
            yield outs
            return
        x = g(x_).requires_grad_(True)
        p = [g(t).requires_grad_(True) for t in ws]
        if name == "pair":
            outs = [ops.conv_ins_pair_bf16(x, *p)]
        else:
            outs = list(ops.conv_ins_pair_bf16_pool_split(x, *p, B // 2, features16=(name == "pair_split16")))
        if name == "pair_split16":
            yield {"pooled": outs[0], "m16": outs[1].data16.float(), "f16": outs[2].data16.float()}
        else:
            yield {"out%d" % i: o for i, o in enumerate(outs)}
        yield _grads(outs, {"x": x, "w1": p[0], "b1": p[1], "w2": p[2], "b2": p[3]}, [g(R(gen, *o.shape)) for o in outs])
    return case


# The shapes are the ones at which the existing per-op tests already go ragged (tests/test_gpu_ops.py, test_gpu_bf16.py): partial
# tiles, W not a multiple of the vector width, one- and two-voxel axes, B = 2, the smallest and widest channel counts per family.
CASES = {
    # conv families: exact-f32 MFMA, tiled bf16x3, z-marching (x3), direct, transpose-read wgrad, conv_q
    "conv[8->8,9x11x37]": conv_case(8, 8, (9, 11, 37), 1),
    "conv[4->8,6x8x16,B2]": conv_case(4, 8, (6, 8, 16), 2),
    "conv[1->4,act,first block]": conv_case(1, 4, (5, 9, 20), 2, act=True, x_grad=False),
    "conv[8->8,act,x_act]": conv_case(8, 8, (6, 8, 16), 1, act=True, x_act=True),
    "conv[128->128,2x3x10]": conv_case(128, 128, (2, 3, 10), 1),
    "conv[12->2,6x6x18]": conv_case(12, 2, (6, 6, 18), 1),
    "conv[48->8,4x6x20]": conv_case(48, 8, (4, 6, 20), 1),
    "conv[8->8,1x2x1,B2]": conv_case(8, 8, (1, 2, 1), 2),
    "conv_x3[4->8,21x40x41]": conv_case(4, 8, (21, 40, 41), 1),
    "conv_x3[8->4,17x16x50,x_act]": conv_case(8, 4, (17, 16, 50), 1, x_act=True),
    "conv_x3[any range]": conv_case(8, 8, (16, 24, 32), 1, xs=1e5),
    "conv_q[16->32,9x17x28,B2]": conv_case(16, 32, (9, 17, 28), 2),
    "conv_q[64->64,8x9x30,B2]": conv_case(64, 64, (8, 9, 30), 2),
    "conv_q[2->12,12x18x21]": conv_case(2, 12, (12, 18, 21), 1),
    # exact-f32 MFMA on odd channel counts (tests/test_gpu_conv_exact.py): scalar loads, ragged channel stages and N tiles,
    # 2 and 4 output rows packed into N; the weight gradients of 43->43 and 3->16 are the exact-f32 kernel's too
    "conv_exact[43->43,act,9x11x37,B2]": conv_case(43, 43, (9, 11, 37), 2, act=True),
    "conv_exact[43->8,act,17x43x45,B2]": conv_case(43, 8, (17, 43, 45), 2, act=True),
    "conv_exact[16->3,act,17x43x45,B2]": conv_case(16, 3, (17, 43, 45), 2, act=True),
    "conv_exact[3->16,act,17x43x45,B2]": conv_case(3, 16, (17, 43, 45), 2, act=True),
    "conv_stats[8->16,6x8x16]": conv_case(8, 16, (6, 8, 16), 1, form="stats", x_act=True),
    "conv_stats[32->32,4x6x9]": conv_case(32, 32, (4, 6, 9), 2, form="stats"),
    "conv_ins[4->8,9x24x37]": conv_case(4, 8, (9, 24, 37), 1, form="ins"),
    "conv_ins[12->4,7x6x18]": conv_case(12, 4, (7, 6, 18), 1, form="ins"),
    "conv_ins[8->8,33x40x48]": conv_case(8, 8, (33, 40, 48), 1, form="ins", x_act=True),
    "conv_ins[8->8,2x2x2]": conv_case(8, 8, (2, 2, 2), 2, form="ins"),
    "conv_raw[8->8,9x11x37]": raw_conv_case(8, 8, (9, 11, 37), 1),
    "conv_raw[4->8,21x40x41]": raw_conv_case(4, 8, (21, 40, 41), 1),
    "conv_raw[16->32,9x17x28,B2]": raw_conv_case(16, 32, (9, 17, 28), 2),
    "conv_raw[1->4,5x9x20,B2]": raw_conv_case(1, 4, (5, 9, 20), 2),
    "chain[4-8-8,20x24x28,B2]": chain_case(4, 8, 8, (20, 24, 28), 2),
    "chain[8-16-16,17x21x40]": chain_case(8, 16, 16, (17, 21, 40), 1),
    "chain[8-8-4,33x40x48]": chain_case(8, 8, 4, (33, 40, 48), 1),
    "chain[6-12-12,18x20x35]": chain_case(6, 12, 12, (18, 20, 35), 1),
    "chain[16-32-32,12x10x20,B2]": chain_case(16, 32, 32, (12, 10, 20), 2),
    # the training chain that never writes the normalised tensor (modet_conv3d_bwd_weight_normin: z-marching weight gradient)
    "chain_lazy_train[4-8-8,52x44x45,B2]": chain_case(4, 8, 8, (52, 44, 45), 2),
    "chain_inference[8-8-8,33x40x48]": chain_case(8, 8, 8, (33, 40, 48), 1, grad=False),
    "chain_inference[16-16-12,9x11x37]": chain_case(16, 16, 12, (9, 11, 37), 1, grad=False),
    "chain_inference[8-12-2,7x9x18]": chain_case(8, 12, 2, (7, 9, 18), 1, grad=False, want_stats=False),
    "normin[8->8,33x40x48]": normin_case(8, 8, (33, 40, 48), 1),
    "normin[4->8,21x40x41]": normin_case(4, 8, (21, 40, 41), 1),
    "normin[12->2,7x9x18]": normin_case(12, 2, (7, 9, 18), 1),
    "normin[8->8,52x44x45,B2,weight gradient]": normin_case(8, 8, (52, 44, 45), 2),
    # norm / pool / layout
    "instnorm_lrelu[8,9x11x37,B2]": elementwise_case("instnorm_lrelu", 8, (9, 11, 37), 2),
    "instnorm_lrelu[4,1x2x1]": elementwise_case("instnorm_lrelu", 4, (1, 2, 1), 1),
    "instnorm_lrelu[8,2x2x2]": elementwise_case("instnorm_lrelu", 8, (2, 2, 2), 2),
    "instnorm_lrelu[8,40x48x40]": elementwise_case("instnorm_lrelu", 8, (40, 48, 40), 1),
    "avgpool2[8,10x12x14]": elementwise_case("avgpool2", 8, (10, 12, 14), 2),
    "avgpool2[4,6x10x14]": elementwise_case("avgpool2", 4, (6, 10, 14), 1),
    "pool_tee[16,6x8x10]": elementwise_case("pool_tee", 16, (6, 8, 10), 1),
    "pool_tee_split[8,6x8x10,B4]": elementwise_case("pool_tee_split", 8, (6, 8, 10), 4),
    "in_pool_split[8,10x12x18,B2]": elementwise_case("in_pool_split", 8, (10, 12, 18), 2),
    "upsample2[3,5x6x7,B2]": elementwise_case("upsample2", 3, (5, 6, 7), 2),
    "upsample2[6,16x41x50,B2,separable]": elementwise_case("upsample2", 6, (16, 41, 50), 2),
    "upsample2[1,1x2x3]": elementwise_case("upsample2", 1, (1, 2, 3), 1),
    "to_cl[3,5x6x7,B2]": elementwise_case("to_cl", 3, (5, 6, 7), 2),
    "to_ncdhw[27,4x5x9]": elementwise_case("to_ncdhw", 27, (4, 5, 9), 1),
    # projection + LayerNorm
    "proj_ln[8->6,70001]": proj_case(8, 6, 70001, False),
    "proj_ln[128->48,1203]": proj_case(128, 48, 1203, False),
    "proj_ln_pair[8->6,70001]": proj_case(8, 6, 70001, True),
    "proj_ln_pair[16->6,5003]": proj_case(16, 6, 5003, True),
    "proj_ln_pair[64->24,1531]": proj_case(64, 24, 1531, True),
    "proj_ln_pair[128->48,1203]": proj_case(128, 48, 1203, True),
    # attention
    "na[h1,9x7x21,B2]": na_case(1, 6, (9, 7, 21), 2),
    "na[h2,5x13x18,B2]": na_case(2, 6, (5, 13, 18), 2),
    "na[h8,3x3x3]": na_case(8, 6, (3, 3, 3), 2),
    "na[h4,2x1x2]": na_case(4, 6, (2, 1, 2), 2),
    "na[h2,hd8,9x6x21]": na_case(2, 8, (9, 6, 21), 1),
    "na[h1,hd64,5x9x18]": na_case(1, 64, (5, 9, 18), 1),
    "level_attn[no flow,fp32 in]": level_attn_case(128, 8, (5, 6, 7), 2, False, False),
    "level_attn[flow,fp32 in]": level_attn_case(8, 1, (9, 11, 21), 1, True, False),
    "level_attn[flow,bf16 in,tee]": level_attn_case(16, 1, (8, 12, 17), 2, True, True, tee=True),
    "level_attn[flow,fp32 in,h2]": level_attn_case(32, 2, (6, 7, 9), 1, True, False),
    "corr3d[8,1x1x3]": corr_case(8, (1, 1, 3), 1),
    "corr3d[12,9x10x33,B2]": corr_case(12, (9, 10, 33), 2),
    "corr3d[32,6x5x7]": corr_case(32, (6, 5, 7), 1),
    # warps: tiles (default), the gather of a bounded flow, nearest, the image warp, deterministic integer atomics, float atomics
    "warp_tiles[8,16x24x40,B2]": warp_case(8, (16, 24, 40), 2, 2.0),
    "warp_tiles[16,13x21x37]": warp_case(16, (13, 21, 37), 1, 6.0, tee=True),
    "warp_tiles[64,10x12x10,B2]": warp_case(64, (10, 12, 10), 2, 1.5),
    "warp_tiles[3,7x9x11,add_flow]": warp_case(3, (7, 9, 11), 1, 1.0, add_flow=True),
    "warp_bounded[3,9x10x21,B2]": warp_case(3, (9, 10, 21), 2, 0.7, add_flow=True, flow_bound=1),
    "warp_nearest[1,8x8x8]": warp_case(1, (8, 8, 8), 2, 2.5, mode=1),
    "warp_image[1,12x16x20,B2]": warp_case(1, (12, 16, 20), 2, 2.0, src_grad=False, tee=True),
    "warp_det[3,12x16x20,B2,add_flow]": warp_case(3, (12, 16, 20), 2, 3.0, add_flow=True, det=True, tiles=False),
    "warp_det[1,8x8x8]": warp_case(1, (8, 8, 8), 1, 3.0, det=True),
    "warp_atomic[8,16x24x32]": warp_case(8, (16, 24, 32), 1, 2.0, tiles=False),
    "warp_atomic[1,12x16x20,B2]": warp_case(1, (12, 16, 20), 2, 2.0, tiles=False),
    "cwm_tail[h2,1003]": cwm_case(2, 1003),
    "cwm_tail[h8,10x12x10]": cwm_case(8, 1200),
    # losses, optimizer, evaluation
    "ncc[9,9x24x32]": loss_case("ncc", (9, 24, 32), 1),
    "ncc[9,4x5x6]": loss_case("ncc", (4, 5, 6), 1),
    "ncc[9,37x50x70,B2,first argument]": loss_case("ncc_first", (37, 50, 70), 2),
    "ncc[5,9x24x32]": loss_case("ncc", (9, 24, 32), 2, win=5),
    "ncc_box[5x3x7]": loss_case("ncc", (9, 24, 33), 2, win=[5, 3, 7]),
    "ncc_box[2x6x3]": loss_case("ncc", (7, 9, 11), 1, win=[2, 6, 3]),
    "ncc_box[1x1x1]": loss_case("ncc", (3, 4, 5), 1, win=[1, 1, 1]),
    "ncc_value_and_grad[9x24x32]": loss_case("ncc_vg", (9, 24, 32), 2),
    "grad3d[l2,7x9x11,B2]": loss_case("grad3d_l2", (7, 9, 11), 2),
    "grad3d[l1,2x2x3]": loss_case("grad3d_l1", (2, 2, 3), 1),
    "grad3d_cl[l2,7x9x11,B2]": loss_case("grad3d_cl_l2", (7, 9, 11), 2),
    "grad3d_cl[l1,9x24x33]": loss_case("grad3d_cl_l1", (9, 24, 33), 1),
    "adam[100003]": adam_case(100003),
    "adam[7]": adam_case(7),
    "eval[7x9x11,B2]": eval_case((7, 9, 11), 2),
    "eval[2x3x2]": eval_case((2, 3, 2), 1),
    # bf16 storage
    "bf16_cast": bf16_case("cast", 0, 0, (), 0),
    "bf16_raw[8->8,9x11x37]": bf16_case("raw", 8, 8, (9, 11, 37), 1),
    "bf16_raw[16->32,6x8x17,B2]": bf16_case("raw", 16, 32, (6, 8, 17), 2),
    "bf16_raw[8->16,21x19x35,B2]": bf16_case("raw", 8, 16, (21, 19, 35), 2),
    "bf16_pair[8->16,9x11x37]": bf16_case("pair", 8, 16, (9, 11, 37), 1),
    "bf16_pair[4->8,20x24x28,B2]": bf16_case("pair", 4, 8, (20, 24, 28), 2),
    "bf16_pair[64->128,1x2x1]": bf16_case("pair", 64, 128, (1, 2, 1), 1),
    "bf16_pair_split[8->8,10x12x18,B2]": bf16_case("pair_split", 8, 8, (10, 12, 18), 2),
    "bf16_pair_split16[8->8,10x12x18,B2]": bf16_case("pair_split16", 8, 8, (10, 12, 18), 2),
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_op_between_guard_bands(px, tag):
    run_guarded(CASES[tag], px, tag.split("[")[0])
    RAN.add(("a", tag))


# ------------------------------------------------------------------------------------------------ (b) the C ABI directly
# Entry points the wrappers reach only with slack (ops._ws adds a float to every workspace) or not at all.  Workspaces are exactly
# *_ws_bytes(...) bytes rounded up to 4, between bands, poisoned; outputs are poisoned too.
def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(code, what):
    _lib().check(code, what)


def abi_qk(shape, heads, d, B, f64):
    def case(g):
        L, gen, sfx = _lib().load(), G(21), "_f64" if f64 else ""
        dt = torch.float64 if f64 else torch.float32
        D, H, W = shape
        q, k = g(R(gen, B, heads, D, H, W, d).to(dt)), g(R(gen, B, heads, D + 2, H + 2, W + 2, d).to(dt))
        rpb, da = g(R(gen, heads, 3, 3, 3).to(dt)), g(R(gen, B, heads, D, H, W, 27).to(dt))
        attn, attn0 = g.empty((B, heads, D, H, W, 27), dt), g.empty((B, heads, D, H, W, 27), dt)
        _ok(getattr(L, "modet_qk_fwd" + sfx)(q.data_ptr(), k.data_ptr(), rpb.data_ptr(), attn.data_ptr(), B, heads, D, H, W, d, _st()), "qk_fwd")
        _ok(getattr(L, "modet_qk_fwd" + sfx)(q.data_ptr(), k.data_ptr(), None, attn0.data_ptr(), B, heads, D, H, W, d, _st()), "qk_fwd")
        yield {"attn": attn, "attn0": attn0}
        nb = getattr(L, "modet_qk_bwd_ws_bytes" + sfx)(B, heads, D, H, W)
        dq, dk, dr, ws = g.empty(q.shape, dt), g.empty(k.shape, dt), g.empty(rpb.shape, dt), g.ws(nb)
        _ok(getattr(L, "modet_qk_bwd" + sfx)(da.data_ptr(), q.data_ptr(), k.data_ptr(), dq.data_ptr(), dk.data_ptr(), dr.data_ptr(),
                                             ws.data_ptr(), nb, B, heads, D, H, W, d, _st()), "qk_bwd")
        yield {"dq": dq, "dk": dk, "drpb": dr}
    return case


def _collapsing_flow(gen, B, D, H, W):
    grid = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"), -1).float()
    target = torch.tensor([D * 0.43, H * 0.51, W * 0.37])
    return ((target - grid)[None] + 0.45 * R(gen, B, D, H, W, 3)).contiguous()


def abi_warp_bwd(kind, C, shape, B, amp, add_flow=0, s16=False):
    """kind: tiles (modet_warp_bwd_tiles + _dsrc_tiles) | det | t (modet_warp_bwd_t) | plain (modet_warp_bwd) | bounded"""
    def case(g):
        L, gen = _lib().load(), G(22)
        D, H, W = shape
        src_ = R(gen, B, D, H, W, C)
        src = g(src_.bfloat16() if s16 else src_)
        if kind == "bounded":
            fl = R(gen, B, D, H, W, 3).clamp(-1, 1)
        else:
            fl = R(gen, B, D, H, W, 3, s=amp) if amp >= 0 else _collapsing_flow(gen, B, D, H, W)
        flow = g(fl)
        do = R(gen, B, D, H, W, C, s=3.7)
        do[:, : D // 3] = 0.0
        dout, add = g(do), g(R(gen, B, D, H, W, 3))
        dsrc, dflow = g.empty(src_.shape), g.empty(fl.shape)
        a = [B, D, H, W, C]
        if kind == "tiles":
            nb = L.modet_warp_bwd_dsrc_tiles_ws_bytes(*a)
            assert nb > 0
            note_many({"guard.warp_tiles_ws_bytes[C%d,%s,B%d]" % (C, "x".join(map(str, shape)), B): nb,
                       "guard.warp_tiles_ws_bytes_per_voxel[C%d,%s,B%d]" % (C, "x".join(map(str, shape)), B): nb / (B * D * H * W)})
            ws, only = g.ws(nb), g.empty(src_.shape)
            _ok(L.modet_warp_bwd_tiles(src.data_ptr(), int(s16), flow.data_ptr(), dout.data_ptr(), dsrc.data_ptr(), dflow.data_ptr(),
                                       add.data_ptr(), ws.data_ptr(), nb, *a, add_flow, _st()), "warp_bwd_tiles")
            ws2 = g.ws(nb)
            _ok(L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), dout.data_ptr(), only.data_ptr(), ws2.data_ptr(), nb, *a, _st()), "dsrc_tiles")
            yield {"dsrc_tiles": dsrc, "dflow": dflow, "dsrc_only": only}
        elif kind == "det":
            nb = L.modet_warp_bwd_det_ws_bytes(*a)
            ws = g.ws(nb)
            _ok(L.modet_warp_bwd_det(src.data_ptr(), int(s16), flow.data_ptr(), dout.data_ptr(), dsrc.data_ptr(), dflow.data_ptr(),
                                     add.data_ptr(), ws.data_ptr(), nb, *a, add_flow, _st()), "warp_bwd_det")
            yield {"dsrc_det": dsrc, "dflow": dflow}
        elif kind == "t":
            _ok(L.modet_warp_bwd_t(src.data_ptr(), int(s16), flow.data_ptr(), dout.data_ptr(), dsrc.data_ptr(), dflow.data_ptr(), *a,
                                   0, 0, _st()), "warp_bwd_t")
            yield {"d_src": dsrc, "dflow": dflow}
        else:
            _ok(L.modet_warp_bwd(src.data_ptr(), flow.data_ptr(), dout.data_ptr(), dsrc.data_ptr(), dflow.data_ptr(), *a, add_flow,
                                 int(kind == "bounded"), _st()), "warp_bwd")
            yield {("dsrc_gather" if kind == "bounded" else "d_src"): dsrc, "dflow": dflow}
    return case


def abi_warp_fwd_typed(C, shape, B):
    """modet_warp_fwd_o16, modet_warp_fwd_t (bf16 src -> fp32 and bf16 out), modet_avgpool2_fwd_x16"""
    def case(g):
        L, gen = _lib().load(), G(23)
        D, H, W = shape
        s_ = R(gen, B, D, H, W, C)
        src, s16, flow = g(s_), g(s_.bfloat16()), g(R(gen, B, D, H, W, 3, s=2.0))
        o16, t32, t16 = g.empty(s_.shape, torch.bfloat16), g.empty(s_.shape), g.empty(s_.shape, torch.bfloat16)
        a = [B, D, H, W, C]
        _ok(L.modet_warp_fwd_o16(src.data_ptr(), flow.data_ptr(), o16.data_ptr(), *a, _st()), "warp_fwd_o16")
        _ok(L.modet_warp_fwd_t(s16.data_ptr(), 1, flow.data_ptr(), t32.data_ptr(), 0, *a, _st()), "warp_fwd_t")
        _ok(L.modet_warp_fwd_t(s16.data_ptr(), 1, flow.data_ptr(), t16.data_ptr(), 1, *a, _st()), "warp_fwd_t")
        x16 = g(R(gen, B, 2 * (D // 2), 2 * (H // 2), 2 * (W // 2), C).bfloat16())
        pooled = g.empty((B, D // 2, H // 2, W // 2, C))
        _ok(L.modet_avgpool2_fwd_x16(x16.data_ptr(), pooled.data_ptr(), B, 2 * (D // 2), 2 * (H // 2), 2 * (W // 2), C, _st()), "avgpool2_fwd_x16")
        yield {"o16": o16.float(), "t32": t32, "t16": t16.float(), "pooled": pooled}
    return case


def abi_upsample_bwd(C, shape, B):
    def case(g):
        L, gen = _lib().load(), G(24)
        d, h, w = shape
        dy = g(R(gen, B, 2 * d, 2 * h, 2 * w, C))
        dx, dx1 = g.empty((B, d, h, w, C)), g.empty((B, d, h, w, C))
        nb = L.modet_upsample2_bwd_sep_ws_bytes(B, d, h, w, C)
        assert nb > 0
        ws = g.ws(nb)
        _ok(L.modet_upsample2_bwd_sep(dy.data_ptr(), dx.data_ptr(), ws.data_ptr(), nb, B, d, h, w, C, 2.0, _st()), "upsample2_bwd_sep")
        _ok(L.modet_upsample2_bwd(dy.data_ptr(), dx1.data_ptr(), B, d, h, w, C, 2.0, _st()), "upsample2_bwd")
        yield {"dx_sep": dx, "dx_gather": dx1}
    return case


def abi_ncc(shape, B, win):
    """win: a (wz,wy,wx) tuple = modet_ncc_fwd_bwd_box; an int = modet_ncc_fwd_bwd (9), _win and _win_scaled"""
    def case(g):
        L, gen = _lib().load(), G(25)
        D, H, W = shape
        I, J = g(torch.rand(B, 1, D, H, W, generator=gen)), g(torch.rand(B, 1, D, H, W, generator=gen))
        out = {}
        if isinstance(win, tuple):
            nb = L.modet_ncc_box_ws_bytes(B, D, H, W, *win)
            assert nb > 0
            loss, dJ, ws = g.empty(1), g.empty(J.shape), g.ws(nb)
            _ok(L.modet_ncc_fwd_bwd_box(I.data_ptr(), J.data_ptr(), loss.data_ptr(), dJ.data_ptr(), ws.data_ptr(), nb, B, D, H, W, *win, _st()), "ncc_box")
            loss2, ws2 = g.empty(1), g.ws(nb)
            _ok(L.modet_ncc_fwd_bwd_box(I.data_ptr(), J.data_ptr(), loss2.data_ptr(), None, ws2.data_ptr(), nb, B, D, H, W, *win, _st()), "ncc_box")
            out.update(loss=loss, dJ=dJ, loss_nograd=loss2)
        else:
            nb = L.modet_ncc_ws_bytes(B, D, H, W)
            for name, call in (("plain", lambda *p: L.modet_ncc_fwd_bwd(*p, B, D, H, W, _st())),
                               ("win", lambda *p: L.modet_ncc_fwd_bwd_win(*p, B, D, H, W, win, _st())),
                               ("scaled", lambda *p: L.modet_ncc_fwd_bwd_win_scaled(*p, B, D, H, W, win, 0.37, _st()))):
                if name == "plain" and win != 9:
                    continue
                loss, dJ, ws = g.empty(1), g.empty(J.shape), g.ws(nb)
                _ok(call(I.data_ptr(), J.data_ptr(), loss.data_ptr(), dJ.data_ptr(), ws.data_ptr(), nb), "ncc " + name)
                out.update({"loss_" + name: loss, "dJ_" + name: dJ})
        yield out
    return case


def abi_corr3d(C, shape, B):
    def case(g):
        L, gen = _lib().load(), G(26)
        D, H, W = shape
        mov, fix, dc = g(R(gen, B, D, H, W, C)), g(R(gen, B, D, H, W, C)), g(R(gen, B, 27, D, H, W))
        nb = L.modet_corr3d_ws_bytes(B, D, H, W, C)
        corr, ws = g.empty((B, 27, D, H, W)), g.ws(nb)
        _ok(L.modet_corr3d_fwd(mov.data_ptr(), fix.data_ptr(), corr.data_ptr(), ws.data_ptr(), nb, B, D, H, W, C, _st()), "corr3d_fwd")
        yield {"corr": corr}
        dm, df, ws2 = g.empty(mov.shape), g.empty(mov.shape), g.ws(nb)
        _ok(L.modet_corr3d_bwd(mov.data_ptr(), fix.data_ptr(), dc.data_ptr(), dm.data_ptr(), df.data_ptr(), ws2.data_ptr(), nb, B, D, H, W, C,
                               _st()), "corr3d_bwd")
        yield {"dmov": dm, "dfix": df}
    return case


def abi_leaf_reduce():
    """modet_leaf_reduce_many: the d_rpb layout of modet_na_bwd and the projection pair's, partial rows between bands"""
    def case(g):
        m, gen = _lib(), G(27)
        L = m.load()
        B, heads, rows, dim, cin, prow = 2, 3, 37, 6, 8, 53
        part1 = g(R(gen, B * heads * rows * 27))
        ncol = 3 * dim + dim * cin
        part2 = g(R(gen, prow * ncol))
        drpb = g.empty(heads * 27)
        dg, dbeta, db, dW = g.empty(dim), g.empty(dim), g.empty(dim), g.empty(dim * cin)
        jobs = (m.LeafJob * 2)()
        jobs[0].part, jobs[0].outer, jobs[0].outer_stride, jobs[0].rows, jobs[0].row_stride = part1.data_ptr(), B, heads * rows * 27, rows, 27
        jobs[0].col_group_stride, jobs[0].ncols, jobs[0].col_group = rows * 27, heads * 27, 27
        jobs[0].dst[0], jobs[0].n[0] = drpb.data_ptr(), heads * 27
        jobs[1].part, jobs[1].outer, jobs[1].outer_stride, jobs[1].rows, jobs[1].row_stride = part2.data_ptr(), 1, 0, prow, ncol
        jobs[1].col_group_stride, jobs[1].ncols, jobs[1].col_group = 0, ncol, ncol
        for i, (t, n) in enumerate(((dg, dim), (dbeta, dim), (db, dim), (dW, dim * cin))):
            jobs[1].dst[i], jobs[1].n[i] = t.data_ptr(), n
        _ok(L.modet_leaf_reduce_many(ctypes.addressof(jobs), 2, _st()), "leaf_reduce_many")
        yield {"drpb": drpb, "dg": dg, "dbeta": dbeta, "db": db, "dW": dW}
    return case


class _Ctx:
    """a step context of the library for one case"""

    def __init__(self, L):
        self.L, self.h = L, ctypes.c_void_p()
        _ok(L.modet_step_ctx_create(ctypes.byref(self.h)), "step_ctx_create")

    def close(self):
        if self.h:
            self.L.modet_step_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()


def abi_wgrad_defer(cin, cout, shape, B, bf16=False):
    """modet_conv3d_bwd_weight_defer (+ y_act for 1 -> 4) / modet_conv3d_bf16_bwd_weight_defer, then the one flush"""
    def case(g):
        L, gen = _lib().load(), G(28)
        D, H, W = shape
        x_, dy_ = R(gen, B, D, H, W, cin), R(gen, B, D, H, W, cout)
        x, dy = g(x_.bfloat16() if bf16 else x_), g(dy_.bfloat16() if bf16 else dy_)
        yact = g(R(gen, B, D, H, W, cout)) if (cin, cout) == (1, 4) and not bf16 else None
        dw, db, dw2, db2 = g.empty((cout, cin, 3, 3, 3)), g.empty(cout), g.empty((cout, cin, 3, 3, 3)), g.empty(cout)
        a = [B, D, H, W, cin, cout]
        ctx = _Ctx(L)
        try:
            if bf16:
                nb = L.modet_conv3d_bf16_bwd_weight_ws_bytes(*a)
                ws, ws2 = g.ws(nb), g.ws(nb)
                _ok(L.modet_conv3d_bf16_bwd_weight_defer(x.data_ptr(), 1, dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, *a, _st(),
                                                         ctx.h), "bf16_bwd_weight_defer")
                _ok(L.modet_conv3d_bf16_bwd_weight(x.data_ptr(), 1, dy.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ws2.data_ptr(), nb, *a, _st()),
                    "bf16_bwd_weight")
            else:
                nb = L.modet_conv3d_bwd_weight_ws_bytes(*a)
                ws, ws2 = g.ws(nb), g.ws(nb)
                ya = None if yact is None else yact.data_ptr()
                _ok(L.modet_conv3d_bwd_weight_defer(x.data_ptr(), dy.data_ptr(), ya, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, *a, _st(),
                                                    ctx.h), "bwd_weight_defer")
                if ya is None:
                    _ok(L.modet_conv3d_bwd_weight(x.data_ptr(), dy.data_ptr(), dw2.data_ptr(), db2.data_ptr(), ws2.data_ptr(), nb, *a, _st()), "bwd_weight")
                else:
                    _ok(L.modet_conv3d_bwd_weight_act(x.data_ptr(), dy.data_ptr(), ya, dw2.data_ptr(), db2.data_ptr(), ws2.data_ptr(), nb, *a, _st()),
                        "bwd_weight_act")
            _ok(L.modet_conv3d_wgrad_defer_flush(ctx.h, _st()), "wgrad_defer_flush")
            torch.cuda.synchronize()
        finally:
            ctx.close()
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "the deferred reduction is the immediate one, bit for bit"
        yield {"dw": dw, "db": db}
    return case


def abi_prepack(layers, shape, B):
    """the prepack protocol of include/modet_hip.h with an arena of exactly modet_conv3d_prepack_arena_bytes: record one pass of
    conv forwards + data gradients, then the same pass on the packed weights -- bit-identical"""
    def case(g):
        L, gen = _lib().load(), G(29)
        D, H, W = shape
        xs = [g(R(gen, B, D, H, W, ci)) for ci, _ in layers]
        wts = [g(R(gen, co, ci, 3, 3, 3, s=0.2)) for ci, co in layers]
        bs = [g(R(gen, co)) for _, co in layers]
        dys = [g(R(gen, B, D, H, W, co)) for _, co in layers]
        ctx = _Ctx(L)

        def one_pass():
            res = []
            for (ci, co), x, w, b, dy in zip(layers, xs, wts, bs, dys):
                nb = L.modet_conv3d_ws_bytes(ci, co)
                y, dx, ws, ws2 = g.empty((B, D, H, W, co)), g.empty((B, D, H, W, ci)), g.ws(nb), g.ws(nb)
                _ok(L.modet_conv3d_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), ws.data_ptr(), nb, B, D, H, W, ci, co, 0, _st(), ctx.h),
                    "conv3d_fwd")
                _ok(L.modet_conv3d_bwd_data(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), ws2.data_ptr(), nb, B, D, H, W, ci, co, _st(), ctx.h),
                    "conv3d_bwd_data")
                res += [y, dx]
            return res
        try:
            _ok(L.modet_conv3d_prepack_record(ctx.h, 1), "prepack_record")
            first = one_pass()
            njobs = L.modet_conv3d_prepack_record(ctx.h, 0)
            ab = L.modet_conv3d_prepack_arena_bytes(ctx.h)
            assert njobs > 0 and ab > 0, (njobs, ab)
            arena = g.ws(ab)
            _ok(L.modet_conv3d_prepack_begin(ctx.h, arena.data_ptr(), ab, _st()), "prepack_begin")
            second = one_pass()
            _ok(L.modet_conv3d_prepack_end(ctx.h), "prepack_end")
            torch.cuda.synchronize()
        finally:
            ctx.close()
        for a_, b_ in zip(first, second):
            assert torch.equal(a_, b_), "packed weights from the arena give other results than packing per launch"
        yield {"r%d" % i: t for i, t in enumerate(second)}
    return case


def abi_eval(shape, B):
    """modet_label_warp_counts / modet_jacdet_nonpos_count into poisoned count buffers"""
    def case(g):
        from smilecode_amd import synth
        L, gen = _lib().load(), G(30)
        D, H, W = shape
        lm, lf = g(torch.from_numpy(synth.make_labels(shape, 24))), g(torch.from_numpy(synth.make_labels(shape, 25)))
        f1, fB = g(R(gen, 1, D, H, W, 3, s=2.0)), g(R(gen, B, D, H, W, 3, s=2.0))
        warped, counts = g.empty((D, H, W), torch.int16), g.empty((3, 55), torch.int64)
        _ok(L.modet_label_warp_counts(lm.data_ptr(), f1.data_ptr(), lf.data_ptr(), warped.data_ptr(), counts.data_ptr(), D, H, W, 54, _st()),
            "label_warp_counts")
        jc, det = g.empty(B, torch.int64), g.empty((B, D, H, W), torch.float64)
        _ok(L.modet_jacdet_nonpos_count(fB.data_ptr(), jc.data_ptr(), det.data_ptr(), B, D, H, W, _st()), "jacdet_nonpos_count")
        jc2 = g.empty(B, torch.int64)
        _ok(L.modet_jacdet_nonpos_count(fB.data_ptr(), jc2.data_ptr(), None, B, D, H, W, _st()), "jacdet_nonpos_count")
        yield {"warped": warped, "counts": counts, "jac": jc, "det": det, "jac2": jc2}
    return case


def abi_flat(n):
    """modet_adam_amsgrad_step with an n that no vector width divides, modet_cast_bf16 both ways, modet_lrelu_bwd,
    modet_scale_by_dev_scalar"""
    def case(g):
        L, gen = _lib().load(), G(31)
        p, gr, m, v, vm = g(R(gen, n)), g(R(gen, n)), g(R(gen, n, s=0.1)), g(R(gen, n).abs() * 0.01), g(R(gen, n).abs() * 0.01)
        _ok(L.modet_adam_amsgrad_step(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), vm.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5,
                                      _st()), "adam")
        x = g(R(gen, n))
        nc = n // 8 * 8 + 8                              # the cast takes multiples of 8 (and refuses the rest): an odd number of 8-groups
        xc, y16, back = g(R(gen, nc)), g.empty(nc, torch.bfloat16), g.empty(nc)
        assert L.modet_cast_bf16(xc.data_ptr(), y16.data_ptr(), nc - 1, 1, _st()) != 0
        _ok(L.modet_cast_bf16(xc.data_ptr(), y16.data_ptr(), nc, 1, _st()), "cast_bf16")
        _ok(L.modet_cast_bf16(y16.data_ptr(), back.data_ptr(), nc, 0, _st()), "cast_bf16")
        dx, sc, s = g.empty(n), g.empty(n), g(torch.tensor([0.37]))
        _ok(L.modet_lrelu_bwd(gr.data_ptr(), x.data_ptr(), dx.data_ptr(), n, _st()), "lrelu_bwd")
        _ok(L.modet_scale_by_dev_scalar(x.data_ptr(), s.data_ptr(), sc.data_ptr(), n, _st()), "scale_by_dev_scalar")
        yield {"p": p, "m": m, "v": v, "vmax": vm, "y16": y16.float(), "back": back, "dx": dx, "scaled": sc}
    return case


def abi_instnorm_bwd(cin, cout, shape, B):
    """the plain (non-amax) backward forms no wrapper calls: modet_conv3d_bwd_data_instats + modet_instnorm_lrelu_bwd_rows,
    modet_instnorm_lrelu_bwd, modet_instnorm_lrelu_bwd_pool; all against each other bit for bit where they compute the same thing"""
    def case(g):
        L, gen = _lib().load(), G(32)
        D, H, W = shape
        V = D * H * W
        x = g(R(gen, B, D, H, W, cin) + 0.3)
        w, dz = g(R(gen, cout, cin, 3, 3, 3, s=0.2)), g(R(gen, B, D, H, W, cout))
        mean, rstd = g.empty(B * cin), g.empty(B * cin)
        nbi = L.modet_instnorm_ws_bytes(B, V, cin)
        wsi = g.ws(nbi)
        _ok(L.modet_instnorm_stats(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, 0, wsi.data_ptr(), nbi, B, V, cin, 1e-5, _st()), "instnorm_stats")
        a = [B, D, H, W, cin, cout]
        rb = L.modet_conv3d_bwd_data_instats_bytes(*a)
        assert rb > 0, "this shape must run the kernel family that carries the epilogue"
        nb = L.modet_conv3d_ws_bytes(cin, cout)
        dy, rows, ws = g.empty(x.shape), g.empty(rb // 4), g.ws(nb)
        _ok(L.modet_conv3d_bwd_data_instats(dz.data_ptr(), w.data_ptr(), dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows.data_ptr(),
                                            rb, ws.data_ptr(), nb, *a, _st(), None), "bwd_data_instats")
        dx_rows, ws2 = g.empty(x.shape), g.ws(2 * B * cin * 4)
        _ok(L.modet_instnorm_lrelu_bwd_rows(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx_rows.data_ptr(), rows.data_ptr(), rb,
                                            ws2.data_ptr(), 2 * B * cin * 4, B, V, cin, _st()), "instnorm_lrelu_bwd_rows")
        dx, ws3 = g.empty(x.shape), g.ws(nbi)
        _ok(L.modet_instnorm_lrelu_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), ws3.data_ptr(), nbi, B, V, cin,
                                       _st()), "instnorm_lrelu_bwd")
        gp, ga = g(R(gen, B, D // 2, H // 2, W // 2, cin)), g(R(gen, B - B // 2, D, H, W, cin))
        dx_pool, ws4 = g.empty(x.shape), g.ws(nbi)
        _ok(L.modet_instnorm_lrelu_bwd_pool(gp.data_ptr(), None, ga.data_ptr(), B // 2, x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                            dx_pool.data_ptr(), ws4.data_ptr(), nbi, B, D, H, W, cin, _st()), "instnorm_lrelu_bwd_pool")
        yield {"dy": dy, "rows": rows, "dx_rows": dx_rows, "dx": dx, "dx_pool": dx_pool}
    return case


ABI = {
    "qk[17x9x65,h2,d6,B2]": abi_qk((17, 9, 65), 2, 6, 2, False),
    "qk[12x35x34,h3,d8]": abi_qk((12, 35, 34), 3, 8, 1, False),
    "qk[33x8x32,h2,d4]": abi_qk((33, 8, 32), 2, 4, 1, False),
    "qk[8x9x10,h2,d3,B2]": abi_qk((8, 9, 10), 2, 3, 2, False),
    "qk[3x3x3,h1,d6]": abi_qk((3, 3, 3), 1, 6, 1, False),
    "qk_f64[5x6x7,h2,d6]": abi_qk((5, 6, 7), 2, 6, 1, True),
    "qk_f64[9x17x33,h3,d8]": abi_qk((9, 17, 33), 3, 8, 1, True),
    "warp_det[8,40x48x40]": abi_warp_bwd("det", 8, (40, 48, 40), 1, 3.0),
    "warp_det[3,12x16x20,B2,add_flow]": abi_warp_bwd("det", 3, (12, 16, 20), 2, 3.0, add_flow=1),
    "warp_det[16,8x12x16,bf16 src]": abi_warp_bwd("det", 16, (8, 12, 16), 1, 3.0, s16=True),
    # the one full-size-ish volume of this file: more than one tile per axis and a tile far over its 1 536-entry segment
    "warp_tiles[8,24x32x40,B2,collapsing flow]": abi_warp_bwd("tiles", 8, (24, 32, 40), 2, -1.0),
    "warp_tiles[16,13x21x37,rough flow]": abi_warp_bwd("tiles", 16, (13, 21, 37), 1, 6.0),
    "warp_tiles[8,8x8x8,every sample leaves]": abi_warp_bwd("tiles", 8, (8, 8, 8), 1, 40.0),
    "warp_tiles[3,7x9x11,add_flow]": abi_warp_bwd("tiles", 3, (7, 9, 11), 1, 1.0, add_flow=1),
    "warp_tiles[32,9x8x17,bf16 src]": abi_warp_bwd("tiles", 32, (9, 8, 17), 1, 3.0, s16=True),
    "warp_atomic_t[8,9x11x21,bf16 src]": abi_warp_bwd("t", 8, (9, 11, 21), 2, 2.0, s16=True),
    "warp_atomic[1,12x16x20,B2]": abi_warp_bwd("plain", 1, (12, 16, 20), 2, 2.0),
    "warp_gather[3,9x10x21,B2]": abi_warp_bwd("bounded", 3, (9, 10, 21), 2, 1.0, add_flow=1),
    "warp_fwd_typed[8,9x11x21,B2]": abi_warp_fwd_typed(8, (9, 11, 21), 2),
    "warp_fwd_typed[4,2x3x5]": abi_warp_fwd_typed(4, (2, 3, 5), 1),
    "upsample_bwd[6,16x41x50,B2]": abi_upsample_bwd(6, (16, 41, 50), 2),
    "upsample_bwd[3,33x40x52]": abi_upsample_bwd(3, (33, 40, 52), 1),
    "ncc_box[5x3x7]": abi_ncc((9, 24, 33), 2, (5, 3, 7)),
    "ncc_box[11x11x11]": abi_ncc((12, 13, 17), 1, (11, 11, 11)),
    "ncc_box[2x6x3]": abi_ncc((7, 9, 11), 1, (2, 6, 3)),
    "ncc[9,37x50x70,B2]": abi_ncc((37, 50, 70), 2, 9),
    "ncc[9,4x5x6]": abi_ncc((4, 5, 6), 1, 9),
    "ncc[3,9x24x32]": abi_ncc((9, 24, 32), 1, 3),
    "corr3d[8,1x1x3]": abi_corr3d(8, (1, 1, 3), 1),
    "corr3d[12,9x10x33,B2]": abi_corr3d(12, (9, 10, 33), 2),
    "corr3d[32,6x5x7]": abi_corr3d(32, (6, 5, 7), 1),
    "leaf_reduce_many": abi_leaf_reduce(),
    "wgrad_defer[8->8,9x11x37]": abi_wgrad_defer(8, 8, (9, 11, 37), 1),
    "wgrad_defer[1->4,y_act,5x9x20,B2]": abi_wgrad_defer(1, 4, (5, 9, 20), 2),
    "wgrad_defer[16->32,9x17x28,B2]": abi_wgrad_defer(16, 32, (9, 17, 28), 2),
    "wgrad_defer[4->8,37x46x63]": abi_wgrad_defer(4, 8, (37, 46, 63), 1),
    "wgrad_defer_bf16[8->16,21x19x35,B2]": abi_wgrad_defer(8, 16, (21, 19, 35), 2, bf16=True),
    "prepack[9x11x37]": abi_prepack([(8, 8), (4, 8), (16, 32), (8, 16)], (9, 11, 37), 1),
    "prepack[21x40x41]": abi_prepack([(4, 8), (8, 8)], (21, 40, 41), 1),
    "eval[7x9x11,B2]": abi_eval((7, 9, 11), 2),
    "eval[2x3x2]": abi_eval((2, 3, 2), 1),
    "flat[100003]": abi_flat(100003),
    "flat[7]": abi_flat(7),
    "instnorm_bwd[8->8,33x40x48]": abi_instnorm_bwd(8, 8, (34, 40, 48), 2),
}
ATOMIC.update({
    "abi.warp_atomic_t.d_src": ATOMIC["warp_atomic.d_src"],
    "abi.warp_atomic.d_src": ATOMIC["warp_atomic.d_src"],
})


@pytest.mark.parametrize("tag", sorted(ABI))
def test_abi_between_guard_bands_with_exact_workspaces(px, tag):
    run_guarded(ABI[tag], px, "abi." + tag.split("[")[0], section="b")
    RAN.add(("b", tag))


# ------------------------------------------------------------------------------------------------ (c) whole steps
# GuardedAlloc is entered BEFORE the model and the Trainer are built: the flat parameter / gradient / Adam buffers, the recording
# pass, the packed-weights arena and everything the step allocates sit between bands; the images are guarded by hand.  Eager
# steps only (a hipGraph replay runs the same kernels on the same addresses).
STEPS = {
    "train[16x32x16]": dict(shape=(16, 32, 16)),
    "train[32x48x32,B2]": dict(shape=(32, 48, 32), batch=2),
    "train[heads_4_4_2_1_1,channels=2]": dict(shape=(32, 48, 32), heads=[4, 4, 2, 1, 1], channels=2),
    "train[bf16 storage]": dict(shape=(32, 48, 32), bf16=True),
    "train[staged backward]": dict(shape=(32, 48, 32), staged=True),
    "train[deterministic]": dict(shape=(32, 48, 32), det=True),
}


def _trainer(kw):
    from smilecode_amd import models, synth
    from smilecode_amd.engine import Trainer
    heads, ch = kw.get("heads", [8, 4, 2, 1, 1]), kw.get("channels", 4)
    extra = dict(act_dtype=torch.bfloat16) if kw.get("bf16") else {}
    model = models.ModeT(kw["shape"], channels=ch, head_dim=6, num_heads=heads, scale=1, **extra).cuda()
    models.load_numpy_weights(model, synth.make_weights(24, ch, 6, heads, 1))
    return Trainer(model, overlap_allreduce=bool(kw.get("staged")))


def _step_passes(kw, mode):
    """three forward+backward passes on constant parameters (the recording pass, then two on the packed-weights arena) and one
    Adam update; -> [(losses, flat gradient)] per pass, the updated flat parameters, the damaged bands"""
    from smilecode_amd import ops, synth
    mov, fix = (torch.from_numpy(a) for a in synth.make_pair(kw["shape"], 24, kw.get("batch", 1)))
    g = Maker(mode)
    prev = ops.set_deterministic(bool(kw.get("det")))
    bands, passes = [], []
    try:
        with (contextlib.nullcontext() if mode is None else guard.GuardedAlloc(canary=mode)):
            tr = _trainer(kw)
            mov, fix = g(mov), g(fix)
            run = tr._fwd_bwd_staged if kw.get("staged") else tr._fwd_bwd
            for _ in range(3):
                out = run(mov, fix)
                torch.cuda.synchronize()
                bands += guard.check()
                passes.append(([float(v) for v in out], tr.fp.grad.clone()))
            ops.adam_amsgrad_step_(tr.fp.flat, tr.fp.grad, tr.m, tr.v, tr.vmax, 1e-4, 1)
            torch.cuda.synchronize()
            bands += guard.check()
            flat = tr.fp.flat.clone()
            names, offsets = [n for n, _ in tr.model.named_parameters()], list(tr.fp.offsets)
            tr.release_steps()
            del tr
    finally:
        ops.set_deterministic(prev)
    return passes, flat, bands, names, offsets


def _unguarded_share(records, tag):
    """the share of device-pointer arguments of a whole-step case that pointed into torch memory outside every guarded buffer
    (tensors torch itself produced: .contiguous(), cat, autograd's sums), by entry point, into the parity report"""
    dev = [(n, c) for n, cs in records for c in cs if c in ("guarded", "torch")]
    loose = [n for n, c in dev if c == "torch"]
    rep = {"guard.%s.device_pointer_arguments" % tag: len(dev), "guard.%s.unguarded" % tag: len(loose)}
    for n in set(loose):
        rep["guard.%s.unguarded.%s" % (tag, n)] = loose.count(n)
    note_many(rep)
    return len(loose), len(dev)


@pytest.mark.parametrize("tag", sorted(STEPS))
def test_train_step_between_guard_bands(px, tag):
    """Comparison with the unguarded step, as test_deterministic_train_step_is_bit_reproducible makes it between two trainers:
    BIT-EQUAL -- in deterministic mode, and in the default mode too wherever every warp of the step that scatters ran the
    destination-tile kernel (integer sums): such a step has no float atomics, and a stray read swallowed at 1e-6 is exactly what
    this file looks for.  Only a step in which the proxy SAW a float-atomic scatter (modet_warp_bwd / _acc / _t handed a d_src:
    feature warps whose channel count the tiles do not take, e.g. channels=2) gets the tolerance of the former tools/exp_guard.py,
    5e-6 of max|g| per parameter tensor."""
    kw = STEPS[tag]
    ref, ref_flat, _, names, offsets = _step_passes(kw, None)
    del px.records[:]
    px.log_args = True
    got, flat, bands, _, _ = _step_passes(kw, 0xFF)
    SEEN["c"].extend(px.records)
    RAN.add(("c", tag))
    loose, dev = _unguarded_share(px.records, tag)
    # a float-atomic scatter = one of these three handed a d_src without the bounded-flow promise (that form gathers):
    # name -> (position of d_src, position of flow_bound) in the argument list (include/modet_hip.h)
    scatter = {"modet_warp_bwd": (3, 11), "modet_warp_bwd_acc": (4, 13), "modet_warp_bwd_t": (4, 12)}
    exact = kw.get("det") or not any(n in scatter and a[scatter[n][0]] and not a[scatter[n][1]] for n, a in px.calls)
    px.log_args = False
    del px.calls[:]
    note_many({"guard.%s.float_atomic_scatter" % tag: 0.0 if exact else 1.0})
    del px.records[:]
    guard.release()
    assert not bands, guard.describe(bands)
    assert bool(torch.isfinite(flat).all()), "parameters after the Adam update"
    for i, ((lr, gr), (lg, gg)) in enumerate(zip(ref, got)):
        assert all(v == v and abs(v) != float("inf") for v in lg), (i, lg)
        assert bool(torch.isfinite(gg).all()), "pass %d: the flat gradient is not finite (a read of a band or of poison)" % i
        gmax = float(gr.abs().max())
        if exact:
            assert lg == lr and torch.equal(gg, gr), "pass %d differs from the unguarded step: max |diff| %.3e of max|g|" % (
                i, float((gg - gr).abs().max()) / gmax)
            continue
        assert max(abs(a - b) for a, b in zip(lg, lr)) <= 5e-6 * max(1.0, max(abs(v) for v in lr)), (i, lg, lr)
        bad = ["%s %.2e" % (n, float((gg[o:o + k] - gr[o:o + k]).abs().max()) / gmax) for n, (o, k) in zip(names, offsets)
               if not float((gg[o:o + k] - gr[o:o + k]).abs().max()) <= 5e-6 * gmax]
        assert not bad, "pass %d: parameter gradients differ from the unguarded step (of max|g|): %s" % (i, ", ".join(bad))
    if exact:
        assert torch.equal(flat, ref_flat), "parameters after the Adam update differ from the unguarded step"
    assert loose <= 0.05 * dev, "%d of %d device-pointer arguments were not guarded" % (loose, dev)


def _inference(kw, mode, with_eval):
    from smilecode_amd import synth, utils
    shape = kw["shape"]
    mov, fix = (torch.from_numpy(a) for a in synth.make_pair(shape, 24, kw.get("batch", 1)))
    g = Maker(mode)
    bands, out = [], {}
    with (contextlib.nullcontext() if mode is None else guard.GuardedAlloc(canary=mode)):
        tr = _trainer(kw)
        y, flow = tr.infer(g(mov), g(fix))
        torch.cuda.synchronize()
        bands += guard.check()
        out.update(y=y.clone(), flow=flow.clone())
        if with_eval:
            xs = g(torch.from_numpy(synth.make_labels(shape, 24))[None, None])
            ys = g(torch.from_numpy(synth.make_labels(shape, 25))[None, None])
            warped, dice = utils.warp_labels_and_dice(xs, flow, ys)
            out.update(warped=warped.clone(), dice=torch.tensor(dice), dice_raw=torch.tensor(float(utils.dice_val_VOI(xs, ys))),
                       jac=torch.tensor(utils.jacobian_nonpositive_fraction(flow)),
                       det=torch.from_numpy(utils.jacobian_determinant_vxm(flow[0])))
            torch.cuda.synchronize()
            bands += guard.check()
        tr.release_steps()
        del tr
    return out, bands


@pytest.mark.parametrize("tag", ["infer[32x48x32,B2]", "infer[bf16 storage]", "infer+eval tail[32x48x32]"])
def test_inference_and_eval_tail_between_guard_bands(px, tag):
    """the inference forward (lazily normalised convs, no saved tensors) and the evaluation tail (label warp + Dice counts,
    Jacobian determinant) on the produced flow.  Nothing here sums with float atomics: results are bit-equal to the unguarded run."""
    kw, with_eval = INFER[tag]
    ref, _ = _inference(kw, None, with_eval)
    del px.records[:]
    got, bands = _inference(kw, 0xFF, with_eval)
    SEEN["c"].extend(px.records)
    RAN.add(("c", tag))
    loose, dev = _unguarded_share(px.records, tag)
    del px.records[:]
    guard.release()
    assert not bands, guard.describe(bands)
    for k in got:
        if got[k].dtype.is_floating_point:
            assert bool(torch.isfinite(got[k]).all()), k
    _same(got, ref, "guarded vs unguarded", "infer")
    assert loose <= 0.05 * dev, "%d of %d device-pointer arguments were not guarded" % (loose, dev)


# ------------------------------------------------------------------------------------------------ (e) values that steer addresses
# A flow is the one input whose VALUES become indices.  A few scattered voxels carry displacements far outside anything a
# registration produces; others put the sample's base corner exactly at -2, -1, dim - 1 and dim along an axis.
FAR = [(1e9, 0.0, 0.0), (-1e9, 0.0, 0.0), (0.0, 3e38, 0.0), (0.0, 0.0, -3e38), (3e38, 3e38, 3e38), (-1e9, 1e9, -3e38),
       (0.0, -3e38, 1e9), (3e38, 0.5, -0.5)]


def _steering_flow(shape, B, variant):
    """-> (flow (B,D,H,W,3) on the host, the FAR voxels' indices).  variant: 'far' = the values of FAR; 'ref' = the same voxels
    at +-1e4 (simply outside the volume: zero padding gives 0 output and 0 gradient there, as oracle.modet_torch.warp confirms
    on the CPU, tests/test_cpu.py); 'nan' / 'inf' = non-finite values there.  Everything else is identical in all variants."""
    D, H, W = shape
    gen = G(41)
    flow = R(gen, B, D, H, W, 3, s=2.0)
    dims = (D, H, W)
    k = 0
    for b in range(B):                               # base corners exactly on the volume's faces, one axis at a time
        for axis in range(3):
            for target in (-2.0, -1.0, -1.5, -0.5, dims[axis] - 1.0, float(dims[axis]), dims[axis] - 0.5, dims[axis] - 1.5):
                p = [(3 + 5 * k) % D, (1 + 3 * k) % H, (2 + 7 * k) % W]
                flow[b, p[0], p[1], p[2], axis] = target - p[axis]
                k += 1
    idx = []
    for i, v in enumerate(FAR):
        p = (i % B, (2 + 3 * i) % D, (5 + 2 * i) % H, (1 + 5 * i) % W)
        idx.append(p)
        if variant == "far":
            val = torch.tensor(v)
        elif variant == "ref":
            val = torch.tensor([0.0 if c == 0.0 or abs(c) < 1.0 else (1e4 if c > 0 else -1e4) for c in v]) + torch.tensor(
                [c if abs(c) < 1.0 else 0.0 for c in v])
        else:
            bad = float("nan") if variant == "nan" else float("inf")
            val = torch.tensor([(bad if c > 0 else -bad) if abs(c) >= 1.0 else c for c in v])
        flow[p] = val
    return flow, idx


def flow_case(C, shape, B, variant, zero_dout_at_far=False):
    """every entry point that turns a flow into addresses, on one flow"""
    def case(g):
        from smilecode_amd import synth
        L, gen = _lib().load(), G(42)
        D, H, W = shape
        fl, idx = _steering_flow(shape, B, variant)
        s_ = R(gen, B, D, H, W, C)
        do = R(gen, B, D, H, W, C)
        if zero_dout_at_far:
            for p in idx:
                do[p] = 0.0
        src, s16, flow, dout, add = g(s_), g(s_.bfloat16()), g(fl), g(do), g(R(gen, B, D, H, W, 3))
        a = [B, D, H, W, C]
        out = {}
        for mode in (0, 1):
            o = g.empty(s_.shape)
            _ok(L.modet_warp_fwd(src.data_ptr(), flow.data_ptr(), o.data_ptr(), *a, mode, 0, _st()), "warp_fwd")
            out["fwd_mode%d" % mode] = o
        if C == 3:
            o = g.empty(s_.shape)
            _ok(L.modet_warp_fwd(src.data_ptr(), flow.data_ptr(), o.data_ptr(), *a, 0, 1, _st()), "warp_fwd add_flow")
            out["fwd_add_flow_minus_flow"] = o - flow          # (the composition adds the flow itself: warp(src, flow) is what is compared)
        if C % 4 == 0:
            o16, t16 = g.empty(s_.shape, torch.bfloat16), g.empty(s_.shape, torch.bfloat16)
            _ok(L.modet_warp_fwd_o16(src.data_ptr(), flow.data_ptr(), o16.data_ptr(), *a, _st()), "warp_fwd_o16")
            _ok(L.modet_warp_fwd_t(s16.data_ptr(), 1, flow.data_ptr(), t16.data_ptr(), 1, *a, _st()), "warp_fwd_t")
            out.update(fwd_o16=o16.float(), fwd_t=t16.float())
        yield dict(out)
        af = int(C == 3)
        out = {"dout_in": dout}
        ds, df = g.empty(s_.shape), g.empty(fl.shape)
        _ok(L.modet_warp_bwd(src.data_ptr(), flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), *a, af, 0, _st()), "warp_bwd")
        out.update(atomic_d_src=ds, bwd_d_flow=df)
        ds, df = g.empty(s_.shape), g.empty(fl.shape)
        _ok(L.modet_warp_bwd_acc(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), add.data_ptr(), *a, af, 0,
                                 _st()), "warp_bwd_acc")
        out.update(atomic_acc_d_src=ds, acc_d_flow=df)
        nb = L.modet_warp_bwd_det_ws_bytes(*a)
        ds, df, ws = g.empty(s_.shape), g.empty(fl.shape), g.ws(nb)
        _ok(L.modet_warp_bwd_det(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), add.data_ptr(), ws.data_ptr(),
                                 nb, *a, af, _st()), "warp_bwd_det")
        out.update(det_d_src=ds, det_d_flow=df)
        nb = L.modet_warp_bwd_dsrc_tiles_ws_bytes(*a)
        if nb:
            ds, df, ws = g.empty(s_.shape), g.empty(fl.shape), g.ws(nb)
            _ok(L.modet_warp_bwd_tiles(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), add.data_ptr(),
                                       ws.data_ptr(), nb, *a, af, _st()), "warp_bwd_tiles")
            only, ws2 = g.empty(s_.shape), g.ws(nb)
            _ok(L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), dout.data_ptr(), only.data_ptr(), ws2.data_ptr(), nb, *a, _st()), "dsrc_tiles")
            out.update(tiles_d_src=ds, tiles_d_flow=df, tiles_only_d_src=only)
        lm, lf = g(torch.from_numpy(synth.make_labels(shape, 24))), g(torch.from_numpy(synth.make_labels(shape, 25)))
        f1 = g(fl[:1].contiguous())
        warped, counts = g.empty((D, H, W), torch.int16), g.empty((3, 55), torch.int64)
        _ok(L.modet_label_warp_counts(lm.data_ptr(), f1.data_ptr(), lf.data_ptr(), warped.data_ptr(), counts.data_ptr(), D, H, W, 54, _st()),
            "label_warp_counts")
        out.update(warped=warped, counts=counts)
        yield out
    return case


FLOW_SHAPES = {"C8,9x11x21,B2": (8, (9, 11, 21), 2), "C3,7x9x11": (3, (7, 9, 11), 1), "C16,16x24x32": (16, (16, 24, 32), 1),
               "C1,12x16x20,B2": (1, (12, 16, 20), 2)}
ATOMIC.update({"flow.atomic_d_src": ATOMIC["warp_atomic.d_src"], "flow.atomic_acc_d_src": ATOMIC["warp_atomic.d_src"]})


@pytest.mark.parametrize("tag", sorted(FLOW_SHAPES))
def test_flows_far_outside_the_volume_between_guard_bands(px, tag):
    """+-1e9 and +-3e38 voxels of displacement, and base corners exactly at -2, -1, dim - 1 and dim: no band is damaged, and every
    output equals the run in which the far voxels carry +-1e4 (bit for bit; the float-atomic d_src within its noise)"""
    C, shape, B = FLOW_SHAPES[tag]
    far = run_guarded(flow_case(C, shape, B, "far"), px, "flow", section="e")
    RAN.add(("e", tag))
    ref = _run(flow_case(C, shape, B, "ref"), None, px, "e")
    _same(far, ref, "flows of +-1e9 / +-3e38 vs +-1e4 in the same voxels", "flow")


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("tag", ["C8,9x11x21,B2", "C3,7x9x11"])
def test_non_finite_flows_between_guard_bands(px, tag, bad):
    """NaN / inf displacements: bands stay intact, and d_src -- in the tile path, the integer-atomic path and the float-atomic path
    alike -- is what it is when those voxels contribute nothing (their d_out zeroed, their flow at 1e4).  What `out` and `d_flow`
    hold AT the non-finite voxels is documented in include/modet_hip.h beside modet_warp_fwd / modet_warp_bwd and pinned here."""
    C, shape, B = FLOW_SHAPES[tag]
    got = _run(flow_case(C, shape, B, bad), 0xFF, px, "e")
    ref = _run(flow_case(C, shape, B, "ref", zero_dout_at_far=True), None, px, "e")
    _, idx = _steering_flow(shape, B, bad)
    for k in ("atomic_d_src", "atomic_acc_d_src", "det_d_src", "tiles_d_src", "tiles_only_d_src"):
        if k in got:
            _same({k: got[k]}, {k: ref[k]}, "non-finite flow vs no contribution from those voxels", "flow")
    where = torch.zeros(got["fwd_mode0"].shape[:4], dtype=torch.bool, device="cuda")
    for p in idx:
        where[p] = True
    nan_masks = {}
    for k, v in got.items():
        if k.endswith("d_src") or k in ("counts", "warped", "dout_in") or v.dim() != 5:
            continue
        # away from the non-finite voxels nothing changes
        assert torch.equal(v[~where], ref[k][~where]), "%s changed away from the non-finite voxels" % k
        at, at_ref = v[where], ref[k][where]
        if C == 3 and k.endswith("d_flow"):              # add_flow: d_flow += d_out, and the reference run's d_out is zero there
            at_ref = at_ref + got["dout_in"][where]
        if k in ("fwd_mode0", "fwd_o16", "fwd_t", "fwd_add_flow_minus_flow"):
            assert bool(torch.isnan(at).all()), "%s: a trilinear sample at a non-finite position is NaN in every channel" % k
        elif k == "fwd_mode1":
            assert bool((at == 0).all()), "nearest: a non-finite position is outside the volume -> 0"
        elif k == "tiles_d_flow":
            assert torch.equal(at, at_ref), "tile path: such a voxel is dropped -- its d_flow is d_flow_add (+ d_out with add_flow)"
        else:                                            # modet_warp_bwd / _acc / _det: one kernel body
            nan = torch.isnan(at)
            assert bool((nan | (at == at_ref)).all()), "%s: a component is NaN or carries no contribution of this warp" % k
            assert bool(nan.any(dim=-1).all()), "%s: every non-finite voxel has a NaN component" % k
            nan_masks[k] = nan
    masks = list(nan_masks.values())
    assert all(torch.equal(m, masks[0]) for m in masks), "the float-atomic, the accumulating and the integer-atomic forms agree"
    # the label warp: nearest, so such a voxel takes label 0 (outside) like any other that leaves the volume
    assert bool((got["warped"][where[0]] == 0).all())


def dout_case(C, shape, B, bad):
    """the warp backward on a d_out with ONE entry replaced by ``bad`` (None: by 0, the clean run) in sample 0; sample 1 (B = 2)
    has a block of zero d_out, so that one of its destination tiles stays empty"""
    def case(g):
        L, gen = _lib().load(), G(43)
        D, H, W = shape
        s_, fl, do = R(gen, B, D, H, W, C), R(gen, B, D, H, W, 3, s=0.3), R(gen, B, D, H, W, C)
        if B > 1:
            do[1, :10, :10, :10] = 0.0
        do[DOUT_BAD + (1,)] = 0.0 if bad is None else bad
        src, flow, dout, add = g(s_), g(fl), g(do), g(R(gen, B, D, H, W, 3))
        a, af = [B, D, H, W, C], int(C == 3)
        out = {"flow_in": flow, "dout_in": dout}
        ds, df = g.empty(s_.shape), g.empty(fl.shape)
        _ok(L.modet_warp_bwd(src.data_ptr(), flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), *a, af, 0, _st()), "warp_bwd")
        out.update(atomic_d_src=ds, bwd_d_flow=df)
        ds, df = g.empty(s_.shape), g.empty(fl.shape)
        _ok(L.modet_warp_bwd_acc(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), add.data_ptr(), *a, af, 0,
                                 _st()), "warp_bwd_acc")
        out.update(atomic_acc_d_src=ds, acc_d_flow=df)
        nb = L.modet_warp_bwd_dsrc_tiles_ws_bytes(*a)
        assert nb > 0
        ds, df, ws = g.empty(s_.shape), g.empty(fl.shape), g.ws(nb)
        _ok(L.modet_warp_bwd_tiles(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), ds.data_ptr(), df.data_ptr(), add.data_ptr(),
                                   ws.data_ptr(), nb, *a, af, _st()), "warp_bwd_tiles")
        only, ws2 = g.empty(s_.shape), g.ws(nb)
        _ok(L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), dout.data_ptr(), only.data_ptr(), ws2.data_ptr(), nb, *a, _st()), "dsrc_tiles")
        out.update(tiles_d_src=ds, tiles_d_flow=df, tiles_only_d_src=only)
        yield out
    return case


DOUT_BAD = (0, 5, 9, 13)        # (sample, z, y, x) of the non-finite d_out entry (channel 1)


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("C,shape,B", [(8, (16, 24, 40), 2), (3, (12, 16, 20), 1)])
def test_non_finite_d_out_between_guard_bands(px, C, shape, B, bad):
    """One NaN / inf entry of d_out, as include/modet_hip.h documents it beside modet_warp_bwd_tiles: bands intact; the tile path
    poisons GLOBALLY -- the fixed-point scale is max |d_out| over the whole tensor, so every cell of every non-empty destination
    tile (of every sample, every channel) is NaN, cells of empty tiles are 0 or (on a face shared with a non-empty tile) NaN;
    the float-atomic path (modet_warp_bwd / _acc) is non-finite at the eight corners of that voxel in that channel only.  Its
    other cells receive the same contributions as in the clean run (that entry = 0) in another order: equal within the
    float-atomic tolerance of ATOMIC, the one exception to bit-equality in this file.  d_flow: non-finite at that voxel,
    bit-equal elsewhere (no atomics)."""
    D, H, W = shape
    got = _run(dout_case(C, shape, B, float(bad)), 0xFF, px, "e")
    clean = _run(dout_case(C, shape, B, None), None, px, "e")
    flow, dout = got["flow_in"].cpu(), got["dout_in"].cpu()
    grid = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"), -1).float()
    base = torch.floor(grid[None] + flow).long()                       # fp32, as the kernels: (float)z + flow, floorf
    lim = torch.tensor([D, H, W])
    kept = ((base >= -1) & (base <= lim - 1)).all(-1) & ((dout != 0) | torch.isnan(dout)).any(-1)
    # ---- the tile path
    tiles = torch.zeros(B, -(-D // 8), -(-H // 8), -(-W // 8), dtype=torch.bool)
    tb = base.clamp(min=0) >> 3
    for b in range(B):
        t = tb[b][kept[b]]
        tiles[b, t[:, 0], t[:, 1], t[:, 2]] = True
    assert bool(tiles[0].all()) and (B == 1 or not bool(tiles[1, 0, 0, 0])), "the case has full samples and one empty tile"
    cell_nonempty = tiles.repeat_interleave(8, 1).repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :D, :H, :W].cuda()
    for k in ("tiles_d_src", "tiles_only_d_src"):
        v = got[k]
        assert bool(torch.isnan(v[cell_nonempty]).all()), "%s: every cell of every non-empty tile is NaN" % k
        rest = v[~cell_nonempty]
        assert bool((torch.isnan(rest) | (rest == 0)).all()), "%s: an empty tile holds 0, or NaN on a face of a non-empty neighbour" % k
        if B > 1:
            assert bool((v[1, :7, :7, :7] == 0).all()), "%s: the inside of the empty tile is 0" % k
    # ---- the float-atomic path: the eight corners of the voxel, in its channel
    b0, z, y, x = DOUT_BAD
    corner = torch.zeros(B, D, H, W, C, dtype=torch.bool)
    bz, by, bx = (int(v) for v in base[b0, z, y, x])
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                if 0 <= bz + dz < D and 0 <= by + dy < H and 0 <= bx + dx < W:
                    corner[b0, bz + dz, by + dy, bx + dx, 1] = True
    assert int(corner.sum()) == 8
    corner = corner.cuda()
    for k in ("atomic_d_src", "atomic_acc_d_src"):
        v = got[k]
        at = v[corner]
        assert bool(torch.isnan(at).all()) if bad == "nan" else bool(torch.isinf(at).all()), "%s at the eight corners: %s" % (k, at)
        assert bool(torch.isfinite(v[~corner]).all()), "%s: non-finite outside the eight corners" % k
        tol = ATOMIC["flow." + k][0]
        err, ref = float((v[~corner] - clean[k][~corner]).abs().max()), float(clean[k].abs().max())
        assert err <= tol * ref, "%s: cells outside the eight corners differ from the clean run by %.3e of max" % (k, err / ref)
    where = torch.zeros(B, D, H, W, dtype=torch.bool, device="cuda")
    where[DOUT_BAD] = True
    for k in ("bwd_d_flow", "acc_d_flow", "tiles_d_flow"):
        assert torch.equal(got[k][~where], clean[k][~where]), "%s changed away from the voxel" % k
        assert not bool(torch.isfinite(got[k][where]).any()), "%s at the voxel: %s" % (k, got[k][where])


# ------------------------------------------------------------------------------------------------ (d) coverage by name
INFER = {"infer[32x48x32,B2]": (dict(shape=(32, 48, 32), batch=2), False), "infer[bf16 storage]": (dict(shape=(32, 48, 32), bf16=True), False),
         "infer+eval tail[32x48x32]": (dict(shape=(32, 48, 32)), True)}


def test_every_launching_entry_point_ran_between_guard_bands(px):
    """A condition on this file, not a measurement: every name of _lib.SIGNATURES that launches (everything but the pure queries
    *_bytes, *_family*, *_ok, *_operands, *_partial_rows, version, strerror and step_ctx_create / destroy) was called at least
    once with every device-pointer argument inside a guarded buffer; in the per-op and ABI cases NO device pointer was outside
    one; in the whole steps at most 5 % were (tensors torch produces itself), each named in the parity report.
    Cases of (a), (b), (c) and the far-flow cases of (e) that were deselected from this session (-k) are run here, guarded once,
    so the union does not depend on the selection (the non-finite cases of (e) add no entry point and are not repeated).  The
    test relies on running after the others of this file in the same process -- pytest's file order, which tests/conftest.py
    keeps inside a rank; under a random-order plugin or pytest-xdist it would only run everything itself, more slowly."""
    for tag in sorted(CASES):
        if ("a", tag) not in RAN:
            _run(CASES[tag], 0xFF, px, "a")
    for tag in sorted(ABI):
        if ("b", tag) not in RAN:
            _run(ABI[tag], 0xFF, px, "b")
    for tag in sorted(FLOW_SHAPES):
        if ("e", tag) not in RAN:
            _run(flow_case(*FLOW_SHAPES[tag], "far"), 0xFF, px, "e")
    for tag in sorted(STEPS):
        if ("c", tag) not in RAN:
            del px.records[:]
            _step_passes(STEPS[tag], 0xFF)
            SEEN["c"].extend(px.records)
            guard.release()
    for tag in sorted(INFER):
        if ("c", tag) not in RAN:
            del px.records[:]
            _inference(INFER[tag][0], 0xFF, INFER[tag][1])
            SEEN["c"].extend(px.records)
            guard.release()
    del px.records[:]
    sig = _lib().SIGNATURES
    need = sorted(n for n in sig if guard.is_launching(n))
    everything = [r for sec in SEEN.values() for r in sec]
    clean = {n for n, cs in everything if "torch" not in cs}
    missing = [n for n in need if n not in clean]
    loose_ab = sorted({n for sec in ("a", "b", "e") for n, cs in SEEN[sec] if "torch" in cs})
    dev_c = [(n, c) for n, cs in SEEN["c"] for c in cs if c in ("guarded", "torch")]
    loose_c = [n for n, c in dev_c if c == "torch"]
    dev_all = sum(1 for _, cs in everything for c in cs if c in ("guarded", "torch"))
    rep = {"guard.coverage.entry_points_launching": len(need), "guard.coverage.entry_points_covered": len(need) - len(missing),
           "guard.coverage.device_pointer_arguments": dev_all, "guard.coverage.unguarded_in_ops_and_abi_cases": len(loose_ab),
           "guard.coverage.whole_steps.device_pointer_arguments": len(dev_c), "guard.coverage.whole_steps.unguarded": len(loose_c)}
    for n in set(loose_c):
        rep["guard.coverage.whole_steps.unguarded.%s" % n] = loose_c.count(n)
    note_many(rep)
    print("guard coverage: %d of %d launching entry points, %d device-pointer arguments seen; whole steps: %d of %d not guarded (%s)" % (
        len(need) - len(missing), len(need), dev_all, len(loose_c), len(dev_c),
        ", ".join("%s x%d" % (n, loose_c.count(n)) for n in sorted(set(loose_c))) or "none"))
    assert not missing, "entry points never called with all device pointers guarded: " + ", ".join(missing)
    assert not loose_ab, "per-op / ABI cases handed the library pointers outside every guarded buffer: " + ", ".join(loose_ab)
    assert len(loose_c) <= 0.05 * len(dev_c), (len(loose_c), len(dev_c))
