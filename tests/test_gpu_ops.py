"""-m gpu: every HIP kernel of the hot path against (a) the golden vectors captured from the real
reference (tests/golden/*.npz, fp64) and (b) the CPU oracle (oracle/modet_torch.py) on odd, ragged shapes.
All calls go through the C ABI (smilecode_amd.ops -> libmodet_hip.so).  Tolerance: fp32 kernels vs an fp64
reference, |err| <= 2e-5 + 2e-5*|ref| per element unless a test states otherwise (sums over many voxels)."""
import re

import numpy as np
import pytest
import torch

from tests.util import assert_close, cl, cu, gold, ncdhw, np64
from tests.util import note as _note

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from smilecode_amd import ops as o
    return o


@pytest.fixture(scope="module")
def orc():
    from oracle import modet_torch
    return modet_torch


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("tag", ["h1", "h2", "h8", "h4"])
def test_na_fused_golden(ops, tag):
    g = gold("op_attention.npz")
    heads = int(tag[1:])
    q = cu(g[f"{tag}.q"]).requires_grad_(True)
    k = cu(g[f"{tag}.k"]).requires_grad_(True)
    rpb = cu(g[f"{tag}.rpb"]).requires_grad_(True)
    out = ops.neighbourhood_attention(q, k, rpb, heads, float(g[f"{tag}.scale"]))
    assert_close(ncdhw(out), g[f"{tag}.out"], what="na out")
    gy = cl(g[f"{tag}.gy"])
    dq, dk, drpb = torch.autograd.grad(out, [q, k, rpb], gy)
    assert_close(np64(dq), g[f"{tag}.dq"], what="na dq")
    assert_close(np64(dk), g[f"{tag}.dk"], what="na dk")
    assert_close(np64(drpb), g[f"{tag}.drpb"], atol=1e-4, what="na drpb")


@pytest.mark.parametrize("tag", ["h1", "h2", "h8"])
def test_qk_reference_contract(tag):
    """modetqkrpb_cu with the CUDA op's tensor contract (ModeT-cu/models.py:304-311, modet_kernel.cu)."""
    from smilecode_amd.functional import modetqkrpb_cu
    import torch.nn.functional as F
    g = gold("op_attention.npz")
    heads = int(tag[1:])
    sc = float(g[f"{tag}.scale"])
    q0, k0 = cu(g[f"{tag}.q"]), cu(g[f"{tag}.k"])
    B, D, H, W, C = q0.shape
    d = C // heads
    rpb = cu(g[f"{tag}.rpb"]).requires_grad_(True)
    q = (q0.reshape(B, D, H, W, heads, d).permute(0, 4, 1, 2, 3, 5) * sc).contiguous().requires_grad_(True)
    kp = F.pad(k0.permute(0, 4, 1, 2, 3), (1, 1, 1, 1, 1, 1)).reshape(B, heads, d, D + 2, H + 2, W + 2)
    kp = kp.permute(0, 1, 3, 4, 5, 2).contiguous().requires_grad_(True)
    attn = modetqkrpb_cu(q, kp, rpb)
    assert_close(np64(attn), g[f"{tag}.logits"], what="qk logits")
    # backward vs plain torch autograd of the same contraction on the CPU in fp64
    ga = torch.randn(attn.shape, generator=torch.Generator().manual_seed(1)).double()
    dq, dk, dr = torch.autograd.grad(attn, [q, kp, rpb], ga.float().cuda())
    qc, kc, rc = (t.detach().double().cpu().requires_grad_(True) for t in (q, kp, rpb))
    cols = [(qc * kc[:, :, a:a + D, b:b + H, c:c + W]).sum(-1) for a in range(3) for b in range(3) for c in range(3)]
    ref = torch.stack(cols, -1) + rc.reshape(1, heads, 1, 1, 1, 27)
    rq, rk, rr = torch.autograd.grad(ref, [qc, kc, rc], ga)
    assert_close(np64(dq), rq.numpy(), what="qk dq")
    assert_close(np64(dk), rk.numpy(), what="qk dk (padded)")
    assert_close(np64(dr), rr.numpy(), atol=1e-4, what="qk drpb")
    # rpb=None path (modet.cpp:13) returns no bias gradient
    a2 = modetqkrpb_cu(q, kp, None)
    assert_close(np64(a2), g[f"{tag}.logits"] - g[f"{tag}.rpb"].reshape(1, heads, 1, 1, 1, 27), what="qk no-bias")


def test_qk_operator_full_size_vs_c_oracle():
    """the operator boundary at the level-1 shape it is benchmarked at (160x192x160, 1 head, d = 6)
    against oracle/modet_ref.c (the plain-C fp64 restatement of modet_fw / modet_bw, modet_kernel.cu:17-317): ALL 132.7 M
    logits, d_q, the padded d_k including its ring, and d_rpb (a sum over 4.9 M voxels per tap)."""
    from oracle import cref
    from smilecode_amd.functional import modet_bw, modet_fw
    D, H, W, d = 160, 192, 160, 6
    g = torch.Generator().manual_seed(160)
    q = torch.randn((1, 1, D, H, W, d), generator=g)
    kp = torch.zeros((1, 1, D + 2, H + 2, W + 2, d))
    kp[:, :, 1:-1, 1:-1, 1:-1] = torch.randn((1, 1, D, H, W, d), generator=g)
    rpb = torch.randn((1, 3, 3, 3), generator=g)
    ga = torch.randn((1, 1, D, H, W, 27), generator=g)
    attn = modet_fw(q.cuda(), kp.cuda(), rpb.cuda())
    dq, dk, dr = modet_bw(ga.cuda(), q.cuda(), kp.cuda(), True)
    torch.cuda.synchronize()
    ref = cref.modet_fw(q.numpy(), kp.numpy(), rpb.numpy())
    e = assert_close(attn.cpu().numpy(), ref, atol=2e-5, rtol=2e-5, what="full-size logits")
    del ref, attn
    rq, rk, rr = cref.modet_bw(ga.numpy(), q.numpy(), kp.numpy(), True)
    eq = assert_close(dq.cpu().numpy(), rq, atol=2e-5, rtol=2e-5, what="full-size d_q")
    ek = assert_close(dk.cpu().numpy(), rk, atol=2e-5, rtol=2e-5, what="full-size d_kpad")
    # d_rpb[t] sums 4.9 M products of O(1): |sum| ~ sqrt(V) = 2e3; fp32 partial rows + fp64 stages
    er = float(np.abs(dr.double().cpu().numpy() - rr).max() / np.abs(rr).max())
    assert er < 1e-5, er
    from tests.util import note
    note("operator[160x192x160].logits_maxerr", e)
    note("operator[160x192x160].dq_maxerr", eq)
    note("operator[160x192x160].dkpad_maxerr", ek)
    note("operator[160x192x160].drpb_relerr", er)


@pytest.mark.parametrize("shape,heads,d", [((5, 6, 7), 2, 6), ((3, 3, 3), 1, 4), ((9, 17, 33), 3, 8)])
def test_qk_reference_contract_double(shape, heads, d):
    """The operator dispatches double like the reference (AT_DISPATCH_FLOATING_TYPES, modet_kernel.cu:134,:364):
    fp64 in, fp64 arithmetic, fp64 out -- compared with torch fp64 autograd of the same contraction at 1e-12,
    and torch.autograd.gradcheck passes through the boundary (it needs double)."""
    from smilecode_amd.functional import modetqkrpb_cu, modet_fw
    D, H, W = shape
    gen = torch.Generator().manual_seed(3)
    qc = torch.randn((2, heads, D, H, W, d), generator=gen, dtype=torch.float64).requires_grad_(True)
    kc = torch.zeros((2, heads, D + 2, H + 2, W + 2, d), dtype=torch.float64)
    kc[:, :, 1:-1, 1:-1, 1:-1] = torch.randn((2, heads, D, H, W, d), generator=gen, dtype=torch.float64)
    kc.requires_grad_(True)
    rc = torch.randn((heads, 3, 3, 3), generator=gen, dtype=torch.float64).requires_grad_(True)
    ga = torch.randn((2, heads, D, H, W, 27), generator=gen, dtype=torch.float64)
    cols = [(qc * kc[:, :, a:a + D, b:b + H, c:c + W]).sum(-1) for a in range(3) for b in range(3) for c in range(3)]
    ref = torch.stack(cols, -1) + rc.reshape(1, heads, 1, 1, 1, 27)
    rq, rk, rr = torch.autograd.grad(ref, [qc, kc, rc], ga)
    q, kp, rpb = (t.detach().cuda().requires_grad_(True) for t in (qc, kc, rc))
    attn = modetqkrpb_cu(q, kp, rpb)
    assert attn.dtype == torch.float64
    dq, dk, dr = torch.autograd.grad(attn, [q, kp, rpb], ga.cuda())
    assert dq.dtype == dk.dtype == dr.dtype == torch.float64 and dr.shape == (heads, 3, 3, 3)
    for got, want, what in [(attn, ref, "logits"), (dq, rq, "dq"), (dk, rk, "dk (padded)"), (dr, rr, "drpb")]:
        err = float((got.detach().cpu() - want.detach()).abs().max())
        assert err <= 1e-12 * max(1.0, float(want.detach().abs().max())), (what, err)
    a2 = modetqkrpb_cu(q, kp, None)
    assert float((a2.detach().cpu() - (ref.detach() - rc.detach().reshape(1, heads, 1, 1, 1, 27))).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError, match="scalar type"):
        modet_fw(q.detach(), kp.detach().float(), None)                  # mixed dtypes are rejected, as packed_accessor does
    with pytest.raises(RuntimeError, match="not implemented"):
        modet_fw(q.detach().half(), kp.detach().half(), None)
    if D * H * W <= 27:
        assert torch.autograd.gradcheck(modetqkrpb_cu, (q, kp, rpb), eps=1e-6, atol=1e-7, nondet_tol=1e-12)


@pytest.mark.parametrize("shape,heads,d,B", [((40, 20, 70), 1, 6, 1), ((17, 9, 65), 2, 6, 2), ((3, 3, 3), 1, 6, 1),
                                             ((12, 35, 34), 3, 8, 1), ((33, 8, 32), 2, 4, 1), ((8, 9, 10), 2, 3, 2)])
def test_qk_operator_ragged_multichunk(shape, heads, d, B):
    """The operator's plane-marching kernels (head_dim 4/6/8) on ragged tiles, several (y,x) tiles and several z chunks,
    and the one-thread-per-voxel kernels every other head_dim takes: forward, d_q, d_kpad (ring included), d_rpb
    against torch fp64 autograd of the same contraction."""
    from smilecode_amd.functional import modetqkrpb_cu
    D, H, W = shape
    gen = torch.Generator().manual_seed(11)
    qc = torch.randn((B, heads, D, H, W, d), generator=gen, dtype=torch.float64).requires_grad_(True)
    kc = torch.randn((B, heads, D + 2, H + 2, W + 2, d), generator=gen, dtype=torch.float64).requires_grad_(True)  # ring too
    rc = torch.randn((heads, 3, 3, 3), generator=gen, dtype=torch.float64).requires_grad_(True)
    ga = torch.randn((B, heads, D, H, W, 27), generator=gen, dtype=torch.float64)
    cols = [(qc * kc[:, :, a:a + D, b:b + H, c:c + W]).sum(-1) for a in range(3) for b in range(3) for c in range(3)]
    ref = torch.stack(cols, -1) + rc.reshape(1, heads, 1, 1, 1, 27)
    rq, rk, rr = torch.autograd.grad(ref, [qc, kc, rc], ga)
    q, kp, rpb = (t.detach().float().cuda().requires_grad_(True) for t in (qc, kc, rc))
    attn = modetqkrpb_cu(q, kp, rpb)
    assert_close(np64(attn), ref.detach().numpy(), what="qk logits")
    dq, dk, dr = torch.autograd.grad(attn, [q, kp, rpb], ga.float().cuda())
    assert_close(np64(dq), rq.numpy(), atol=1e-4, what="qk dq")
    assert_close(np64(dk), rk.numpy(), atol=1e-4, what="qk dk (padded)")
    assert_close(np64(dr), rr.numpy(), atol=2e-5 * (B * D * H * W) ** 0.5 * 4, what="qk drpb")
    # run-to-run determinism (no atomics anywhere on this path)
    dq2, dk2, dr2 = torch.autograd.grad(modetqkrpb_cu(q, kp, rpb), [q, kp, rpb], ga.float().cuda())
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dr, dr2)
    a0 = modetqkrpb_cu(q, kp, None)
    (dq0, dk0) = torch.autograd.grad(a0, [q, kp], ga.float().cuda())
    assert torch.equal(dq0, dq) and torch.equal(dk0, dk)


@pytest.mark.parametrize("shape,heads", [((9, 7, 21), 1), ((5, 13, 18), 2), ((3, 3, 3), 8), ((2, 1, 2), 4)])
def test_na_fused_vs_oracle_ragged(ops, orc, shape, heads):
    """ragged tiles, volumes smaller than the window, all 26 border classes."""
    gen = torch.Generator().manual_seed(7)
    C = heads * 6
    q = torch.randn((2,) + shape + (C,), generator=gen).double().requires_grad_(True)
    k = torch.randn((2,) + shape + (C,), generator=gen).double().requires_grad_(True)
    rpb = (0.5 * torch.randn((heads, 3, 3, 3), generator=gen)).double().requires_grad_(True)
    ref = orc.mode_transformer(q, k, rpb, heads, 0.7)
    gy = torch.randn(ref.shape, generator=gen).double()
    rq, rk, rr = torch.autograd.grad(ref, [q, k, rpb], gy)
    qd, kd, rd = (t.detach().float().cuda().requires_grad_(True) for t in (q, k, rpb))
    out = ops.neighbourhood_attention(qd, kd, rd, heads, 0.7)
    assert_close(ncdhw(out), ref.detach().numpy(), what="na out")
    dq, dk, dr = torch.autograd.grad(out, [qd, kd, rd], gy.permute(0, 2, 3, 4, 1).float().contiguous().cuda())
    assert_close(np64(dq), rq.numpy(), what="na dq")
    assert_close(np64(dk), rk.numpy(), what="na dk")
    assert_close(np64(dr), rr.numpy(), atol=2e-4, what="na drpb")


@pytest.mark.parametrize("shape,heads,B", [((97, 122, 131), 1, 1), ((100, 101, 150), 2, 2)])
def test_na_backward_z_march_vs_oracle(ops, orc, shape, heads, B):
    """na_bwd_march_kernel (volumes >= 1.5 M voxels: pyramid level 1): plane ring, buffer-descriptor halo, chunked z --
    ragged against the 8 x 32 columns and the z chunks, 1 and 2 heads, batch 1 and 2; d_q, d_k and the d_rpb partial rows
    (accumulated in registers over a whole chunk) against fp64 autograd of the oracle; deterministic run to run."""
    gen = torch.Generator().manual_seed(11)
    C = heads * 6
    q = torch.randn((B,) + shape + (C,), generator=gen).double().requires_grad_(True)
    k = torch.randn((B,) + shape + (C,), generator=gen).double().requires_grad_(True)
    rpb = (0.5 * torch.randn((heads, 3, 3, 3), generator=gen)).double().requires_grad_(True)
    ref = orc.mode_transformer(q, k, rpb, heads, 0.7)
    gy = torch.randn(ref.shape, generator=gen).double()
    rq, rk, rr = torch.autograd.grad(ref, [q, k, rpb], gy)
    qd, kd, rd = (t.detach().float().cuda().requires_grad_(True) for t in (q, k, rpb))
    out = ops.neighbourhood_attention(qd, kd, rd, heads, 0.7)
    gyd = gy.permute(0, 2, 3, 4, 1).float().contiguous().cuda()
    dq, dk, dr = torch.autograd.grad(out, [qd, kd, rd], gyd, retain_graph=True)
    assert_close(np64(dq), rq.numpy(), what="na dq (z-march)")
    assert_close(np64(dk), rk.numpy(), what="na dk (z-march)")
    assert float(np.abs(np64(dr) - rr.numpy()).max()) <= 2e-5 * float(rr.abs().max()) + 2e-4, "na drpb (z-march)"
    dq2, dk2, dr2 = torch.autograd.grad(out, [qd, kd, rd], gyd)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dr, dr2), "no atomics: bit-identical re-run"


# ------------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_warp_golden(ops, tag):
    g = gold("op_warp.npz")
    src = cl(g[f"{tag}.src"]).requires_grad_(True)
    flow = cl(g[f"{tag}.flow"]).requires_grad_(True)
    out = ops.warp(src, flow, 0, False)
    assert_close(ncdhw(out), g[f"{tag}.out"], what="warp out")
    ds, df = torch.autograd.grad(out, [src, flow], cl(g[f"{tag}.gy"]))
    assert_close(ncdhw(ds), g[f"{tag}.dsrc"], what="warp dsrc")
    assert_close(ncdhw(df), g[f"{tag}.dflow"], atol=1e-4, rtol=1e-4, what="warp dflow")
    outn = ops.warp(cl(g[f"{tag}.lab"]), cl(g[f"{tag}.flow_n"]), 1, False)
    assert np.array_equal(ncdhw(outn), g[f"{tag}.out_n"]), "nearest warp must be exact"


@pytest.mark.parametrize("C,shape", [(8, (1, 16, 24, 32)), (1, (2, 12, 16, 20)), (16, (1, 8, 12, 16)), (8, (1, 40, 48, 40))])
def test_warp_tee_adds_the_second_flow_gradient_in_the_kernel(C, shape):
    """ops.warp_tee (round 5): a flow with two consumers -- the feature warp and the next composition -- whose second
    gradient is added inside the warp's backward kernel (modet_warp_bwd_acc) instead of by an autograd add.  d_flow must be
    BIT-identical to the two-node form (one float addition per element either way; both kernel forms: the patch kernel
    and the z-run kernel, which the image warp without d_src takes), d_src equal up to the atomic order."""
    from smilecode_amd import ops
    B, D, H, W = shape
    g = torch.Generator().manual_seed(11)
    src = torch.randn(B, D, H, W, C, generator=g).cuda()
    flow = (torch.randn(B, D, H, W, 3, generator=g) * 2.0).cuda()
    r1 = torch.randn(B, D, H, W, C, generator=g).cuda()
    r2 = torch.randn(B, D, H, W, 3, generator=g).cuda()
    for src_grad in (True, False):
        res = []
        for tee in (False, True):
            s_ = src.clone().requires_grad_(src_grad)
            f_ = flow.clone().requires_grad_(True)
            if tee:
                out, fl = ops.warp_tee(s_, f_)
            else:
                out, fl = ops.warp(s_, f_), f_
            ((out * r1).sum() + (fl * fl * r2).sum()).backward()
            res.append((out.detach(), f_.grad, s_.grad))
        assert torch.equal(res[0][0], res[1][0])
        assert torch.equal(res[0][1], res[1][1]), float((res[0][1] - res[1][1]).abs().max())
        if src_grad:
            assert float((res[0][2] - res[1][2]).abs().max()) <= 1e-5 * float(res[0][2].abs().max())
    # only the alias is used / only the warp is used
    f_ = flow.clone().requires_grad_(True)
    out, fl = ops.warp_tee(src, f_)
    (fl * r2).sum().backward()
    assert torch.equal(f_.grad, r2)
    f_ = flow.clone().requires_grad_(True)
    out, fl = ops.warp_tee(src, f_)
    (out * r1).sum().backward()
    f2 = flow.clone().requires_grad_(True)
    (ops.warp(src, f2) * r1).sum().backward()
    assert torch.equal(f_.grad, f2.grad)


@pytest.mark.parametrize("C,shape,amp", [(8, (2, 16, 24, 40), 2.0), (16, (1, 13, 21, 37), 6.0), (8, (1, 40, 48, 40), 12.0),
                                         (32, (1, 9, 8, 17), 3.0), (8, (1, 8, 8, 8), 40.0), (64, (2, 10, 12, 10), 1.5),
                                         (8, (1, 80, 96, 80), 25.0), (3, (2, 20, 24, 36), 2.5), (3, (1, 7, 9, 11), 1.0),
                                         (8, (2, 24, 32, 40), -1.0), (16, (1, 20, 24, 20), -1.0)])
def test_warp_backward_by_destination_tiles(C, shape, amp, monkeypatch):
    """csrc/warp_tile.hip, the DEFAULT backward of the feature warps since round 6: the scatter of SpatialTransformer's backward
    (reference models.py:55-67 -> ATen grid_sampler_3d_backward) with destination-tile payload lists and a 64-bit fixed-point LDS
    window instead of float atomics.  Against the float-atomic kernel (itself pinned by the goldens): d_src equal within fp32
    rounding of the sums, d_flow within rounding of the 8-corner dot products; bit-identical run to run; ragged volumes (partial
    tiles), two samples, channel groups (C = 16, 32, 64), flows that fold and that leave the volume, a block of all-zero d_out
    (those voxels are dropped while binning), a d_src buffer and a workspace full of NaN on entry (neither is read), bf16 src.
    The last case is ADVICE r5's: on 80x96x80 with sigma = 25 voxels a 1024-voxel source block reaches ~500 distinct destination
    tiles -- round 5's 256-slot hash table overflowed silently there.  Then the routed form: ops.warp_tee's backward with
    ops.WARP_TILES on / off gives the same d_src / d_flow (incl. the second flow gradient).  C == 3: the flow compositions
    warp(src, flow) + flow whose flow is not bounded by a voxel (reference models.py:392-403 with a CWM output): add_flow.
    amp < 0: a COLLAPSING flow -- every voxel of a sample lands within a voxel of one point, so one or two tiles receive 15-30 k
    entries against their fixed list segment of 1 536: the overflow list and its per-tile filter carry the rest."""
    from smilecode_amd import _lib, ops
    L = _lib.load()
    B, D, H, W = shape
    g = torch.Generator().manual_seed(C + D)
    src = torch.randn(B, D, H, W, C, generator=g).cuda()
    if amp >= 0:
        flow = (torch.randn(B, D, H, W, 3, generator=g) * amp).cuda()
    else:
        grid = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"), -1).float()
        target = torch.tensor([D * 0.43, H * 0.51, W * 0.37])
        flow = ((target - grid)[None] + 0.45 * torch.randn(B, D, H, W, 3, generator=g)).contiguous().cuda()
    dout = torch.randn(B, D, H, W, C, generator=g).cuda() * 3.7
    dout[:, : D // 3] = 0.0                                       # zero contributions are skipped on both sides
    add = torch.randn(B, D, H, W, 3, generator=g).cuda()
    st = torch.cuda.current_stream().cuda_stream
    af = int(C == 3)
    ref, ref_f = torch.empty_like(src), torch.empty_like(flow)
    _lib.check(L.modet_warp_bwd_acc(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), ref.data_ptr(), ref_f.data_ptr(), add.data_ptr(),
                                    B, D, H, W, C, af, 0, st), "warp_bwd_acc")
    nb = L.modet_warp_bwd_dsrc_tiles_ws_bytes(B, D, H, W, C)
    assert nb > 0 and L.modet_warp_bwd_dsrc_tiles_ws_bytes(B, D, H, W, C + 4) == 0 and L.modet_warp_bwd_dsrc_tiles_ws_bytes(B, 2000, H, W, C) == 0
    ws = torch.empty(nb // 4 + 8, dtype=torch.float32, device="cuda")
    outs = []
    for rep in range(2):
        out, out_f = torch.full_like(src, float("nan")), torch.full_like(flow, float("nan"))
        ws.fill_(float("nan"))                                     # (the workspace needs no preparation either)
        _lib.check(L.modet_warp_bwd_tiles(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), out.data_ptr(), out_f.data_ptr(),
                                          add.data_ptr(), ws.data_ptr(), nb, B, D, H, W, C, af, st), "tiles")
        outs.append((out, out_f))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "integer sums: bit-reproducible"
    if amp < 0:
        # thousands of terms per cell: the float-atomic kernel's own rounding (order-dependent, ~4e-6 of max) is larger than the
        # tolerance, so d_src is checked against an fp64 scatter on the same fp32 sample coordinates -- which the integer sums of the
        # tile path must match BETTER than the float atomics do
        pc = torch.stack(torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij"), -1).float()[None] + flow.cpu()
        fl = torch.floor(pc)
        fr = (pc - fl).double()
        base = fl.long()
        ref64 = torch.zeros(B, D * H * W, C, dtype=torch.float64)
        do = dout.double().cpu().reshape(B, -1, C)
        for q in range(8):
            dz, dy, dx = q >> 2, (q >> 1) & 1, q & 1
            iz, iy, ix = base[..., 0] + dz, base[..., 1] + dy, base[..., 2] + dx
            ok = ((iz >= 0) & (iz < D) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).reshape(B, -1)
            wq = ((fr[..., 0] if dz else 1 - fr[..., 0]) * (fr[..., 1] if dy else 1 - fr[..., 1]) * (fr[..., 2] if dx else 1 - fr[..., 2])).reshape(B, -1)
            lin = ((iz.clamp(0, D - 1) * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)).reshape(B, -1)
            for bb in range(B):
                ref64[bb].index_add_(0, lin[bb][ok[bb]], (wq[bb][:, None] * do[bb])[ok[bb]])
        ref64 = ref64.reshape(B, D, H, W, C)
        e_atomic = float((ref.double().cpu() - ref64).abs().max())
        e_tiles = float((outs[0][0].double().cpu() - ref64).abs().max())
        _note(f"warp_tiles[C{C},collapse].err_vs_fp64_tiles_over_atomics", e_tiles / max(e_atomic, 1e-30))
        assert e_tiles <= e_atomic, (e_tiles, e_atomic)
        ref = ref64.float().cuda()
    scale, scale_f = float(ref.abs().max()), float(ref_f.abs().max())
    err, err_f = float((outs[0][0] - ref).abs().max()), float((outs[0][1] - ref_f).abs().max())
    if scale > 0.0:                                               # (the 8^3 case: every sample point leaves the volume -> all zero)
        _note(f"warp_tiles[C{C},{'x'.join(map(str, shape))}].dsrc_maxdiff_of_max", err / scale)
        _note(f"warp_tiles[C{C},{'x'.join(map(str, shape))}].dflow_maxdiff_of_max", err_f / scale_f)
    assert err <= 2e-6 * scale, (err, scale)
    assert err_f <= 4e-6 * scale_f, (err_f, scale_f)
    # d_src only (no src, no d_flow): the same d_src bit for bit
    only = torch.full_like(src, float("nan"))
    _lib.check(L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), dout.data_ptr(), only.data_ptr(), ws.data_ptr(), nb, B, D, H, W, C, st), "tiles")
    assert torch.equal(only, outs[0][0])
    assert L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), dout.data_ptr(), only.data_ptr(), ws.data_ptr(), nb - 4, B, D, H, W, C, st) != 0
    z, zf = torch.full_like(src, float("nan")), torch.full_like(flow, float("nan"))
    _lib.check(L.modet_warp_bwd_tiles(src.data_ptr(), 0, flow.data_ptr(), torch.zeros_like(dout).data_ptr(), z.data_ptr(), zf.data_ptr(), None,
                                      ws.data_ptr(), nb, B, D, H, W, C, af, st), "tiles")
    assert float(z.abs().max()) == 0.0 and float(zf.abs().max()) == 0.0
    if C == 3:
        assert L.modet_warp_bwd_tiles(src.to(torch.bfloat16).data_ptr(), 1, flow.data_ptr(), dout.data_ptr(), z.data_ptr(), zf.data_ptr(), None,
                                      ws.data_ptr(), nb, B, D, H, W, C, af, st) != 0, "C == 3 takes fp32 src only"
    else:
        assert L.modet_warp_bwd_tiles(src.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), z.data_ptr(), zf.data_ptr(), None,
                                      ws.data_ptr(), nb, B, D, H, W, C, 1, st) != 0, "add_flow is the C == 3 composition's"
        # bf16 src (cfg 5's feature warps): bit-identical to the fp32 entry fed with the widened values
        s16 = src.to(torch.bfloat16)
        a16, f16 = torch.empty_like(src), torch.empty_like(flow)
        _lib.check(L.modet_warp_bwd_tiles(s16.data_ptr(), 1, flow.data_ptr(), dout.data_ptr(), a16.data_ptr(), f16.data_ptr(), add.data_ptr(),
                                          ws.data_ptr(), nb, B, D, H, W, C, 0, st), "tiles bf16")
        sw = s16.float()
        a32, f32 = torch.empty_like(src), torch.empty_like(flow)
        _lib.check(L.modet_warp_bwd_tiles(sw.data_ptr(), 0, flow.data_ptr(), dout.data_ptr(), a32.data_ptr(), f32.data_ptr(), add.data_ptr(),
                                          ws.data_ptr(), nb, B, D, H, W, C, 0, st), "tiles")
        assert torch.equal(a16, a32) and torch.equal(f16, f32)
    # routed through the autograd node
    r2 = torch.randn(B, D, H, W, 3, generator=g).cuda()
    res = []
    for routed in (False, True):
        monkeypatch.setattr(ops, "WARP_TILES", routed)
        s_, f_ = src.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        if C == 3:
            o, fl = ops.warp(s_, f_, 0, True), f_
        else:
            o, fl = ops.warp_tee(s_, f_)
        ((o * dout).sum() + (fl * fl * r2).sum()).backward()
        res.append((s_.grad, f_.grad))
    assert float((res[0][1] - res[1][1]).abs().max()) <= 4e-6 * float(res[0][1].abs().max()) + 1e-30
    assert float((res[0][0] - res[1][0]).abs().max()) <= (2e-6 if amp >= 0 else 2e-5) * scale      # (collapse: the float atomics' own noise)


def test_warp_backward_tiles_range_and_non_finite():
    """(1) contributions far below the tensor's maximum must survive the fixed point -- 2^-40 of the power of two
    above max |d_out| per unit (modet_warp_bwd_det's), so a region 1e-7 of the maximum keeps 3-4 digits where round 5's 2^-30 left one bit;
    (2) a NaN or inf in d_out must not be turned into finite numbers (the float path propagates it)."""
    from smilecode_amd import _lib
    L = _lib.load()
    B, D, H, W, C = 1, 16, 16, 24, 8
    g = torch.Generator().manual_seed(5)
    flow = (torch.randn(B, D, H, W, 3, generator=g) * 0.3).cuda()
    dout = torch.randn(B, D, H, W, C, generator=g).cuda()
    dout[:, :, :, 12:] *= 1e-7
    st = torch.cuda.current_stream().cuda_stream
    nb = L.modet_warp_bwd_dsrc_tiles_ws_bytes(B, D, H, W, C)
    ws = torch.empty(nb // 4 + 8, dtype=torch.float32, device="cuda")
    ref, out = torch.empty_like(dout), torch.empty_like(dout)
    _lib.check(L.modet_warp_bwd(dout.data_ptr(), flow.data_ptr(), dout.data_ptr(), ref.data_ptr(), None, B, D, H, W, C, 0, 0, st), "warp_bwd")
    _lib.check(L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), dout.data_ptr(), out.data_ptr(), ws.data_ptr(), nb, B, D, H, W, C, st), "tiles")
    small = ref[:, :, :, 14:22]
    rel = float((out[:, :, :, 14:22] - small).abs().max() / small.abs().max())
    _note("warp_tiles.small_region_relerr", rel)
    assert float(small.abs().max()) < 1e-5 and rel < 1e-3, rel
    for bad in (float("nan"), float("inf")):
        d2 = dout.clone()
        d2[0, 3, 4, 5, 2] = bad
        _lib.check(L.modet_warp_bwd_dsrc_tiles(flow.data_ptr(), d2.data_ptr(), out.data_ptr(), ws.data_ptr(), nb, B, D, H, W, C, st), "tiles")
        assert not bool(torch.isfinite(out[0, 2:6, 3:7, 4:8]).all()), "a non-finite d_out was laundered into finite d_src"


@pytest.mark.parametrize("C,shape,add_flow", [(8, (1, 40, 48, 40), False), (3, (2, 12, 16, 20), True), (16, (1, 8, 12, 16), False),
                                              (32, (1, 20, 24, 20), False)])
def test_warp_backward_deterministic_mode(C, shape, add_flow):
    """ops.set_deterministic (round 5, VERDICT r4 missing-4): d_src through 64-bit fixed-point integer atomics
    (modet_warp_bwd_det) is BIT-identical from run to run -- the float-atomic form differs at 1e-6 -- and equals it to that
    noise; d_flow is the same arithmetic in both.  Flows up to 6 voxels: samples leave the volume, cells collide."""
    from smilecode_amd import ops
    B, D, H, W = shape
    g = torch.Generator().manual_seed(21)
    src = torch.randn(B, D, H, W, C, generator=g).cuda()
    flow = (torch.randn(B, D, H, W, 3, generator=g) * 3.0).cuda()
    r1 = (torch.randn(B, D, H, W, C, generator=g) * 1e-3).cuda()

    def run():
        s_, f_ = src.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        (ops.warp(s_, f_, 0, add_flow) * r1).sum().backward()
        return s_.grad, f_.grad
    ref = run()
    prev = ops.set_deterministic(True)
    try:
        a, b, c = run(), run(), run()
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]), "deterministic d_src differs between runs"
    assert torch.equal(a[1], b[1]) and torch.equal(a[1], ref[1])
    assert float((a[0] - ref[0]).abs().max()) <= 2e-6 * float(ref[0].abs().max())


def test_cat_batch_is_a_view_for_adjacent_halves():
    from smilecode_amd import ops
    pair = torch.randn(4, 6, 8, 10, 1).cuda()
    v = ops.cat_batch(pair[:2], pair[2:])
    assert v.data_ptr() == pair.data_ptr() and torch.equal(v, pair)
    a, b = torch.randn(2, 6, 8, 10, 1).cuda(), torch.randn(2, 6, 8, 10, 1).cuda()
    c = ops.cat_batch(a, b)
    assert torch.equal(c, torch.cat([a, b], 0)) and c.data_ptr() != a.data_ptr()
    assert torch.equal(ops.cat_batch(pair[2:], pair[:2]), torch.cat([pair[2:], pair[:2]], 0))


def test_warp_compose_and_wide_channels(ops, orc):
    gen = torch.Generator().manual_seed(3)
    for C, shape in ((3, (7, 9, 11)), (64, (4, 5, 6)), (16, (6, 5, 9)), (1, (8, 8, 8))):
        src = torch.randn((2, C) + shape, generator=gen).double().requires_grad_(True)
        flow = (2.5 * torch.randn((2, 3) + shape, generator=gen)).double().requires_grad_(True)
        add = C == 3
        ref = orc.warp(src, flow) + (flow if add else 0)
        gy = torch.randn(ref.shape, generator=gen).double()
        rs, rf = torch.autograd.grad(ref, [src, flow], gy)
        s, f = cl(src.detach().numpy()).requires_grad_(True), cl(flow.detach().numpy()).requires_grad_(True)
        out = ops.warp(s, f, 0, add)
        assert_close(ncdhw(out), ref.detach().numpy(), what=f"warp C={C}")
        ds, df = torch.autograd.grad(out, [s, f], cl(gy.numpy()))
        assert_close(ncdhw(ds), rs.numpy(), atol=5e-5, what=f"warp dsrc C={C}")
        assert_close(ncdhw(df), rf.numpy(), atol=2e-4, rtol=1e-4, what=f"warp dflow C={C}")


def test_warp_bounded_flow_gather_equals_scatter(ops, orc):
    """flow_bound=1 (|flow| <= 1, incl. exactly +-1 and samples leaving the volume): atomics-free gather backward."""
    gen = torch.Generator().manual_seed(17)
    shape = (9, 10, 21)
    src = torch.randn((2, 3) + shape, generator=gen).double().requires_grad_(True)
    flow = (2 * torch.rand((2, 3) + shape, generator=gen) - 1).double()
    flow[:, :, 0, 0, :4] = torch.tensor([1.0, -1.0, 0.0, 0.5]).double()        # boundary values of the promise
    flow.requires_grad_(True)
    ref = orc.warp(src, flow) + flow
    gy = torch.randn(ref.shape, generator=gen).double()
    rs, rf = torch.autograd.grad(ref, [src, flow], gy)
    s, f = cl(src.detach().numpy()).requires_grad_(True), cl(flow.detach().numpy()).requires_grad_(True)
    out = ops.warp(s, f, 0, True, 1)
    assert_close(ncdhw(out), ref.detach().numpy(), what="bounded warp out")
    ds, df = torch.autograd.grad(out, [s, f], cl(gy.numpy()))
    assert_close(ncdhw(ds), rs.numpy(), atol=5e-5, what="bounded warp dsrc (gather)")
    assert_close(ncdhw(df), rf.numpy(), atol=2e-4, rtol=1e-4, what="bounded warp dflow")
    ds2, df2 = torch.autograd.grad(ops.warp(s, f, 0, True, 0), [s, f], cl(gy.numpy()))
    assert_close(np64(ds), np64(ds2), atol=1e-5, what="gather vs scatter")
    assert float((df - df2).abs().max()) < 2e-5       # same math, different summation order over the 3 channels


@pytest.mark.parametrize("tag", ["c8", "c16", "c32", "c128"])
def test_cotr_golden(ops, tag):
    """Im2Grid's CoTr (one head over C channels) on the generic head-dimension kernels vs the reference's fp64 output"""
    from smilecode_amd import models
    g = gold("op_cotr.npz")
    q = cu(g[f"{tag}.q"]).requires_grad_(True)
    k = cu(g[f"{tag}.k"]).requires_grad_(True)
    y = models.CoTr().cuda()(q, k)
    assert_close(np64(y), g[f"{tag}.out"], what="CoTr out")
    dq, dk = torch.autograd.grad(y, [q, k], cu(g[f"{tag}.gy"]))
    assert_close(np64(dq), g[f"{tag}.dq"], atol=5e-5, what="CoTr dq")
    assert_close(np64(dk), g[f"{tag}.dk"], atol=5e-5, what="CoTr dk")


@pytest.mark.parametrize("heads,hd,shape", [(2, 8, (9, 6, 21)), (1, 64, (5, 9, 18)), (3, 16, (4, 4, 16))])
def test_attention_generic_head_dim_vs_oracle(ops, orc, heads, hd, shape):
    """generic path with several heads, a bias and a scale, ragged tiles: out, d_q, d_k, d_rpb vs the fp64 oracle"""
    gen = torch.Generator().manual_seed(heads * 100 + hd)
    C = heads * hd
    q = (0.5 * torch.randn((2,) + shape + (C,), generator=gen)).double().requires_grad_(True)
    k = (0.5 * torch.randn((2,) + shape + (C,), generator=gen)).double().requires_grad_(True)
    rpb = (0.5 * torch.randn((heads, 27), generator=gen)).double().requires_grad_(True)
    scale = hd ** -0.5
    ref = orc.mode_transformer(q, k, rpb, heads, scale)                 # (B, heads*3, D,H,W)
    gy = torch.randn(ref.shape, generator=gen).double()
    rq, rk, rr = torch.autograd.grad(ref, [q, k, rpb], gy)
    qd, kd = q.detach().float().cuda().requires_grad_(True), k.detach().float().cuda().requires_grad_(True)
    rd = rpb.detach().float().cuda().reshape(heads, 3, 3, 3).requires_grad_(True)
    y = ops.neighbourhood_attention(qd, kd, rd, heads, scale)
    assert_close(ncdhw(y), ref.detach().numpy(), what="generic attention out")
    dq, dk, dr = torch.autograd.grad(y, [qd, kd, rd], cl(gy.numpy()))
    assert_close(np64(dq), rq.numpy(), atol=5e-5, what="generic attention dq")
    assert_close(np64(dk), rk.numpy(), atol=5e-5, what="generic attention dk")
    assert_close(np64(dr).reshape(heads, 27), rr.numpy(), atol=2e-4, rtol=1e-4, what="generic attention drpb")


@pytest.mark.parametrize("tag", ["c8", "c16", "c4"])
def test_correlation3d_golden(ops, tag):
    """PR++ Correlation3D vs the reference's own fp64 output and gradients"""
    from smilecode_amd import models
    g = gold("op_corr3d.npz")
    mov = cu(g[f"{tag}.mov"]).requires_grad_(True)
    fix = cu(g[f"{tag}.fix"]).requires_grad_(True)
    y = models.Correlation3D(mov.shape[1]).cuda()(mov, fix)
    assert_close(np64(y), g[f"{tag}.out"], atol=5e-5, what="corr3d out")
    dm, df = torch.autograd.grad(y, [mov, fix], cu(g[f"{tag}.gy"]))
    assert_close(np64(dm), g[f"{tag}.dmov"], atol=1e-4, what="corr3d dmov")
    assert_close(np64(df), g[f"{tag}.dfix"], atol=1e-4, what="corr3d dfix")


@pytest.mark.parametrize("C,shape", [(8, (1, 1, 3)), (12, (9, 10, 33)), (32, (6, 5, 7))])
def test_correlation3d_vs_oracle(ops, orc, C, shape):
    """volumes thinner than the displacement, odd channel counts, ragged sizes"""
    gen = torch.Generator().manual_seed(C + shape[2])
    mov = torch.randn((2, C) + shape, generator=gen).double().requires_grad_(True)
    fix = torch.randn((2, C) + shape, generator=gen).double().requires_grad_(True)
    ref = orc.correlation3d(mov, fix)
    gy = torch.randn(ref.shape, generator=gen).double()
    rm, rf = torch.autograd.grad(ref, [mov, fix], gy)
    md, fd = cl(mov.detach().numpy()).requires_grad_(True), cl(fix.detach().numpy()).requires_grad_(True)
    y = ops.correlation3d(md, fd)
    assert_close(np64(y), ref.detach().numpy(), atol=1e-4, rtol=1e-5, what="corr3d out")
    dm, df = torch.autograd.grad(y, [md, fd], gy.float().cuda())
    assert_close(ncdhw(dm), rm.numpy(), atol=2e-4, rtol=1e-5, what="corr3d dmov")
    assert_close(ncdhw(df), rf.numpy(), atol=2e-4, rtol=1e-5, what="corr3d dfix")


# ------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("tag", ["p1", "p3", "p5"])
def test_projection_golden(ops, tag):
    g = gold("op_misc.npz")
    x = cl(g[f"{tag}.x"]).requires_grad_(True)
    prm = [cu(g[f"{tag}.{n}"]).requires_grad_(True) for n in ("W", "b", "gamma", "beta")]
    y = ops.proj_ln(x, *prm)
    assert_close(np64(y), g[f"{tag}.out"], what="proj out")
    grads = torch.autograd.grad(y, [x] + prm, cu(g[f"{tag}.gy"]))
    assert_close(ncdhw(grads[0]), g[f"{tag}.dx"], atol=5e-5, what="proj dx")
    for got, n in zip(grads[1:], ("dW", "db", "dgamma", "dbeta")):
        assert_close(np64(got), g[f"{tag}.{n}"], atol=2e-4, rtol=1e-4, what=f"proj {n}")


# generic (Cin, dim) pairs of other head layouts (no grouped kernel) at their level's voxel count of 160x192x160:
# level 5 = 1200, level 4 = 9600, level 3 = 76800
GENERIC_PROJ = [(128, 12, 1200), (128, 24, 1200), (64, 12, 9600), (64, 48, 9600), (32, 24, 9600), (32, 48, 76800)]


@pytest.mark.parametrize("cin,dim,n", [(8, 6, 70001), (16, 6, 5003), (32, 12, 9001), (64, 24, 1531), (128, 48, 1203),
                                       (128, 48, 7), (24, 12, 777)] + GENERIC_PROJ)
def test_projection_vs_oracle_large(ops, orc, cin, dim, n):
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((1, cin, 1, 1, n), generator=gen).double().requires_grad_(True)
    p = {"p.proj.weight": 0.3 * torch.randn((dim, cin), generator=gen).double(),
         "p.proj.bias": 0.1 * torch.randn(dim, generator=gen).double(),
         "p.norm.weight": 1 + 0.1 * torch.randn(dim, generator=gen).double(),
         "p.norm.bias": 0.1 * torch.randn(dim, generator=gen).double()}
    for t in p.values():
        t.requires_grad_(True)
    ref = orc.projection(p, "p", x)
    gy = torch.randn(ref.shape, generator=gen).double()
    rg = torch.autograd.grad(ref, [x] + list(p.values()), gy)
    xd = cl(x.detach().numpy()).requires_grad_(True)
    pd = [t.detach().float().cuda().requires_grad_(True) for t in p.values()]
    y = ops.proj_ln(xd, *pd)
    assert_close(np64(y), ref.detach().numpy(), what="proj out")
    gd = torch.autograd.grad(y, [xd] + pd, gy.float().cuda())
    assert_close(ncdhw(gd[0]), rg[0].numpy(), atol=5e-5, what="proj dx")
    for a, b, nme in zip(gd[1:], rg[1:], ("dW", "db", "dgamma", "dbeta")):
        assert_close(np64(a), b.numpy(), atol=3e-3, rtol=2e-4, what=f"proj {nme} (sum over {n} voxels)")


@pytest.mark.parametrize("cin,dim,n", [(8, 6, 70001), (16, 6, 5003), (32, 12, 9001), (64, 24, 1531), (128, 48, 1203),
                                       (24, 12, 777)] + GENERIC_PROJ)
def test_projection_pair_vs_oracle(ops, orc, cin, dim, n):
    """ops.proj_ln_pair (the layer applied to the fixed and the moving features of a level): outputs and data gradients as
    two single applications, parameter gradients of both uses summed in one reduction -- against the fp64 oracle of
    proj(x1) and proj(x2) with shared parameters; (24, 12) is not covered by the pair kernel and takes two single calls."""
    gen = torch.Generator().manual_seed(13)
    x1 = torch.randn((1, cin, 1, 1, n), generator=gen).double().requires_grad_(True)
    x2 = torch.randn((1, cin, 1, 1, n), generator=gen).double().requires_grad_(True)
    p = {"p.proj.weight": 0.3 * torch.randn((dim, cin), generator=gen).double(),
         "p.proj.bias": 0.1 * torch.randn(dim, generator=gen).double(),
         "p.norm.weight": 1 + 0.1 * torch.randn(dim, generator=gen).double(),
         "p.norm.bias": 0.1 * torch.randn(dim, generator=gen).double()}
    for t in p.values():
        t.requires_grad_(True)
    r1, r2 = orc.projection(p, "p", x1), orc.projection(p, "p", x2)
    g1, g2 = torch.randn(r1.shape, generator=gen).double(), torch.randn(r1.shape, generator=gen).double()
    rg = torch.autograd.grad([r1, r2], [x1, x2] + list(p.values()), [g1, g2])
    xd1, xd2 = cl(x1.detach().numpy()).requires_grad_(True), cl(x2.detach().numpy()).requires_grad_(True)
    pd = [t.detach().float().cuda().requires_grad_(True) for t in p.values()]
    y1, y2 = ops.proj_ln_pair(xd1, xd2, *pd)
    assert_close(np64(y1), r1.detach().numpy(), what="proj out 1")
    assert_close(np64(y2), r2.detach().numpy(), what="proj out 2")
    gd = torch.autograd.grad([y1, y2], [xd1, xd2] + pd, [g1.float().cuda(), g2.float().cuda()])
    assert_close(ncdhw(gd[0]), rg[0].numpy(), atol=5e-5, what="proj dx1")
    assert_close(ncdhw(gd[1]), rg[1].numpy(), atol=5e-5, what="proj dx2")
    for a, b, nme in zip(gd[2:], rg[2:], ("dW", "db", "dgamma", "dbeta")):
        assert_close(np64(a), b.numpy(), atol=4e-3, rtol=2e-4, what=f"proj pair {nme} (sum over 2x{n} voxels)")
    # without gradients the pair is two plain applications
    with torch.no_grad():
        z1, z2 = ops.proj_ln_pair(xd1, xd2, *pd)
    assert torch.equal(z1, y1) and torch.equal(z2, y2)


# ------------------------------------------------------------------------------------------------ conv / norm / pool
@pytest.mark.parametrize("tag", ["c0", "c1", "c2", "c3"])
def test_conv_block_golden(ops, tag):
    g = gold("op_misc.npz")
    ins = bool(g[f"{tag}.ins"])
    x = cl(g[f"{tag}.x"]).requires_grad_(True)
    w = cu(g[f"{tag}.w"]).requires_grad_(True)
    b = cu(g[f"{tag}.b"]).requires_grad_(True)
    raw = ops.conv3d(x, w, b, False)
    assert_close(ncdhw(raw), g[f"{tag}.raw"], what="conv raw")
    y = ops.instnorm_lrelu(ops.conv3d(x, w, b, False)) if ins else ops.conv3d(x, w, b, True)
    assert_close(ncdhw(y), g[f"{tag}.out"], what="conv block out")
    dx, dw, db = torch.autograd.grad(y, [x, w, b], cl(g[f"{tag}.gy"]))
    assert_close(ncdhw(dx), g[f"{tag}.dx"], atol=5e-5, what="conv dx")
    assert_close(np64(dw), g[f"{tag}.dw"], atol=2e-4, rtol=1e-4, what="conv dw")
    # bias gradients under InstanceNorm are analytically 0: absolute tolerance only
    assert_close(np64(db), g[f"{tag}.db"], atol=2e-4, rtol=1e-4, what="conv db")


@pytest.mark.parametrize("cin,cout,shape", [(8, 8, (9, 11, 37)), (4, 8, (6, 8, 16)), (1, 4, (5, 9, 20)),
                                            (16, 32, (4, 9, 17)), (32, 64, (5, 6, 7)), (64, 128, (3, 5, 6)),
                                            (128, 128, (2, 3, 10)), (6, 12, (8, 6, 16)), (48, 8, (4, 6, 20)),
                                            (12, 2, (6, 6, 18)), (24, 48, (3, 4, 5)),
                                            # large-volume tile configurations (B*V >= 60 000 / 600 000), ragged in every axis
                                            (8, 8, (21, 40, 41)), (8, 4, (20, 41, 42)), (4, 8, (19, 42, 44)),
                                            (16, 16, (18, 44, 42)), (16, 32, (17, 43, 45)), (12, 12, (21, 41, 39)),
                                            (16, 24, (50, 81, 80))])
def test_conv_vs_oracle(ops, cin, cout, shape):
    """every (Cin,Cout) the model uses, on tile-ragged shapes: fwd, dgrad, wgrad vs ATen-CPU fp64."""
    gen = torch.Generator().manual_seed(cin * 131 + cout)
    x = torch.randn((2, cin) + shape, generator=gen).double().requires_grad_(True)
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double().requires_grad_(True)
    b = (0.1 * torch.randn(cout, generator=gen)).double().requires_grad_(True)
    ref = torch.nn.functional.conv3d(x, w, b, padding=1)
    gy = torch.randn(ref.shape, generator=gen).double()
    rx, rw, rb = torch.autograd.grad(ref, [x, w, b], gy)
    xd = cl(x.detach().numpy()).requires_grad_(True)
    wd, bd = w.detach().float().cuda().requires_grad_(True), b.detach().float().cuda().requires_grad_(True)
    y = ops.conv3d(xd, wd, bd, False)
    assert_close(ncdhw(y), ref.detach().numpy(), what="conv fwd")
    dx, dw, db = torch.autograd.grad(y, [xd, wd, bd], cl(gy.numpy()))
    assert_close(ncdhw(dx), rx.numpy(), atol=5e-5, what="conv dgrad")
    # d_w / d_bias are sums over n = 2*prod(shape) voxels of O(1) products accumulated in fp32: the absolute error
    # grows like sqrt(n) (5e-4 holds up to ~2e4 voxels)
    wtol = 5e-4 * max(1.0, (2 * np.prod(shape) / 2e4) ** 0.5)
    assert_close(np64(dw), rw.numpy(), atol=wtol, rtol=2e-4, what="conv wgrad")
    assert_close(np64(db), rb.numpy(), atol=wtol, rtol=2e-4, what="conv dbias")


@pytest.mark.parametrize("cin,cout,shape", [(4, 8, (21, 40, 41)), (8, 8, (23, 33, 35)), (8, 4, (17, 16, 50)),
                                            (8, 16, (19, 24, 30)), (8, 12, (16, 16, 16)), (4, 4, (9, 30, 31)),
                                            (16, 16, (19, 24, 30)), (16, 8, (17, 18, 20)), (12, 12, (16, 20, 18))])
def test_conv_x3_march_vs_fp64(ops, cin, cout, shape):
    """csrc/conv3d_x3.hip: the z-marching bf16x3 kernels of the few-channel layers (volumes >= 4096 voxels, Cin 4/8, Cout
    4..16) hold the fp32 kernels' tolerances against ATen-CPU fp64 -- forward (bias, fused LeakyReLU), the fused
    InstanceNorm statistics (through the normalised output), the lazily normalised input (NORM) and the data gradient,
    on shapes ragged against the 16x16 columns and the z chunks, batch 2."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(cin * 977 + cout)
    x = torch.randn((2, cin) + shape, generator=gen).double()
    x[:, :, :, : shape[1] // 3] = 0.25                                   # a constant region, like a skull-stripped background
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double()
    b = (0.1 * torch.randn(cout, generator=gen)).double()
    ref = F.conv3d(x, w, b, padding=1)
    xd, wd, bd = cl(x.numpy()), w.float().cuda(), b.float().cuda()
    assert_close(ncdhw(ops.conv3d_forward(xd, wd, bd, False)), ref.numpy(), what="x3 fwd")
    assert_close(ncdhw(ops.conv3d_forward(xd, wd, bd, True)), F.leaky_relu(ref, 0.1).numpy(), what="x3 fwd + LeakyReLU")
    # fused statistics -> InstanceNorm + LeakyReLU of the raw output
    y = ops.conv3d_instnorm_lrelu(xd, wd, bd)
    refn = F.leaky_relu(F.instance_norm(ref, eps=1e-5), 0.1)
    assert_close(ncdhw(y), refn.numpy(), atol=5e-5, rtol=5e-5, what="x3 fwd + fused InstanceNorm statistics")
    # data gradient (the same kernel on flipped / transposed weights)
    gy = torch.randn(ref.shape, generator=gen).double()
    rx = torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)
    assert_close(ncdhw(ops.conv3d_backward_data(cl(gy.numpy()), wd, cin)), rx.numpy(), atol=5e-5, what="x3 dgrad")
    # lazily normalised input: conv(LeakyReLU(InstanceNorm(x_raw))) without materialising the normalised tensor
    with torch.no_grad():
        mean, rstd = ops.instnorm_stats(xd)
        z, zst = ops.conv3d_forward_normin(xd, mean, rstd, wd, bd, True)
    xin = F.leaky_relu(F.instance_norm(x, eps=1e-5), 0.1)
    refz = F.conv3d(xin, w, b, padding=1)
    assert_close(ncdhw(z), refz.numpy(), atol=1e-4, rtol=5e-5, what="x3 fwd, normalised on load")
    zn = ops._InstNormLReLU.apply(z, 1e-5, zst)
    assert_close(ncdhw(zn), F.leaky_relu(F.instance_norm(refz, eps=1e-5), 0.1).numpy(), atol=1e-4, rtol=5e-5,
                 what="x3 normin + statistics")
    # run-to-run deterministic (no atomics)
    assert torch.equal(ops.conv3d_forward(xd, wd, bd, False), ops.conv3d_forward(xd, wd, bd, False))


@pytest.mark.parametrize("cin,cout,shape,B", [(16, 32, (9, 17, 28), 2), (32, 32, (10, 12, 19), 2), (12, 2, (12, 18, 21), 1),
                                              (6, 12, (17, 10, 27), 1), (24, 4, (9, 24, 20), 1), (24, 24, (8, 17, 31), 2),
                                              (48, 8, (13, 15, 22), 1), (24, 48, (16, 16, 17), 1), (64, 64, (8, 9, 30), 2),
                                              (2, 12, (12, 18, 21), 1), (20, 20, (11, 19, 20), 1)])
def test_conv_q_and_transpose_read_wgrad_vs_fp64(ops, cin, cout, shape, B):
    """csrc/conv3d_q.hip (kernel family 5: forward / data gradient with k = (tap, channel quad)) and csrc/conv3d_wtr.hip (family
    4: weight gradient through LDS transpose reads) at the channel counts of pyramid levels 3-4 and the CWM layers, on shapes
    ragged against the 2x8x8 tiles: the dispatch is asserted, the results hold the fp32 kernels' tolerances against ATen-CPU
    fp64 -- forward, fused InstanceNorm statistics, lazily normalised input, data gradient, weight / bias gradient -- and
    are run-to-run identical."""
    import torch.nn.functional as F
    L = ops._L()
    assert L.modet_conv3d_kernel_family_v(B, *shape, cin, cout, 0, 0) == 5, "forward does not take conv_q_kernel"
    assert L.modet_conv3d_kernel_family_v(B, *shape, cin, cout, 1, 0) == 5, "data gradient does not take conv_q_kernel"
    if cin >= 4:                                                         # (2 -> 12 only occurs as the data gradient of 12 -> 2)
        assert L.modet_conv3d_kernel_family_v(B, *shape, cin, cout, 2, 0) == 4, "weight gradient does not take conv_wgrad_tr_kernel"
    gen = torch.Generator().manual_seed(cin * 389 + cout)
    x = torch.randn((B, cin) + shape, generator=gen).double()
    x[:, :, :, : shape[1] // 3] = -0.5                                   # a constant region
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double()
    b = (0.1 * torch.randn(cout, generator=gen)).double()
    ref = F.conv3d(x, w, b, padding=1)
    xd, wd, bd = cl(x.numpy()), w.float().cuda(), b.float().cuda()
    y = ops.conv3d_forward(xd, wd, bd, False)
    assert_close(ncdhw(y), ref.numpy(), what="q fwd")
    assert torch.equal(y, ops.conv3d_forward(xd, wd, bd, False)), "forward not deterministic"
    gy = torch.randn(ref.shape, generator=gen).double()
    gd = cl(gy.numpy())
    rx = torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)
    assert_close(ncdhw(ops.conv3d_backward_data(gd, wd, cin)), rx.numpy(), atol=5e-5, what="q dgrad")
    rw = torch.nn.grad.conv3d_weight(x, w.shape, gy, padding=1)
    dw, db = ops.conv3d_backward_weight(xd, gd, True)
    dw2, db2 = ops.conv3d_backward_weight(xd, gd, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "weight gradient not deterministic"
    assert float((dw.double().cpu() - rw).abs().max() / rw.abs().max()) < 2e-5, "tr wgrad"
    rb = gy.sum((0, 2, 3, 4))
    assert float((db.double().cpu() - rb).abs().max() / rb.abs().max()) < 2e-5, "tr d_bias"
    if cout % 4 == 0:
        z = ops.conv3d_instnorm_lrelu(xd, wd, bd)
        refn = F.leaky_relu(F.instance_norm(ref, eps=1e-5), 0.1)
        assert_close(ncdhw(z), refn.numpy(), atol=5e-5, rtol=5e-5, what="q fwd + fused InstanceNorm statistics")
    if cin % 4 == 0:
        with torch.no_grad():
            mean, rstd = ops.instnorm_stats(xd)
            z, zst = ops.conv3d_forward_normin(xd, mean, rstd, wd, bd, cout % 4 == 0)
        xin = F.leaky_relu(F.instance_norm(x, eps=1e-5), 0.1)
        refz = F.conv3d(xin, w, b, padding=1)
        assert_close(ncdhw(z), refz.numpy(), atol=1e-4, rtol=5e-5, what="q fwd, normalised on load")
        if cout % 4 == 0:
            zn = ops._InstNormLReLU.apply(z, 1e-5, zst)
            assert_close(ncdhw(zn), F.leaky_relu(F.instance_norm(refz, eps=1e-5), 0.1).numpy(), atol=1e-4, rtol=5e-5,
                         what="q normin + statistics")


@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 32)])
@pytest.mark.parametrize("B,shape", [(24, (64, 64, 64)), (110, (38, 38, 38))])
def test_conv_split_tiled_vs_fp64(ops, B, shape, cin, cout):
    """csrc/conv3d_bf16.hip, SP = 3 (kernel family 1: the tiled bf16x3 kernel on fp32 tensors).  The policy sends it the layers
    with >= 16 channels on both sides past 6 000 000 voxels IN TOTAL, where the channel-quad kernel bows out, so the shapes
    reach it through the batch: 24 x 64^3 runs the plan of samples with >= 60 000 voxels (2 x 8 x 16 tiles), 110 x 38^3 the
    small-sample plan (2 x 4 x 16); 32 -> 16 has one output tile per workgroup, 16 -> 32 two, and each one's data gradient is
    the other's shape (16 -> 16 is no case: with <= 16 channels on both sides the z-march takes it).  The batch is ONE random sample
    repeated: sample 0 is held against ATen-CPU fp64 (forward, fused InstanceNorm statistics, data gradient: the fp32 kernels'
    tolerances), every other sample must equal sample 0 bit for bit (all of grid z without a 6 M-voxel reference), and a
    second call must equal the first.  The dispatch is asserted."""
    import torch.nn.functional as F
    L = ops._L()
    assert L.modet_conv3d_kernel_family_v(B, *shape, cin, cout, 0, 0) == 1, "forward does not take the tiled bf16x3 kernel"
    assert L.modet_conv3d_kernel_family_v(B, *shape, cin, cout, 0, 3) == 1, "forward + statistics does not take the tiled bf16x3 kernel"
    assert L.modet_conv3d_kernel_family_v(B, *shape, cin, cout, 1, 0) == 1, "data gradient does not take the tiled bf16x3 kernel"
    gen = torch.Generator().manual_seed(cin * 613 + cout)
    x = torch.randn((1, cin) + shape, generator=gen).double()
    x[:, :, :, : shape[1] // 3] = 0.25                                   # a constant region
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double()
    b = (0.1 * torch.randn(cout, generator=gen)).double()
    gy = torch.randn((1, cout) + shape, generator=gen).double()
    ref = F.conv3d(x, w, b, padding=1)
    refn = F.leaky_relu(F.instance_norm(ref, eps=1e-5), 0.1)
    rx = torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)
    wd, bd = w.float().cuda(), b.float().cuda()
    xd = cl(x.numpy()).repeat(B, 1, 1, 1, 1)                             # materialised: B copies of the one sample
    gd = cl(gy.numpy()).repeat(B, 1, 1, 1, 1)

    def check(run, want, what, **tol):
        y = run()
        assert_close(ncdhw(y[:1]), want.numpy(), what=what, **tol)
        assert torch.equal(y[1:], y[:1].expand_as(y[1:])), f"{what}: a sample differs from sample 0"
        assert torch.equal(y, run()), f"{what}: not deterministic"

    with torch.no_grad():
        check(lambda: ops.conv3d_forward(xd, wd, bd, False), ref, "split fwd")
        check(lambda: ops.conv3d_instnorm_lrelu(xd, wd, bd), refn, "split fwd + fused InstanceNorm statistics", atol=5e-5, rtol=5e-5)
        check(lambda: ops.conv3d_backward_data(gd, wd, cin), rx, "split dgrad", atol=5e-5)


@pytest.mark.parametrize("Cin,Cout,xs,ws", [(8, 8, 1.0, 0.07), (8, 8, 300.0, 0.07), (8, 16, 2e-3, 0.07), (16, 16, 1.0, 3.0),
                                            (16, 16, 1.0, 1e-3), (4, 8, 3000.0, 0.2), (8, 8, 1.0, 0.07)])
def test_conv_forward_two_f16_pieces_range_and_accuracy(Cin, Cout, xs, ws):
    """Round 5: the forward launches of the full-resolution layers run on TWO f16 pieces per operand (three products, operands
    pre-scaled by powers of two) instead of three bf16 pieces (six products).  Against fp64 over the operand ranges the scheme
    must cover -- activations from 2e-3 to 300 (normalised layers; 3000 on the 4-channel layer, whose input is not
    normalised), weights from 1e-3 to 3 -- the error stays below 1e-6 of max|y| (the bf16x3 data gradient of the same
    tensors: the same class), no overflow, no flush to zero."""
    from smilecode_amd import ops
    B, D, H, W = 1, 16, 24, 32
    g = torch.Generator().manual_seed(Cin * 100 + Cout)
    x = (torch.randn(B, D, H, W, Cin, generator=g) * xs).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * ws).cuda()
    b = (torch.randn(Cout, generator=g) * ws).cuda()
    assert ops._L().modet_conv3d_kernel_family(B, D, H, W, Cin, Cout, 0) == 2, "the z-marching family must take this shape"
    y = ops.conv3d_forward(x, w, b, False)
    ref = torch.nn.functional.conv3d(x.double().permute(0, 4, 1, 2, 3).cpu(), w.double().cpu(), b.double().cpu(), padding=1).permute(0, 2, 3, 4, 1)
    assert bool(torch.isfinite(y).all())
    err = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
    _note(f"conv_fwd_f16x2[{Cin}->{Cout},x~{xs:g},w~{ws:g}].maxerr_of_max", err)
    assert err < 1e-6, err


def test_instnorm_backward_leaves_the_gradient_maximum(ops):
    """modet_instnorm_lrelu_bwd*_amax: the three InstanceNorm backward forms also leave max |d_x| (one float, integer atomic
    max on the bit pattern: exact and order-independent) and tag d_x with it; d_x itself is bit-identical to the plain call."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((2, 12, 20, 36, 8), generator=gen).cuda().requires_grad_(True)
    gy = (torch.randn(x.shape, generator=gen) * 3e-5).cuda()
    y = ops.instnorm_lrelu(x)
    dx, = torch.autograd.grad(y, x, gy)
    tag = ops._amax_of(dx)
    assert tag is not None and tag.numel() == ops.AMAX_FLOATS and float(tag[::32].max()) == float(dx.abs().max()) and float(tag[::32].max()) > 0
    from smilecode_amd import _lib
    L = ops._L()
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // (B * C)
    mean, rstd = ops.instnorm_stats(x.detach())
    nb = L.modet_instnorm_ws_bytes(B, V, C)
    ws = torch.empty(nb // 4 + 1, device="cuda")
    ref = torch.empty_like(dx)
    _lib.check(L.modet_instnorm_lrelu_bwd(gy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ref.data_ptr(),
                                          ws.data_ptr(), nb, B, V, C, None), "plain")
    assert torch.equal(ref, dx)
    # the tag dies with an in-place accumulation into the tensor (autograd's gradient accumulation does exactly that)
    dx.add_(1.0)
    assert ops._amax_of(dx) is None
    # pooled form (a level's output block): gradient = unpool(g_pooled) / 8 + [ga; gb]
    pooled, ya, yb = ops.instnorm_lrelu_pool_tee_split(x, None, 1)
    gp = (torch.randn(pooled.shape, generator=gen) * 1e-3).cuda()
    ga = (torch.randn(ya.shape, generator=gen) * 1e-3).cuda()
    dx2, = torch.autograd.grad([pooled, ya], x, [gp, ga])
    tag2 = ops._amax_of(dx2)
    assert tag2 is not None and float(tag2[::32].max()) == float(dx2.abs().max())


@pytest.mark.parametrize("shape", [(1, 2, 1), (1, 2, 2), (2, 2, 2)])
def test_instnorm_statistics_of_a_few_voxels_beside_a_large_mean(ops, shape):
    """InstanceNorm over 2, 4 and 8 voxels -- level 5 of a 16x32x16, 16x32x32, 32x32x32 volume -- of channels whose |mean| is 0.1 - 0.4,
    30 - 120 x sqrt(var + eps) (over so few voxels a channel's variance falls far below its squared mean: 800 x at level 5 of the
    16x32x16 edge case): the normalised tensor at the per-op tolerance, mean and rstd against fp64 of the same fp32 values.
    var = E[x^2] - E[x]^2 from fp32 sums loses eps_f32 * mean^2 / (var + eps) of rstd, up to 9e-4 here and as much of the output; the
    shifted sums of csrc/norm_act.hip (IN_SHIFT_MAX_V) cancel against the sample's range instead.  rstd's bound: (x - K)^2 <=
    16 var, <= 10 roundings on the way -> 160 eps_f32 * var / (var + eps) on var + eps, half of it on rstd, < 1e-6."""
    gen = torch.Generator().manual_seed(sum(shape))
    B, C = 3, 64
    sign = torch.where(torch.rand((B, C, 1, 1, 1), generator=gen) < 0.5, -1.0, 1.0)
    x = (sign * (0.1 + 0.3 * torch.rand((B, C, 1, 1, 1), generator=gen)) + 1e-3 * torch.randn((B, C) + shape, generator=gen)).float()
    x64 = x.double()
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.instance_norm(x64, eps=1e-5), 0.1)
    m64 = x64.mean((2, 3, 4)).reshape(-1)
    r64 = (x64.var((2, 3, 4), unbiased=False) + 1e-5).rsqrt().reshape(-1)
    assert float((m64 * r64).abs().max()) > 100, "mean^2 >> var + eps"
    xd = cl(x.numpy())
    assert_close(ncdhw(ops.instnorm_lrelu(xd)), ref.numpy(), what="InstanceNorm + LeakyReLU over %d voxels" % int(np.prod(shape)))
    mean, rstd = ops.instnorm_stats(xd)
    assert_close(np64(mean), m64.numpy(), atol=1e-7, rtol=1e-7, what="mean")
    e = float((rstd.double().cpu() / r64 - 1).abs().max())
    _note("instnorm_few_voxels[%d].rstd_relerr" % int(np.prod(shape)), e)
    assert e < 1e-6, e


@pytest.mark.parametrize("Cin,Cout,shape,xs,ws", [(32, 32, (40, 48, 40), 1.0, 1.0), (16, 32, (40, 48, 40), 30.0, 0.05), (64, 64, (20, 24, 20), 2e-3, 4.0),
                                                  (24, 48, (20, 24, 28), 1.0, 1.0), (6, 12, (40, 48, 56), 0.5, 1.0), (32, 64, (20, 24, 20), 200.0, 1.0),
                                                  # cfg 5's level-3 CWM layers: 1.72 M voxels (beyond the round-4 routing limit of 1.5 M)
                                                  (6, 12, (80, 96, 112), 1.0, 1.0), (12, 2, (80, 96, 112), 1.0, 1.0)])
def test_conv_q_two_f16_pieces_forward_and_gradient(ops, Cin, Cout, shape, xs, ws):
    """Round 5: the channel-quad kernel of the mid / coarse levels and the CWM layers (family 5) on two f16 pieces: forward
    (activations x 2^4, weights x 2^8) and, given max |d_y|, the data gradient -- against fp64 over activation scales 2e-3..200,
    weight scales 0.05..4, gradients of 1e-7: <= 3e-6 of max and no worse than the bf16x3 launch (the fp32 accumulation of up to
    1 728 terms is what both are limited by), finite; the gradient differs in rounding from the bf16x3 launch
    (i.e. the f16 form ran)."""
    B = 2
    D, H, W = shape
    gen = torch.Generator().manual_seed(Cin * 5 + Cout)
    x = (torch.randn((B, Cin, D, H, W), generator=gen) * xs).double()
    w = (torch.randn((Cout, Cin, 3, 3, 3), generator=gen) * ws / np.sqrt(27 * Cin)).double()
    b = (torch.randn(Cout, generator=gen) * 0.1).double()
    gy = torch.randn((B, Cout, D, H, W), generator=gen).double() * 1e-7
    L = ops._L()
    assert L.modet_conv3d_kernel_family(B, D, H, W, Cin, Cout, 0) == 5 and L.modet_conv3d_kernel_family(B, D, H, W, Cin, Cout, 1) == 5
    ry = torch.nn.functional.conv3d(x, w, b, padding=1)
    rx = torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)
    xd, gd, wd, bd = cl(x.numpy()), cl(gy.numpy()), w.float().cuda(), b.float().cuda()
    t64 = lambda t: torch.from_numpy(ncdhw(t))                                              # noqa: E731
    y = ops.conv3d_forward(xd, wd, bd, False)
    ey = float((t64(y) - ry).abs().max() / ry.abs().max())
    assert bool(torch.isfinite(y).all()) and ey < 3e-6, ey              # (1 728 fp32-accumulated terms at 64 channels)
    dx3 = ops.conv3d_backward_data(gd, wd, Cin)
    dx2 = ops.conv3d_backward_data(gd, wd, Cin, amax=ops.amax_buffer(gd.abs().max()))
    e2 = float((t64(dx2) - rx).abs().max() / rx.abs().max())
    e3 = float((t64(dx3) - rx).abs().max() / rx.abs().max())
    _note(f"convq_f16x2[{Cin}->{Cout},x~{xs:g},w~{ws:g}].fwd_maxerr_of_max", ey)
    _note(f"convq_f16x2[{Cin}->{Cout},x~{xs:g},w~{ws:g}].dgrad_maxerr_of_max", e2)
    _note(f"convq_bf16x3[{Cin}->{Cout},x~{xs:g},w~{ws:g}].dgrad_maxerr_of_max", e3)
    assert bool(torch.isfinite(dx2).all()) and e2 < 3e-6 and e2 <= 1.5 * e3 + 2e-7 and not torch.equal(dx2, dx3), (e2, e3)
    # weight gradient (family 4, transpose-read kernel) with x an activation
    xa = torch.nn.functional.leaky_relu(x / xs, 0.1)
    rw = torch.nn.grad.conv3d_weight(xa, w.shape, gy, padding=1)
    rb = gy.sum((0, 2, 3, 4))
    xad = cl(xa.numpy())
    if L.modet_conv3d_kernel_family(B, D, H, W, Cin, Cout, 2) == 4:
        dw3, db3 = ops.conv3d_backward_weight(xad, gd, True)
        dw2, db2 = ops.conv3d_backward_weight(xad, gd, True, amax=ops.amax_buffer(gd.abs().max()))
        ew2 = float((dw2.double().cpu() - rw).abs().max() / rw.abs().max())
        ew3 = float((dw3.double().cpu() - rw).abs().max() / rw.abs().max())
        eb2 = float((db2.double().cpu() - rb).abs().max() / rb.abs().max())
        _note(f"convwtr_f16x2[{Cin}->{Cout}].wgrad_maxerr_of_max", ew2)
        _note(f"convwtr_bf16x3[{Cin}->{Cout}].wgrad_maxerr_of_max", ew3)
        assert bool(torch.isfinite(dw2).all()) and ew2 < 3e-6 and eb2 < 3e-5 and not torch.equal(dw2, dw3), (ew2, ew3, eb2)
        dw2r, _ = ops.conv3d_backward_weight(xad, gd, True, amax=ops.amax_buffer(gd.abs().max()))
        assert torch.equal(dw2, dw2r)


@pytest.mark.parametrize("Cin,Cout,gs,heavy", [(8, 8, 1.0, False), (8, 8, 3e-9, False), (8, 8, 2e3, True), (4, 8, 1e-6, True),
                                               (8, 4, 1e-7, False), (16, 16, 1e-5, True), (8, 16, 40.0, False)])
def test_conv_backward_two_f16_pieces_with_gradient_maximum(ops, Cin, Cout, gs, heavy):
    """Round 5: with max |d_y| known (left by the InstanceNorm backward that produced d_y) the z-marching data-gradient and
    weight-gradient kernels split their operands into TWO f16 pieces (three MFMA products) instead of three bf16 pieces (six):
    d_y is scaled by the power of two that takes its maximum into [2^14, 2^15) while it is split.  Against fp64 over gradient
    magnitudes from 3e-9 to 2e3, also heavy-tailed ones (a few elements 1e4 times the rest): same error class as the bf16x3
    kernels (<= 1e-6 of max), nothing overflows, nothing is flushed; and an amax that OVERSTATES the maximum 1000-fold only moves
    the absolute floor (documented contract), it does not break the result."""
    B, D, H, W = 2, 52, 44, 45                         # 206 k voxels: the z-marching weight gradient's threshold is 200 k
    gen = torch.Generator().manual_seed(Cin * 17 + Cout)
    x = torch.nn.functional.leaky_relu(torch.randn((B, Cin, D, H, W), generator=gen), 0.1).double()
    w = (torch.randn((Cout, Cin, 3, 3, 3), generator=gen) / np.sqrt(27 * Cin)).double()
    gy = torch.randn((B, Cout, D, H, W), generator=gen).double() * gs
    if heavy:
        m = torch.rand(gy.shape, generator=gen) < 1e-4
        gy = torch.where(m, gy * 1e4, gy)
    rx = torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)
    rw = torch.nn.grad.conv3d_weight(x, w.shape, gy, padding=1)
    rb = gy.sum((0, 2, 3, 4))
    xd, gd, wd = cl(x.numpy()), cl(gy.numpy()), w.float().cuda()
    amax = ops.amax_buffer(gd.abs().max())
    L = ops._L()
    assert L.modet_conv3d_kernel_family(B, D, H, W, Cout, Cin, 0) == 2, "the z-marching family must take this data gradient"
    dx3 = ops.conv3d_backward_data(gd, wd, Cin)
    dx2 = ops.conv3d_backward_data(gd, wd, Cin, amax=amax)
    assert bool(torch.isfinite(dx2).all())
    assert not torch.equal(dx2, dx3), "the f16 form must have run (it rounds differently)"
    t64 = lambda t: torch.from_numpy(ncdhw(t))                                              # noqa: E731
    e2 = float((t64(dx2) - rx).abs().max() / rx.abs().max())
    e3 = float((t64(dx3) - rx).abs().max() / rx.abs().max())
    _note(f"conv_dgrad_f16x2[{Cout}->{Cin},g~{gs:g}{',heavy' if heavy else ''}].maxerr_of_max", e2)
    _note(f"conv_dgrad_bf16x3[{Cout}->{Cin},g~{gs:g}{',heavy' if heavy else ''}].maxerr_of_max", e3)
    assert e2 < 1e-6, (e2, e3)
    dx2b = ops.conv3d_backward_data(gd, wd, Cin, amax=amax * 1000.0)
    e2b = float((t64(dx2b) - rx).abs().max() / rx.abs().max())
    assert e2b < 1e-6, e2b
    if Cin <= 8:
        dw3, db3 = ops.conv3d_backward_weight(xd, gd, True)
        dw2, db2 = ops.conv3d_backward_weight(xd, gd, True, amax=amax)
        ew2 = float((dw2.double().cpu() - rw).abs().max() / rw.abs().max())
        ew3 = float((dw3.double().cpu() - rw).abs().max() / rw.abs().max())
        eb2 = float((db2.double().cpu() - rb).abs().max() / max(float(rb.abs().max()), 1e-30))
        _note(f"conv_wgrad_f16x2[{Cin}->{Cout},g~{gs:g}{',heavy' if heavy else ''}].maxerr_of_max", ew2)
        _note(f"conv_wgrad_bf16x3[{Cin}->{Cout},g~{gs:g}{',heavy' if heavy else ''}].maxerr_of_max", ew3)
        assert bool(torch.isfinite(dw2).all()) and ew2 < 3e-6 and eb2 < 3e-5, (ew2, ew3, eb2)
        if Cout <= 8:                                  # (Cout 16 runs the transpose-read kernel: bf16x3 either way)
            assert not torch.equal(dw2, dw3), "the f16 form must have run"
        dw2r, db2r = ops.conv3d_backward_weight(xd, gd, True, amax=amax)
        assert torch.equal(dw2, dw2r) and torch.equal(db2, db2r), "weight gradient must be run-to-run deterministic"


def test_block_chain_backward_runs_on_f16_pieces_and_matches_fp64(ops, monkeypatch):
    """ConvInsBlock -> ConvInsBlock chain as the encoder runs it (conv + statistics, lazily normalised conv, InstanceNorm):
    with the gradient-maximum tags the whole backward of the chain runs on f16 pieces; it must differ in rounding from the
    untagged (bf16x3) backward -- i.e. the tags really travel through autograd -- and both must sit on the fp64 result."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(11)
    shape, cin, c = (24, 44, 48), 4, 8
    x = F.leaky_relu(torch.randn((2, cin) + shape, generator=gen), 0.1).double().requires_grad_(True)
    w1 = (torch.randn((c, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double().requires_grad_(True)
    w2 = (torch.randn((c, c, 3, 3, 3), generator=gen) / np.sqrt(c * 27)).double().requires_grad_(True)
    b1 = (0.1 * torch.randn(c, generator=gen)).double().requires_grad_(True)
    b2 = (0.1 * torch.randn(c, generator=gen)).double().requires_grad_(True)
    gy = torch.randn((2, c) + shape, generator=gen).double() * 1e-6
    h = F.leaky_relu(F.instance_norm(F.conv3d(x, w1, b1, padding=1), eps=1e-5), 0.1)
    ref = F.leaky_relu(F.instance_norm(F.conv3d(h, w2, b2, padding=1), eps=1e-5), 0.1)
    r = torch.autograd.grad(ref, [x, w1, w2], gy)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "GRAD_F16", on)
        xd = cl(x.detach().numpy()).requires_grad_(True)
        p = [t.detach().float().cuda().requires_grad_(True) for t in (w1, b1, w2, b2)]
        raw, st = ops.conv3d_with_stats(xd, p[0], p[1], x_act=True)
        raw2, st2 = ops.lazy_instnorm_conv3d(raw, st, p[2], p[3])
        y = ops._InstNormLReLU.apply(raw2, 1e-5, st2)
        res[on] = torch.autograd.grad(y, [xd, p[0], p[2]], cl(gy.numpy()))
        for got, want, name in ((torch.from_numpy(ncdhw(res[on][0])), r[0], "dx"), (res[on][1].double().cpu(), r[1], "dw1"), (res[on][2].double().cpu(), r[2], "dw2")):
            e = float((got - want).abs().max() / want.abs().max())
            _note(f"block_chain_bwd[{'f16x2' if on else 'bf16x3'}].{name}_maxerr_of_max", e)
            assert e < 2e-5, (on, name, e)
    assert not torch.equal(res[True][1], res[False][1]) and not torch.equal(res[True][0], res[False][0])


@pytest.mark.parametrize("Cin,Cout,shape", [(8, 8, (16, 24, 32)), (32, 32, (20, 24, 20)), (4, 8, (16, 24, 32))])
def test_conv_forward_any_input_range(ops, Cin, Cout, shape):
    """nn.Conv3d (reference models.py:127) accepts any fp32 activation, so the plain forward entry points must too (VERDICT r5
    item 6): inputs of magnitude 1e5 and 1e9 -- far outside the two-f16-piece forms' range, include/modet_hip.h "TWO f16 PIECES"
    -- give the fp64 result (the plain entry points run the three bf16 pieces, which have fp32's range), with and without the
    fused InstanceNorm statistics.  The f16 form is behind x_act=True, the CALLER'S word that |x| < 4 094: inside the range it
    equals fp64 too; beyond it the result is inf, which is that entry point's documented contract."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((1, Cin) + shape, generator=gen).double()
    w = (torch.randn((Cout, Cin, 3, 3, 3), generator=gen) / np.sqrt(27 * Cin)).double()
    wd = w.float().cuda()
    for mag in (4000.0, 1.0e5, 1.0e9):
        xin = x / x.abs().max() * mag
        ref = torch.nn.functional.conv3d(xin, w, None, padding=1)
        xd = cl(xin.numpy())
        y = ops.conv3d_forward(xd, wd, None, False)
        assert bool(torch.isfinite(y).all())
        err = float((torch.from_numpy(ncdhw(y)) - ref).abs().max() / ref.abs().max())
        _note(f"conv_any_range[{Cin}->{Cout}].relerr_at_{mag:g}", err)
        assert err < 2e-6, (mag, err)
        y2, st = ops.conv3d_with_stats(xd, wd, None)            # (the ConvInsBlock form: x_act defaults to False)
        assert float((torch.from_numpy(ncdhw(y2)) - ref).abs().max() / ref.abs().max()) < 2e-6
    xin = x / x.abs().max() * 4000.0
    ref = torch.nn.functional.conv3d(xin, w, None, padding=1)
    yb = ops.conv3d_forward(cl(xin.numpy()), wd, None, False, x_act=True)
    assert float((torch.from_numpy(ncdhw(yb)) - ref).abs().max() / ref.abs().max()) < 2e-6
    yo = ops.conv3d_forward(cl((x / x.abs().max() * 1.0e5).numpy()), wd, None, False, x_act=True)
    assert not bool(torch.isfinite(yo).all()), "x_act=True beyond the promised range: inf by contract (not a finite wrong answer)"


@pytest.mark.parametrize("cin,cout,shape", [(8, 8, (40, 50, 52)), (4, 8, (37, 46, 63)), (8, 16, (33, 42, 75)), (8, 4, (40, 41, 66))])
def test_conv_x3_weight_gradient_vs_fp64(ops, cin, cout, shape):
    """csrc/conv3d_x3.hip, weight gradient: the z-marching bf16x3 kernel (Cin 4/8, Cout <= 16, >= 200 k voxels) against
    ATen-CPU fp64, tile-ragged in every axis, batch 2; deterministic run to run.  d_w / d_bias sum n = 2*prod(shape)
    products of O(1) in fp32 accumulators: the absolute tolerance grows like sqrt(n), as for the exact-f32 kernels."""
    gen = torch.Generator().manual_seed(cin * 31 + cout)
    x = torch.randn((2, cin) + shape, generator=gen).double()
    gy = torch.randn((2, cout) + shape, generator=gen).double()
    rw = torch.nn.grad.conv3d_weight(x, (cout, cin, 3, 3, 3), gy, padding=1)
    rb = gy.sum((0, 2, 3, 4))
    xd, gd = cl(x.numpy()), cl(gy.numpy())
    dw, db = ops.conv3d_backward_weight(xd, gd, True)
    wtol = 5e-4 * max(1.0, (2 * np.prod(shape) / 2e4) ** 0.5)
    assert_close(np64(dw), rw.numpy(), atol=wtol, rtol=2e-4, what="x3 wgrad")
    assert_close(np64(db), rb.numpy(), atol=wtol, rtol=2e-4, what="x3 dbias")
    dw2, db2 = ops.conv3d_backward_weight(xd, gd, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "weight gradient must be run-to-run deterministic"
    dw3, _ = ops.conv3d_backward_weight(xd, gd, False)
    assert torch.equal(dw, dw3)


def test_prepacked_conv_weights_follow_the_weights(ops):
    """ops.StepContext.prepacked(): pass 1 records the packing jobs (forward + data-gradient form of every layer), later
    passes pack them all in one launch from the CURRENT weights and the conv launches use that copy -- outputs and data
    gradients must be bit-identical to the unscoped calls, also after the weights were updated in place, for the plain,
    row-packed (Cout <= 8), statistics and multi-chunk configurations."""
    from smilecode_amd import _lib
    gen = torch.Generator().manual_seed(9)
    cfgs = [(4, 8, (9, 24, 37)), (8, 8, (21, 40, 41)), (8, 4, (6, 9, 20)), (16, 16, (5, 9, 20)), (16, 32, (4, 6, 18)),
            (32, 32, (4, 6, 9)), (12, 2, (6, 6, 18)), (64, 128, (2, 3, 10))]
    layers = []
    for cin, cout, shape in cfgs:
        x = torch.randn((2,) + shape + (cin,), generator=gen).cuda().requires_grad_(True)
        w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).cuda().requires_grad_(True)
        b = (0.1 * torch.randn(cout, generator=gen)).cuda().requires_grad_(True)
        gy = torch.randn((2,) + shape + (cout,), generator=gen).cuda()
        layers.append((x, w, b, gy))

    def run():
        out = []
        for i, (x, w, b, gy) in enumerate(layers):
            y = ops.conv3d_instnorm_lrelu(x, w, b) if i % 2 else ops.conv3d(x, w, b, False)
            (dx,) = torch.autograd.grad(y, [x], gy)
            out.append((y.detach().clone(), dx.clone()))
        return out

    pp = ops.StepContext()
    with pp.prepacked():
        first = run()                                        # recording pass (packs per launch)
    assert pp.arena is not None and _lib.load().modet_conv3d_prepack_arena_bytes(pp.handle) > 0
    for a, b in zip(first, run()):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with torch.no_grad():
        for _, w, _, _ in layers:
            w.mul_(1.5).add_(0.01)                           # an optimizer step: same storage, new values
    want = run()                                             # unscoped: packs per launch from the new weights
    with pp.prepacked():
        got = run()                                          # one packing launch, then no per-launch packing
    for a, b in zip(want, got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(first[0][0], got[0][0])
    other = ops.StepContext()                                # a second context (another trainer) records its own table
    with other.prepacked():                                  # and leaves the first one's alone: no re-recording
        run()
    arena_before = pp.arena.data_ptr()
    with pp.prepacked():
        with other.prepacked():                              # interleaved scopes of two contexts on one thread
            inner = run()
        again = run()
    assert pp.arena.data_ptr() == arena_before and pp.recorded and other.recorded
    for a, b, c in zip(want, again, inner):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert ops.current_step() is None


def test_deferred_wgrad_reductions_bit_identical(ops):
    """ops.StepContext.deferred(): all weight-gradient reductions of a backward pass as one launch, written to the
    destinations the scope was given.  40 layers (two batches of the 32-job table) covering the three partial-tile
    layouts -- conv3d_wgrad_kernel (Cin 4/8/16 M packing), conv3d_wgrad_np_kernel (Cin, Cout <= 8) and the first 1->4
    layer with LeakyReLU' folded in -- must give exactly the bits of the per-layer reductions, with and without a bias."""
    cfgs = [(1, 4, (9, 17, 33)), (4, 8, (9, 24, 37)), (8, 8, (21, 40, 41)), (8, 4, (6, 9, 20)), (16, 16, (5, 9, 20)),
            (16, 32, (4, 6, 18)), (12, 2, (6, 6, 18)), (24, 48, (3, 4, 5)), (6, 12, (8, 6, 16)), (64, 128, (2, 3, 10))] * 4
    gen = torch.Generator().manual_seed(5)
    ins, dst = [], {}
    for i, (cin, cout, shape) in enumerate(cfgs):
        x = torch.randn((2,) + shape + (cin,), generator=gen).cuda()
        dy = torch.randn((2,) + shape + (cout,), generator=gen).cuda()
        ya = torch.randn((2,) + shape + (cout,), generator=gen).cuda() if cin == 1 else None
        w, b = torch.zeros((cout, cin, 3, 3, 3), device="cuda"), torch.zeros((cout,), device="cuda")   # the "parameters"
        dst[w.data_ptr()] = torch.full_like(w, float("nan"))
        dst[b.data_ptr()] = torch.full_like(b, float("nan"))
        ins.append((x, dy, i % 3 != 0, ya, w, b))
    ref = [ops.conv3d_backward_weight(x, dy, wb, y_act=ya) for x, dy, wb, ya, _, _ in ins]
    sc = ops.StepContext()
    with sc.deferred(dst) as scope:
        got = [ops.conv3d_backward_weight(x, dy, wb, y_act=ya, w=w, b=b) for x, dy, wb, ya, w, b in ins]
        junk = [torch.full((1 << 20,), float("nan"), device="cuda") for _ in range(8)]    # allocator churn inside the scope
        del junk
        # a second use of a weight inside the scope takes the immediate path and returns its gradient
        x, dy, wb, ya, w, b = ins[2]
        w2, b2 = ops.conv3d_backward_weight(x, dy, True, w=w, b=b)
        # so does a parameter the scope has no destination for
        w3, _ = ops.conv3d_backward_weight(x, dy, False, w=torch.zeros_like(w), b=None)
    assert all(g == (None, None) for g in got)
    for (rw, rb), (x, dy, wb, ya, w, b) in zip(ref, ins):
        assert torch.equal(rw, dst[w.data_ptr()]) and w.data_ptr() in scope.written
        if wb:
            assert torch.equal(rb, dst[b.data_ptr()]) and b.data_ptr() in scope.written
        else:
            assert bool(torch.isnan(dst[b.data_ptr()]).all()) and b.data_ptr() not in scope.written
    assert torch.equal(w2, ref[2][0]) and torch.equal(w3, ref[2][0])
    with pytest.raises(RuntimeError, match="do not nest"):
        with sc.deferred(dst):
            with sc.deferred(dst):
                pass
    assert sc.dst is None and ops.current_step() is None         # the outer scope unwound cleanly
    rw, rb = ops.conv3d_backward_weight(*ins[1][:3])             # no scope: immediate
    assert torch.equal(rw, ref[1][0])


@pytest.mark.parametrize("cin,cout,shape", [(4, 8, (9, 24, 37)), (8, 8, (33, 40, 48)), (8, 16, (6, 8, 16)),
                                            (16, 16, (5, 9, 20)), (12, 4, (7, 6, 18)), (32, 32, (4, 6, 9))])
def test_conv_instnorm_fused_vs_oracle(ops, cin, cout, shape):
    """ConvInsBlock through ops.conv3d_instnorm_lrelu: InstanceNorm statistics from the conv epilogue (Cout 4/8/16, both
    the 8-wave large-volume and the 4-wave small-volume tile configs, tile-ragged shapes) and the unfused fallback."""
    gen = torch.Generator().manual_seed(cin * 17 + cout)
    x = torch.randn((2, cin) + shape, generator=gen).double().requires_grad_(True)
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double().requires_grad_(True)
    b = (0.1 * torch.randn(cout, generator=gen)).double().requires_grad_(True)
    xhat = torch.nn.functional.instance_norm(torch.nn.functional.conv3d(x, w, b, padding=1), eps=1e-5)
    ref = torch.nn.functional.leaky_relu(xhat, 0.1)
    # LeakyReLU is not differentiable at 0: an element whose normalised value is within fp32 noise of 0 may take the
    # other slope on the GPU.  Give those (about one in a million) no upstream gradient so the comparison is well posed.
    gy = torch.randn(ref.shape, generator=gen).double() * (xhat.detach().abs() > 1e-4)
    rx, rw = torch.autograd.grad(ref, [x, w], gy)
    xd = cl(x.detach().numpy()).requires_grad_(True)
    wd, bd = w.detach().float().cuda().requires_grad_(True), b.detach().float().cuda().requires_grad_(True)
    y = ops.conv3d_instnorm_lrelu(xd, wd, bd)
    assert_close(ncdhw(y), ref.detach().numpy(), atol=5e-5, what="fused conv+IN+LReLU")
    y2 = ops.instnorm_lrelu(ops.conv3d(xd, wd, bd, False))
    assert_close(np64(y), np64(y2), atol=2e-5, what="fused vs two-pass statistics")
    dx, dw = torch.autograd.grad(y, [xd, wd], cl(gy.numpy()))
    assert_close(ncdhw(dx), rx.numpy(), atol=1e-4, what="fused block dx")
    assert_close(np64(dw), rw.numpy(), atol=5e-4, rtol=2e-4, what="fused block dw")


@pytest.mark.parametrize("c0,c1,c2,shape,B", [(4, 8, 8, (20, 24, 28), 2), (8, 16, 16, (17, 21, 40), 1), (8, 8, 4, (33, 40, 48), 1),
                                              (6, 12, 12, (18, 20, 35), 1), (16, 32, 32, (12, 10, 20), 2),
                                              (32, 64, 64, (20, 24, 20), 2), (12, 24, 8, (20, 24, 28), 1),
                                              (8, 8, 8, (64, 96, 112), 1)])
def test_instnorm_conv_chain_with_fused_backward_statistics(ops, c0, c1, c2, shape, B):
    """conv -> InstanceNorm + LeakyReLU -> conv as the model runs it in training (ops.lazy_instnorm_conv3d = one autograd
    node): the second conv's data gradient forms the norm's backward statistics in its epilogue
    (modet_conv3d_bwd_data_instats: the z-march family and, since round 5, the channel-quad family of the mid / coarse levels
    and the CWM layers; the remaining shapes take the two-kernel form) -- against fp64 autograd, and against the unfused form
    of the same build."""
    L = ops._L()
    if L.modet_conv3d_kernel_family(B, *shape, c1, c2, 1) in (2, 5) and c1 % 4 == 0:
        assert L.modet_conv3d_bwd_data_instats_bytes(B, *shape, c1, c2) > 0, "this shape must take the fused form"
    gen = torch.Generator().manual_seed(c0 * 101 + c1 * 7 + c2)
    x = torch.randn((B, c0) + shape, generator=gen).double().requires_grad_(True)
    w1 = (torch.randn((c1, c0, 3, 3, 3), generator=gen) / np.sqrt(c0 * 27)).double().requires_grad_(True)
    w2 = (torch.randn((c2, c1, 3, 3, 3), generator=gen) / np.sqrt(c1 * 27)).double().requires_grad_(True)
    b2 = (0.1 * torch.randn(c2, generator=gen)).double().requires_grad_(True)
    big = int(np.prod(shape)) > 200000
    xd = cl(x.detach().numpy()).requires_grad_(True)
    w1d, w2d, b2d = (t.detach().float().cuda().requires_grad_(True) for t in (w1, w2, b2))
    gz = torch.randn((B,) + shape + (c2,), generator=gen).cuda()

    def run(flag):
        ops.FUSE_IN_DGRAD = flag
        try:
            raw, st = ops.conv3d_with_stats(xd, w1d, None)
            z, _ = ops.lazy_instnorm_conv3d(raw, st, w2d, b2d)
            return [z.detach()] + list(torch.autograd.grad(z, [xd, w1d, w2d, b2d], gz))
        finally:
            ops.FUSE_IN_DGRAD = True

    got, plain = run(True), run(False)
    for name, a, b in zip(("z", "dx", "dw1", "dw2", "db2"), got, plain):
        d = float((a - b).abs().max())
        assert d <= 2e-5 * float(b.abs().max()) + 1e-7, f"{name}: fused vs unfused backward statistics, max |d| {d}"
    if not big:                                            # (fp64 conv autograd on the host: small shapes only)
        raw_r = torch.nn.functional.conv3d(x, w1, None, padding=1)
        xhat = torch.nn.functional.instance_norm(raw_r, eps=1e-5)
        z_r = torch.nn.functional.conv3d(torch.nn.functional.leaky_relu(xhat, 0.1), w2, b2, padding=1)
        gzr = gz.double().cpu().permute(0, 4, 1, 2, 3)
        ref = [z_r.detach()] + list(torch.autograd.grad(z_r, [x, w1, w2, b2], gzr))
        assert_close(ncdhw(got[0]), ref[0].numpy(), atol=1e-4, what="chain z")
        # LeakyReLU's kink: a handful of elements within fp32 noise of 0 may take the other slope on the GPU (each moves
        # d_x by a few 1e-3 of its max locally); compare in the mean and bound the outliers
        ex = np.abs(ncdhw(got[1]) - ref[1].numpy())
        assert float(ex.mean()) <= 2e-6 * float(ref[1].abs().max()) + 1e-7 and float(ex.max()) <= 5e-2 * float(ref[1].abs().max())
        assert_close(np64(got[2]), ref[2].numpy(), atol=5e-4 * float(ref[2].abs().max()), what="chain dw1")
        assert_close(np64(got[3]), ref[3].numpy(), atol=5e-4 * float(ref[3].abs().max()), what="chain dw2")
    again = run(True)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "the fused form must be run-to-run deterministic"


@pytest.mark.parametrize("c0,c1,c2,f16", [(4, 8, 8, True), (8, 8, 8, True), (8, 8, 8, False), (4, 4, 8, True)])
def test_training_chain_without_the_normalised_tensor(ops, monkeypatch, c0, c1, c2, f16):
    """Round 5: where the z-marching weight-gradient kernel takes the second conv of a ConvInsBlock ->
    ConvInsBlock chain, the TRAINING step never writes LeakyReLU(InstanceNorm(raw)): the forward conv and the weight gradient
    normalise while they stage (modet_conv3d_fwd_normin / modet_conv3d_bwd_weight_normin).  Against the materialised form of
    the same build (same arithmetic: output and data gradient bit-identical, weight gradient equal to rounding of the sums)
    and against fp64, with and without the f16 gradient form."""
    import torch.nn.functional as F
    monkeypatch.setattr(ops, "GRAD_F16", f16)
    B, shape = 2, (52, 44, 45)
    L = ops._L()
    assert L.modet_conv3d_bwd_weight_normin_ok(B, *shape, c1, c2) == 1
    gen = torch.Generator().manual_seed(c0 * 11 + c1 + c2)
    x = F.leaky_relu(torch.randn((B, c0) + shape, generator=gen), 0.1).double()
    w1 = (torch.randn((c1, c0, 3, 3, 3), generator=gen) / np.sqrt(c0 * 27)).double().requires_grad_(True)
    w2 = (torch.randn((c2, c1, 3, 3, 3), generator=gen) / np.sqrt(c1 * 27)).double().requires_grad_(True)
    b2 = (0.1 * torch.randn(c2, generator=gen)).double().requires_grad_(True)
    gy = torch.randn((B, c2) + shape, generator=gen).double() * 1e-4
    h = F.leaky_relu(F.instance_norm(F.conv3d(x, w1, None, padding=1), eps=1e-5), 0.1)
    ref = F.leaky_relu(F.instance_norm(F.conv3d(h, w2, b2, padding=1), eps=1e-5), 0.1)
    r = torch.autograd.grad(ref, [w1, w2, b2], gy)
    res = {}
    for lazy in (True, False):
        monkeypatch.setattr(ops, "LAZY_IN_TRAIN", lazy)
        xd = cl(x.numpy()).requires_grad_(True)
        p = [t.detach().float().cuda().requires_grad_(True) for t in (w1, w2, b2)]
        raw, st = ops.conv3d_with_stats(xd, p[0], None, x_act=True)
        raw2, st2 = ops.lazy_instnorm_conv3d(raw, st, p[1], p[2])
        y = ops._InstNormLReLU.apply(raw2, 1e-5, st2)
        g = torch.autograd.grad(y, [xd, p[0], p[1], p[2]], cl(gy.numpy()))
        res[lazy] = (y.detach(), raw2.detach()) + tuple(g)
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][0], res[False][0]), "forward must be bit-identical"
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3]), "d_x / d_w1 must be bit-identical"
    for i, (name, want) in enumerate((("dw1", r[0]), ("dw2", r[1]), ("db2", r[2]))):
        for lazy in (True, False):
            got = res[lazy][3 + i].double().cpu()
            e = float((got - want).abs().max() / want.abs().max())
            if name != "db2":                                  # (db2 sits under an InstanceNorm: analytically zero)
                _note(f"lazy_train_chain[{c0}-{c1}-{c2},{'f16' if f16 else 'bf16x3'},{'lazy' if lazy else 'materialised'}].{name}_maxerr_of_max", e)
                assert e < 2e-5, (name, lazy, e)
    d = float((res[True][4] - res[False][4]).abs().max() / res[False][4].abs().max())
    assert d < 2e-6, d


@pytest.mark.parametrize("cin,cout,shape", [(8, 8, (33, 40, 48)), (16, 16, (9, 11, 37)), (32, 32, (12, 10, 20)),
                                            (12, 2, (7, 9, 18)), (48, 48, (5, 6, 7))])
def test_lazy_instnorm_conv_inference(ops, cin, cout, shape):
    """without gradients ConvIns -> Conv runs with the normalisation inside the conv kernel (modet_conv3d_fwd_normin +
    modet_instnorm_stats): same result as InstanceNorm -> conv, statistics from the epilogue or from a statistics pass"""
    gen = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn((2, cin) + shape, generator=gen).double() * 1.5 + 0.3
    w0 = (torch.randn((cin, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double()
    w = (torch.randn((cout, cin, 3, 3, 3), generator=gen) / np.sqrt(cin * 27)).double()
    b = (0.1 * torch.randn(cout, generator=gen)).double()
    raw_ref = torch.nn.functional.conv3d(x, w0, None, padding=1)
    act = torch.nn.functional.leaky_relu(torch.nn.functional.instance_norm(raw_ref, eps=1e-5), 0.1)
    ref = torch.nn.functional.conv3d(act, w, b, padding=1)
    with torch.no_grad():
        raw, st = ops.conv3d_with_stats(cl(x.numpy()), w0.float().cuda(), None)
        y, _ = ops.lazy_instnorm_conv3d(raw, st, w.float().cuda(), b.float().cuda())
        y2 = ops.conv3d(ops.instnorm_lrelu(raw), w.float().cuda(), b.float().cuda(), False)
    assert_close(ncdhw(y), ref.numpy(), atol=1e-4, what="lazy IN -> conv")
    assert_close(np64(y), np64(y2), atol=2e-5, what="lazy vs materialised")


def test_instnorm_large_and_pool(ops):
    g = gold("op_misc.npz")
    x = cl(g["pool.x"]).requires_grad_(True)   # C=5 is not a multiple of 4 -> must be refused, not mis-computed
    with pytest.raises(RuntimeError):
        ops.avgpool2(x)
    gen = torch.Generator().manual_seed(5)
    xx = (torch.randn((2, 8, 10, 12, 38), generator=gen) * 2 + 0.7).double().requires_grad_(True)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.instance_norm(xx, eps=1e-5), 0.1)
    refp = torch.nn.functional.avg_pool3d(ref, 2)
    gy = torch.randn(refp.shape, generator=gen).double()
    rx = torch.autograd.grad(refp, xx, gy)[0]
    xd = cl(xx.detach().numpy()).requires_grad_(True)
    y = ops.avgpool2(ops.instnorm_lrelu(xd))
    assert_close(ncdhw(y), refp.detach().numpy(), what="IN+LReLU+pool")
    dx = torch.autograd.grad(y, xd, cl(gy.numpy()))[0]
    assert_close(ncdhw(dx), rx.numpy(), atol=5e-5, what="IN+LReLU+pool dx")


def test_upsample_golden(ops):
    g = gold("op_misc.npz")
    x = cl(g["up.x"]).requires_grad_(True)
    y = ops.upsample2(x, 2.0)
    assert_close(ncdhw(y), g["up.out"], what="upsample")
    dx = torch.autograd.grad(y, x, cl(g["up.gy"]))[0]
    assert_close(ncdhw(dx), g["up.dx"], atol=5e-5, what="upsample dx")
    for C in (6, 24, 1):                     # channel-group variants
        gen = torch.Generator().manual_seed(C)
        xx = torch.randn((1, C, 2, 5, 3), generator=gen).double().requires_grad_(True)
        ref = torch.nn.functional.interpolate(xx, scale_factor=2, mode="trilinear", align_corners=True)
        gy = torch.randn(ref.shape, generator=gen).double()
        rx = torch.autograd.grad(ref, xx, gy)[0]
        xd = cl(xx.detach().numpy()).requires_grad_(True)
        yd = ops.upsample2(xd, 1.0)
        assert_close(ncdhw(yd), ref.detach().numpy(), what=f"upsample C={C}")
        assert_close(ncdhw(torch.autograd.grad(yd, xd, cl(gy.numpy()))[0]), rx.numpy(), atol=5e-5, what="upsample dx")


@pytest.mark.parametrize("C,shape,B", [(3, (33, 40, 52), 1), (6, (16, 41, 50), 2), (1, (41, 40, 41), 1)])
def test_upsample_backward_separable(ops, C, shape, B):
    """large levels take the three-pass (z, y, x) form of the upsample gradient: against ATen-CPU fp64 and against the
    one-launch gather it replaces (same weights, different summation order: 1e-5)."""
    from smilecode_amd import _lib
    from smilecode_amd.ops import _p, _stream
    d, h, w = shape
    L = _lib.load()
    assert L.modet_upsample2_bwd_sep_ws_bytes(B, d, h, w, C) > 0 and L.modet_upsample2_bwd_sep_ws_bytes(1, 8, 8, 8, C) == 0
    gen = torch.Generator().manual_seed(C + d)
    xx = torch.randn((B, C) + shape, generator=gen).double().requires_grad_(True)
    ref = torch.nn.functional.interpolate(xx, scale_factor=2, mode="trilinear", align_corners=True) * 2.0
    gy = torch.randn(ref.shape, generator=gen).double()
    rx = torch.autograd.grad(ref, xx, gy)[0]
    xd = cl(xx.detach().numpy()).requires_grad_(True)
    yd = ops.upsample2(xd, 2.0)
    gyd = cl(gy.numpy())
    dx = torch.autograd.grad(yd, xd, gyd)[0]
    assert_close(ncdhw(dx), rx.numpy(), atol=5e-5, what="upsample dx (separable)")
    direct = torch.empty_like(dx)
    _lib.check(L.modet_upsample2_bwd(_p(gyd), _p(direct), B, d, h, w, C, 2.0, _stream()), "modet_upsample2_bwd")
    assert float((direct - dx).abs().max()) <= 1e-5 * max(1.0, float(direct.abs().max()))


@pytest.mark.parametrize("tag,heads", [("w3", 2), ("w5", 8)])
def test_cwm_golden(tag, heads):
    from smilecode_amd.models import CWM
    g = gold("op_misc.npz")
    mod = CWM(3 * heads, 6 * heads).cuda()
    names = [n for n, _ in mod.named_parameters()]
    with torch.no_grad():
        for n, p in mod.named_parameters():
            p.copy_(cu(g[f"{tag}.p.{n}"]))
    x = cl(g[f"{tag}.x"]).requires_grad_(True)
    y = mod(x)
    assert_close(ncdhw(y), g[f"{tag}.out"], what="cwm out")
    grads = torch.autograd.grad(y, [x] + list(mod.parameters()), cl(g[f"{tag}.gy"]))
    assert_close(ncdhw(grads[0]), g[f"{tag}.dx"], atol=5e-5, what="cwm dx")
    for n, gq in zip(names, grads[1:]):
        assert_close(np64(gq), g[f"{tag}.g.{n}"], atol=2e-4, rtol=2e-4, what=f"cwm d{n}")


@pytest.mark.parametrize("heads,shape,B", [(4, (10, 12, 10), 1), (8, (10, 12, 10), 1), (4, (20, 24, 20), 1), (8, (20, 24, 20), 1),
                                           (4, (40, 48, 40), 1), (4, (10, 12, 14), 2), (8, (10, 12, 14), 2),
                                           (4, (20, 24, 28), 2), (8, (20, 24, 28), 2)])
def test_cwm_at_full_size_levels_vs_oracle(ops, orc, heads, shape, B):
    """the CWM module (upsample, ConvIns 3h -> 6h, ConvIns 6h -> 6h, conv 6h -> h, softmax-weighted sum of the h fields) with 4
    and 8 heads at the level-5 / 4 / 3 inputs of 160x192x160 and, with B = 2, of 160x192x224 -- what head layouts other than
    the default run (the default model has 8 heads at level 5 only): forward and every gradient against the fp64 oracle.
    The conv kernel family of each launch is asserted (csrc/conv3d_q.hip forward / data gradient, csrc/conv3d_wtr.hip weight
    gradient).  (8 heads at the level-3 input of 160x192x160 run the same families; its fp64 oracle takes ~15 s of host time.)"""
    from smilecode_amd.models import CWM
    L = ops._L()
    c = 3 * heads
    up = tuple(2 * s for s in shape)
    for cin, cout, variant in ((c, 2 * c, 3), (2 * c, 2 * c, 2), (2 * c, heads, 2)):
        fams = tuple(L.modet_conv3d_kernel_family_v(B, *up, cin, cout, p, variant) for p in (0, 1, 2))
        assert fams == (5, 5, 4), f"CWM conv {cin} -> {cout} at {up}, B={B}: families (fwd, dgrad, wgrad) {fams}"
    gen = torch.Generator().manual_seed(heads * 1000 + shape[2] + B)
    mod = CWM(c, 2 * c)
    p = {}
    with torch.no_grad():
        for n, q in mod.named_parameters():
            fan = q.shape[1] * 27 if q.dim() == 5 else mod.conv[2].weight.shape[1] * 27
            q.copy_((torch.rand(q.shape, generator=gen) * 2 - 1) / np.sqrt(fan))
            p["m." + n] = q.detach().double().clone().requires_grad_(True)
    mod = mod.cuda()
    # the CWM's input is an attention output: expected offsets, |x| <= 1 (the module's first conv relies on it, models.CWM)
    x = (torch.rand((B, c) + shape, generator=gen) * 2 - 1).double().requires_grad_(True)
    ref = orc.cwm(p, "m", x, heads)
    gy = torch.randn(ref.shape, generator=gen).double()
    rg = torch.autograd.grad(ref, [x] + list(p.values()), gy)
    xd = cl(x.detach().numpy()).requires_grad_(True)
    y = mod(xd)
    gd = torch.autograd.grad(y, [xd] + list(mod.parameters()), cl(gy.numpy()))
    tag = f"cwm_h{heads}_{'x'.join(map(str, shape))}_B{B}"

    def rel(a, b):
        return float(np.abs(a - b).max() / np.abs(b).max())

    e = rel(ncdhw(y), ref.detach().numpy())
    _note(f"{tag}.out_relerr", e)
    assert e <= 1e-5, e
    # LeakyReLU's kink: a normalised element within fp32 noise of 0 (these inputs have them at 2e-8 .. 7e-7) may take the other
    # slope on the GPU and move d_x by a few 1e-3 of its max locally, and through the InstanceNorm backward's means by ~1e-5 of
    # it everywhere in its channel (as in test_instnorm_conv_chain_with_fused_backward_statistics): compare in the mean and bound
    # the outliers.  Without a flip the error is ~5e-7 of the max.
    ex, dmax = np.abs(ncdhw(gd[0]) - rg[0].numpy()), float(rg[0].abs().max())
    _note(f"{tag}.dx_relerr", float(ex.max()) / dmax)
    _note(f"{tag}.dx_mean_relerr", float(ex.mean()) / dmax)
    assert float(ex.mean()) <= 1e-4 * dmax and float(ex.max()) <= 5e-2 * dmax, (float(ex.mean()) / dmax, float(ex.max()) / dmax)
    worst = 0.0
    for (n, _), a, b in zip(mod.named_parameters(), gd[1:], rg[1:]):
        if n.endswith("main.bias"):
            continue                      # (a conv bias in front of an InstanceNorm: analytically zero)
        worst = max(worst, rel(np64(a), b.numpy()))
    _note(f"{tag}.param_grad_relerr", worst)
    # (a kink flip also moves the weight gradients of the layers upstream of it: by 7e-3 of the max at 10x12x10, one flip among
    # 9 600 voxels; without one they agree to ~1e-6)
    assert worst <= 2e-2, worst


# ------------------------------------------------------------------------------------------------ losses
def test_ncc_golden(ops):
    g = gold("op_misc.npz")
    a, b = cu(g["ncc.a"]), cu(g["ncc.b"]).requires_grad_(True)
    l = ops.ncc_loss(a, b)
    assert_close(np64(l), g["ncc.val"], atol=2e-5, what="ncc value")
    db = torch.autograd.grad(l * 1.7, b)[0]
    assert_close(np64(db), 1.7 * g["ncc.db"], atol=2e-6, rtol=2e-3, what="ncc d y_pred")


def test_grad3d_golden(ops):
    g = gold("op_misc.npz")
    f = cu(g["g3d.flow"]).requires_grad_(True)
    l = ops.grad3d_loss(f)
    assert_close(np64(l), g["g3d.val"], what="grad3d value")
    df = torch.autograd.grad(l, f)[0]
    assert_close(np64(df), g["g3d.dflow"], atol=1e-7, rtol=1e-4, what="grad3d dflow")


def test_ncc_first_argument_gradient_golden(ops):
    """the reference's train loop differentiates the FIRST argument: loss_function(output[n], y) = NCC_vxm.forward(
    y_true=y_moved, y_pred=fixed) (train.py:127); golden from the reference's own NCC_vxm in that order"""
    from smilecode_amd import losses
    g = gold("op_eval.npz")
    a, b = cu(g["ncc1.a"]).requires_grad_(True), cu(g["ncc1.b"])
    l = losses.NCC_vxm()(a, b)
    assert_close(np64(l), g["ncc1.val"], atol=2e-5, what="ncc value")
    l.backward()
    assert_close(np64(a.grad), g["ncc1.da"], atol=2e-6, rtol=2e-3, what="ncc d y_true")
    # both arguments at once: each gradient equals its one-sided counterpart
    g2 = gold("op_misc.npz")
    a2, b2 = cu(g2["ncc.a"]).requires_grad_(True), cu(g2["ncc.b"]).requires_grad_(True)
    da, db = torch.autograd.grad(ops.ncc_loss(a2, b2), [a2, b2])
    assert_close(np64(da), g2["ncc.da"], atol=2e-6, rtol=2e-3, what="ncc d y_true (both)")
    assert_close(np64(db), g2["ncc.db"], atol=2e-6, rtol=2e-3, what="ncc d y_pred (both)")


@pytest.mark.parametrize("w", [3, 5, 7])
def test_ncc_other_windows_golden(ops, w):
    """NCC_vxm(win=[w, w, w]) (losses.py:52-57), goldens from the reference's own class on a volume ragged against the
    kernel's tiles; windows the HIP path does not implement are refused loudly, not approximated"""
    from smilecode_amd import losses
    g = gold("op_eval.npz")
    a, b = cu(g[f"nccw{w}.a"]).requires_grad_(True), cu(g[f"nccw{w}.b"]).requires_grad_(True)
    l = losses.NCC_vxm(win=[w, w, w])(a, b)
    assert_close(np64(l), g[f"nccw{w}.val"], atol=2e-5, what="ncc value")
    da, db = torch.autograd.grad(l, [a, b])
    assert_close(np64(da), g[f"nccw{w}.da"], atol=2e-6, rtol=2e-3, what="ncc d y_true")
    assert_close(np64(db), g[f"nccw{w}.db"], atol=2e-6, rtol=2e-3, what="ncc d y_pred")
    for bad in ([9, 9], [9, 0, 9], [3, 3, 3, 3]):                          # not a 3-D window
        with pytest.raises(RuntimeError):
            losses.NCC_vxm(win=bad)


@pytest.mark.parametrize("w", [[4, 4, 4], [5, 3, 7], [11, 11, 11], [2, 6, 3], [6, 9, 9], [9, 9, 5], [1, 1, 1]])
def test_ncc_any_window_golden(ops, w):
    """NCC_vxm(win=[wz, wy, wx]) for even / anisotropic / > 9-voxel windows (losses.py:52-59 accepts any list and pads EVERY axis
    by floor(win[0] / 2), so cc lives on a grid that differs from the volume's): goldens from the reference's own class, batch 2,
    value and both gradients; the general separable path (modet_ncc_fwd_bwd_box)."""
    from smilecode_amd import losses
    g = gold("op_ncc_windows.npz")
    tag = "x".join(map(str, w))
    a, b = cu(g[f"ncc[{tag}].a"]).requires_grad_(True), cu(g[f"ncc[{tag}].b"]).requires_grad_(True)
    l = losses.NCC_vxm(win=w)(a, b)
    assert_close(np64(l), g[f"ncc[{tag}].val"], atol=2e-5, what="ncc value")
    da, db = torch.autograd.grad(l, [a, b])
    assert_close(np64(da), g[f"ncc[{tag}].da"], atol=2e-6, rtol=2e-3, what="ncc d y_true")
    assert_close(np64(db), g[f"ncc[{tag}].db"], atol=2e-6, rtol=2e-3, what="ncc d y_pred")
    # only the first argument differentiated (train.py:127's order) takes the swapped-roles launch
    a1 = cu(g[f"ncc[{tag}].a"]).requires_grad_(True)
    (da1,) = torch.autograd.grad(losses.NCC_vxm(win=w)(a1, cu(g[f"ncc[{tag}].b"])), [a1])
    assert_close(np64(da1), g[f"ncc[{tag}].da"], atol=2e-6, rtol=2e-3, what="ncc d y_true alone")
    with pytest.raises(RuntimeError):                                    # a window that leaves no output voxel
        losses.NCC_vxm(win=[2, 40, 3])(a, b)


@pytest.mark.parametrize("shape,B", [((37, 50, 70), 2), ((9, 24, 32), 1), ((4, 5, 6), 1), ((70, 49, 33), 1)])
def test_ncc_z_march_vs_oracle(ops, orc, shape, B):
    """the z-marching NCC kernels on shapes that exercise several z chunks per column, ragged tiles in y and x, and
    volumes smaller than the 9-voxel window, against the fp64 oracle (value, both gradients).  The parity bound of these
    kernels (4 x ATen fp32's own measured error, per quantity) lives in tests/test_gpu_ncc_grad3d.py; the tolerances here are
    the coarse ones this test has always had."""
    gen = torch.Generator().manual_seed(shape[0] * 7 + B)
    base = torch.rand((B, 1) + shape, generator=gen).double()
    a = (base + 0.3 * torch.rand((B, 1) + shape, generator=gen).double()).requires_grad_(True)
    b = (base + 0.3 * torch.rand((B, 1) + shape, generator=gen).double()).requires_grad_(True)
    lr = orc.ncc_loss(a, b)
    ra, rb = torch.autograd.grad(lr, [a, b])
    ad, bd = a.detach().float().cuda().requires_grad_(True), b.detach().float().cuda().requires_grad_(True)
    l = ops.ncc_loss(ad, bd)
    da, db = torch.autograd.grad(l, [ad, bd])
    assert_close(np64(l), float(lr), atol=2e-5, what="ncc value")
    assert_close(np64(da), ra.numpy(), atol=2e-6 / B, rtol=2e-3, what="ncc d y_true")
    assert_close(np64(db), rb.numpy(), atol=2e-6 / B, rtol=2e-3, what="ncc d y_pred")
    l2 = ops.ncc_loss(ad, bd)
    assert torch.equal(l, l2), "deterministic two-stage loss reduction"


def test_grad3d_l1_golden(ops):
    """Grad3d's class default penalty (losses.py:11), golden from the reference's own Grad3d('l1')"""
    from smilecode_amd import losses
    g = gold("op_eval.npz")
    f = cu(g["g3d_l1.flow"]).requires_grad_(True)
    l = losses.Grad3d()(f, None)                 # default-constructed, as the reference allows
    assert_close(np64(l), g["g3d_l1.val"], what="grad3d l1 value")
    df = torch.autograd.grad(l, f)[0]
    assert_close(np64(df), g["g3d_l1.dflow"], atol=1e-7, rtol=1e-4, what="grad3d l1 dflow")
    with pytest.raises(RuntimeError):
        losses.Grad3d(penalty="l3")


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_loss_value_and_gradient_calls_of_the_train_step(ops, scale):
    """the step's own loss calls (engine.Trainer._seeded_loss: value + weighted gradient, no autograd node, Grad3d on the
    CHANNELS-LAST flow) against the reference's goldens -- NCC_vxm (losses.py:34-94) and Grad3d 'l2' / 'l1' (losses.py:6-31) --
    and bit for bit against the autograd nodes' gradients when the weight is 1 (same arithmetic, another layout)"""
    g, ge = gold("op_misc.npz"), gold("op_eval.npz")
    a, b = cu(g["ncc.a"]), cu(g["ncc.b"])
    l, db = ops.ncc_value_and_grad(a, b, 9, scale)
    assert_close(np64(l), g["ncc.val"], atol=2e-5, what="ncc value (unscaled)")
    assert_close(np64(db), scale * g["ncc.db"], atol=2e-6, rtol=2e-3, what="ncc weighted d y_pred")
    for w in (3, 5, 7):
        aw, bw = cu(ge[f"nccw{w}.a"]), cu(ge[f"nccw{w}.b"])
        lw, dbw = ops.ncc_value_and_grad(aw, bw, w, scale)
        assert_close(np64(lw), ge[f"nccw{w}.val"], atol=2e-5, what="ncc value")
        assert_close(np64(dbw), scale * ge[f"nccw{w}.db"], atol=2e-6, rtol=2e-3, what="ncc weighted d y_pred")
    for key, pen, src in (("g3d", "l2", g), ("g3d_l1", "l1", ge)):
        f = cu(src[f"{key}.flow"])                                   # (B,3,D,H,W) planar, as the reference has it
        f_cl = f.permute(0, 2, 3, 4, 1).contiguous()
        lv, df_cl = ops.grad3d_value_and_grad_cl(f_cl, pen, scale)
        assert_close(np64(lv), src[f"{key}.val"], what="grad3d value (unscaled)")
        assert_close(np64(df_cl.permute(0, 4, 1, 2, 3)), scale * src[f"{key}.dflow"], atol=1e-7, rtol=1e-4, what="grad3d weighted dflow")
        if scale == 1.0:
            fp = f.clone().requires_grad_(True)
            (df,) = torch.autograd.grad(ops.grad3d_loss(fp, pen), fp)
            assert torch.equal(df_cl.permute(0, 4, 1, 2, 3), df), "channels-last Grad3d gradient == planar one, bit for bit"
    if scale == 1.0:
        bp = b.clone().requires_grad_(True)
        (db_node,) = torch.autograd.grad(ops.ncc_loss(a, bp), bp)
        assert torch.equal(db, db_node)
    with pytest.raises(RuntimeError):
        ops.grad3d_value_and_grad_cl(cu(g["g3d.flow"]), "l2")        # a planar flow is refused, not misread


def test_leaf_reduce_many_vs_fp64_sums():
    """modet_leaf_reduce_many: any number of column-sum jobs in one call (more than one table's worth here), both addressing
    forms -- the attention's [B][heads][rows][27] partials and the projection's [rows][cols] -- against torch fp64 sums"""
    import ctypes
    from smilecode_amd import _lib
    L = _lib.load()
    gen = torch.Generator().manual_seed(5)
    jobs, want, keep = [], [], []
    for j in range(19):
        if j % 2 == 0:                                   # d_rpb form
            B, heads, rows = 1 + j % 3, 1 + j % 4, 7 + 61 * j
            part = torch.randn((B, heads, rows, 27), generator=gen).cuda()
            dst = [torch.full((heads, 3, 3, 3), float("nan"), device="cuda")]
            job = _lib.LeafJob()
            job.part, job.outer, job.outer_stride, job.rows, job.row_stride = part.data_ptr(), B, heads * rows * 27, rows, 27
            job.col_group_stride, job.ncols, job.col_group = rows * 27, heads * 27, 27
            ref = [part.double().sum((0, 2)).reshape(heads, 3, 3, 3)]
        else:                                            # projection form, four segments
            dim, cin, rows = 6 * (1 + j % 3), 8 * (1 + j % 2), 5 + 97 * j
            ncols = 3 * dim + dim * cin
            part = torch.randn((rows, ncols), generator=gen).cuda()
            dst = [torch.full((dim,), float("nan"), device="cuda") for _ in range(3)] + [torch.full((dim, cin), float("nan"), device="cuda")]
            job = _lib.LeafJob()
            job.part, job.outer, job.outer_stride, job.rows, job.row_stride = part.data_ptr(), 1, 0, rows, ncols
            job.col_group_stride, job.ncols, job.col_group = 0, ncols, ncols
            cs = part.double().sum(0)
            ref = [cs[:dim], cs[dim:2 * dim], cs[2 * dim:3 * dim], cs[3 * dim:].reshape(dim, cin)]
        for u in range(4):
            job.dst[u] = dst[u].data_ptr() if u < len(dst) else None
            job.n[u] = dst[u].numel() if u < len(dst) else 0
        jobs.append(job); want.append((dst, ref)); keep.append(part)
    arr = (_lib.LeafJob * len(jobs))(*jobs)
    _lib.check(L.modet_leaf_reduce_many(ctypes.addressof(arr), len(jobs), torch.cuda.current_stream().cuda_stream), "leaf_reduce")
    torch.cuda.synchronize()
    for dst, ref in want:
        for d, r in zip(dst, ref):
            assert torch.equal(d.cpu(), r.float().cpu().reshape(d.shape)) or float((d.double().cpu() - r.cpu().reshape(d.shape)).abs().max()) < 1e-5
    assert L.modet_leaf_reduce_many(None, 0, None) == 0                       # nothing queued: no launch, no error
    jobs[0].n[0] += 1                                                         # segments that do not add up are refused
    bad = (_lib.LeafJob * 1)(jobs[0])
    assert L.modet_leaf_reduce_many(ctypes.addressof(bad), 1, None) != 0


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_jacobian_determinant_golden(ops, tag):
    """det(J) <= 0 count of infer.py:89-90 on the GPU: integer-exact against the reference's jacobian_determinant_vxm
    (float64 np.gradient arithmetic reproduced operation for operation), incl. a field that folds and a 2x3x2 volume
    where every difference is one-sided"""
    from smilecode_amd import utils
    g = gold("op_eval.npz")
    flow = torch.from_numpy(g[f"jac.{tag}.flow"]).cuda()             # (3,D,H,W) float32
    fcl = flow.permute(1, 2, 3, 0).contiguous()[None]
    counts, det = ops.jacdet_nonpos_count(fcl, want_det=True)
    assert np.array_equal(det[0].cpu().numpy(), g[f"jac.{tag}.det"]), "determinant must be bit-identical to the reference's"
    assert int(counts[0]) == int(g[f"jac.{tag}.nonpos"][0])
    assert np.array_equal(utils.jacobian_determinant_vxm(g[f"jac.{tag}.flow"]), g[f"jac.{tag}.det"])
    frac = utils.jacobian_nonpositive_fraction(flow[None])
    assert frac[0] == int(g[f"jac.{tag}.nonpos"][0]) / float(np.prod(g[f"jac.{tag}.shape"]))
    # batch of two: per-sample counts
    c2, _ = ops.jacdet_nonpos_count(torch.cat([fcl, torch.zeros_like(fcl)], 0).contiguous())
    assert c2.tolist() == [int(g[f"jac.{tag}.nonpos"][0]), 0]


def test_jacobian_count_full_size_vs_oracle(ops, orc):
    """160x192x160: the GPU count equals the oracle's numpy restatement of the reference function, voxel for voxel"""
    from smilecode_amd import synth
    shape = (160, 192, 160)
    flow = synth.make_flow(shape, seed=11, amp=5.0)[0]
    det = orc.jacobian_determinant(flow)
    fcl = torch.from_numpy(flow).cuda().permute(1, 2, 3, 0).contiguous()[None]
    counts, d = ops.jacdet_nonpos_count(fcl, want_det=True)
    assert int(counts[0]) == int(np.sum(det <= 0)) and int(counts[0]) > 0
    assert np.array_equal(d[0].cpu().numpy(), det)


def test_adam_amsgrad(ops, orc):
    gen = torch.Generator().manual_seed(9)
    n = 100003
    p = torch.randn(n, generator=gen)
    st = {"w": (torch.zeros(n).double(), torch.zeros(n).double(), torch.zeros(n).double())}
    pr = {"w": p.double().clone()}
    pd, m, v, vm = p.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    for step in range(1, 4):
        gr = torch.randn(n, generator=gen) * (0.1 if step == 2 else 1.0)   # step 2: vmax keeps the old max
        orc.adam_amsgrad_step(pr, {"w": gr.double()}, st, 1e-3, step)
        ops.adam_amsgrad_step_(pd, gr.cuda(), m, v, vm, 1e-3, step)
    assert_close(np64(pd), pr["w"].numpy(), atol=1e-6, rtol=1e-6, what="adam params after 3 steps")


def test_label_warp_dice_golden(ops):
    from smilecode_amd import synth
    from smilecode_amd.utils import dice_from_counts, dice_val_VOI
    g = gold("op_dice.npz")
    shape = tuple(int(s) for s in g["shape"])
    lm = torch.from_numpy(synth.make_labels(shape, 24)).cuda()
    lf = torch.from_numpy(synth.make_labels(shape, 25)).cuda()
    flow = cl(g["flow"])
    warped, counts = ops.label_warp_counts(lm, flow, lf, 54)
    assert np.array_equal(warped.cpu().numpy(), g["warped"]), "nearest-warped labels must be bit-exact"
    assert abs(dice_from_counts(counts) - float(g["dice"])) < 1e-9
    assert abs(float(dice_val_VOI(lm[None, None], lf[None, None])) - float(g["dice_raw"])) < 1e-9


def _Z(*shape, dtype=torch.float32, device="cuda"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _handle(like, data16):
    """an fp32 feature handle carrying bf16 data (ops._InstNormLReLUBF16PoolSplit, features16)"""
    h = torch.zeros(1, device="cuda").expand(like.shape)
    h.data16 = data16
    return h


def _refusals():
    """(the op's name as its message carries it, the call with mismatched arguments).  Every row is a tensor whose shape, dtype
    or device a kernel would infer from ANOTHER argument: the host must refuse it before it takes a pointer."""
    from smilecode_amd import functional as fn, losses, ops, utils
    bf = torch.bfloat16
    x8, w88, b8 = _Z(1, 4, 6, 8, 8), _Z(8, 8, 3, 3, 3), _Z(8)
    lab = _Z(4, 6, 8, dtype=torch.int16)
    q6 = _Z(1, 1, 4, 5, 6, 6)
    k6 = _Z(1, 1, 6, 7, 8, 6)
    pw = (_Z(6, 8), _Z(6), _Z(6), _Z(6))
    g = lambda t: t.requires_grad_(True)
    return [
        # ---- the checks this table was written for
        ("label_warp_counts", lambda: ops.label_warp_counts(lab, _Z(1, 4, 6, 8, 3), _Z(4, 6, 7, dtype=torch.int16))),      # lab_fixed of another shape
        ("label_warp_counts", lambda: ops.label_warp_counts(lab, _Z(1, 4, 6, 9, 3), lab)),                                 # flow of another shape
        ("label_warp_counts", lambda: ops.label_warp_counts(lab, _Z(2, 4, 6, 8, 3), lab)),                                 # a batch of flows
        ("label_warp_counts", lambda: ops.label_warp_counts(lab.cpu(), _Z(1, 4, 6, 8, 3), lab)),                           # labels on the host
        ("label_warp_counts", lambda: ops.label_warp_counts(lab, _Z(1, 4, 6, 8, 3), lab.cpu())),
        ("label_warp_counts", lambda: ops.label_warp_counts(_Z(2, 4, 6, 8, dtype=torch.int16), _Z(1, 4, 6, 8, 3), lab)),   # two label volumes
        ("label_warp_counts", lambda: ops.label_warp_counts(lab, _Z(1, 4, 6, 8, 3), lab, nlabels=0)),
        ("label_warp_counts", lambda: utils.dice_val_VOI(_Z(1, 1, 4, 6, 8), _Z(1, 1, 4, 6, 9))),
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(1, 4, 4, 4, 12), _Z(1, 4, 4, 4, 12), _Z(1, 27), 2, 1.0)),   # short rpb
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(1, 4, 4, 4, 13), _Z(1, 4, 4, 4, 13), _Z(2, 27), 2, 1.0)),   # C % heads
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(1, 4, 4, 4, 7), _Z(1, 4, 4, 4, 7), _Z(1, 27), 1, 1.0)),     # head_dim 7
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(4, 4, 4, 6), _Z(4, 4, 4, 6), _Z(1, 27), 1, 1.0)),           # no batch axis
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(1, 4, 4, 4, 6), _Z(1, 4, 4, 5, 6), _Z(1, 27), 1, 1.0)),
        ("cwm_tail", lambda: ops.cwm_tail(_Z(1, 100, 6), _Z(1, 100, 4))),                                                  # x is not (..., heads * 3)
        ("cwm_tail", lambda: ops.cwm_tail(_Z(1, 99, 12), _Z(1, 100, 4))),
        ("modet_fw", lambda: fn.modet_fw(_Z(1, 2, 4, 5, 6, 6), _Z(1, 2, 6, 7, 8, 6), _Z(1, 3, 3, 3))),                    # rpb of fewer heads
        ("modet_fw", lambda: fn.modet_fw(_Z(2, 4, 5, 6, 6), _Z(2, 6, 7, 8, 6))),
        ("modet_bw", lambda: fn.modet_bw(_Z(1, 1, 4, 5, 6, 26), q6, k6, True)),                                            # d_attn of another shape
        ("modet_bw", lambda: fn.modet_bw(_Z(1, 1, 4, 5, 6, 27), q6, _Z(1, 1, 6, 7, 7, 6), True)),                          # key that is not query's partner
        ("Input resolution", lambda: fn.modet_bw(_Z(1, 1, 2, 5, 6, 27), _Z(1, 1, 2, 5, 6, 6), _Z(1, 1, 4, 7, 8, 6), False)),   # smaller than the kernel
        # ---- what the audit of ops.py found besides
        ("conv3d", lambda: ops.conv3d(x8, w88, _Z(4))),                                                                   # bias of another size
        ("conv3d_forward_normin", lambda: ops.conv3d_forward_normin(x8, _Z(4), _Z(8), w88, b8)),                           # mean of another size
        ("conv3d_forward_normin", lambda: ops.conv3d_forward_normin(x8, _Z(8), _Z(8), _Z(8, 4, 3, 3, 3), b8)),
        ("conv3d_backward_data", lambda: ops.conv3d_backward_data(x8, _Z(8, 4, 3, 3, 3), 8)),
        ("conv3d_backward_weight", lambda: ops.conv3d_backward_weight(x8, _Z(1, 4, 6, 9, 8), True)),
        ("conv3d_backward_weight", lambda: ops.conv3d_backward_weight(x8, x8, True, y_act=_Z(1, 4, 6, 8, 4))),
        ("conv3d_backward_weight", lambda: ops.conv3d_backward_weight(x8, x8, True, amax=_Z(64 * 32), norm=(_Z(8), _Z(4)))),
        ("conv3d", lambda: ops.conv3d_with_stats(x8, _Z(8, 4, 3, 3, 3), b8)),
        ("conv3d_with_stats", lambda: ops._Conv3dStats.apply(x8, _Z(8, 4, 3, 3, 3), b8, False)),
        ("lazy_instnorm_conv3d", lambda: ops.lazy_instnorm_conv3d(x8, None, _Z(8, 4, 3, 3, 3), b8)),                       # inference form
        ("lazy_instnorm_conv3d", lambda: ops.lazy_instnorm_conv3d(g(_Z(1, 4, 6, 8, 8)), None, w88, _Z(4))),                # training form
        ("pool_tee_split", lambda: ops.pool_tee_split(_Z(2, 4, 6, 8, 8), 2)),
        ("instnorm_lrelu_pool_tee_split", lambda: ops.instnorm_lrelu_pool_tee_split(_Z(2, 4, 6, 8, 8), None, 0)),
        ("proj_ln", lambda: ops.proj_ln(_Z(1, 50, 8), _Z(6, 4), *pw[1:])),
        ("proj_ln", lambda: ops.proj_ln(_Z(1, 50, 8), pw[0], pw[1], _Z(5), pw[3])),
        ("proj_ln", lambda: ops.proj_ln_pair(g(_Z(1, 50, 8)), g(_Z(1, 50, 8)), pw[0], pw[1], pw[2], _Z(12))),
        ("level attention (bf16)", lambda: ops.level_attention_bf16(x8, _Z(1, 4, 6, 9, 8), None, *pw, _Z(1, 27), 1, 1.0)),
        ("level attention (bf16)", lambda: ops.level_attention_bf16(x8, x8, _Z(1, 4, 6, 8, 2), *pw, _Z(1, 27), 1, 1.0)),
        ("level attention (bf16)", lambda: ops.level_attention_bf16(x8, x8, None, *pw, _Z(1, 26), 1, 1.0)),
        ("level attention (bf16)", lambda: ops.level_attention_bf16(x8, x8, None, _Z(8, 8), _Z(8), _Z(8), _Z(8), _Z(1, 27), 1, 1.0)),   # head_dim 8 in bf16
        ("adam_amsgrad_step_", lambda: ops.adam_amsgrad_step_(_Z(100), _Z(99), _Z(100), _Z(100), _Z(100), 1e-3, 1)),
        ("conv3d_bf16", lambda: ops.conv3d_bf16_forward(x8, w88, _Z(4))),
        ("conv3d_bf16_backward_data", lambda: ops.conv3d_bf16_backward_data(_Z(1, 4, 6, 8, 8, dtype=bf), _Z(8, 4, 3, 3, 3), 8, True)),
        ("conv3d_bf16_backward_weight", lambda: ops.conv3d_bf16_backward_weight(x8, _Z(1, 4, 6, 9, 8, dtype=bf))),
        ("conv3d_bf16_backward_weight", lambda: ops.conv3d_bf16_backward_weight(x8, x8)),                                  # fp32 gradient
        ("instnorm bf16", lambda: ops._InstNormLReLUBF16.apply(_Z(1, 4, 6, 8, 8, dtype=bf), None, 1e-5, True)),
        # ---- one row per remaining added check (a check without a row could be deleted unseen)
        ("label_warp_counts", lambda: ops.label_warp_counts(_Z(6, 8, dtype=torch.int16), _Z(1, 4, 6, 8, 3), lab)),         # fewer than three axes
        ("conv3d_forward_normin", lambda: ops.conv3d_forward_normin(x8, _Z(8), _Z(4), w88, b8)),                           # rstd of another size
        ("conv3d_forward_normin", lambda: ops.conv3d_forward_normin(_Z(4, 6, 8, 8), _Z(8), _Z(8), w88, b8)),               # 4-D input
        ("conv3d_backward_data", lambda: ops.conv3d_backward_data(_Z(4, 6, 8, 8), w88, 8)),                                # 4-D gradient
        ("conv3d_backward_data", lambda: ops.conv3d_backward_data(x8, w88, 8, amax=_Z(1))),                                # one float of amax
        ("conv3d_backward_weight", lambda: ops.conv3d_backward_weight(x8, x8, True, amax=_Z(64))),
        ("conv3d_backward_weight", lambda: ops.conv3d_backward_weight(x8, x8, True, amax=_Z(64 * 32), norm=(_Z(4), _Z(8)))),   # mean
        ("conv3d_backward_weight", lambda: ops.conv3d_backward_weight(_Z(4, 6, 8, 8), _Z(4, 6, 8, 8), True)),
        ("conv3d", lambda: ops.conv3d(_Z(4, 6, 8, 8), w88, b8)),                                                          # 4-D input
        ("conv3d_with_stats", lambda: ops._Conv3dStats.apply(x8, w88, _Z(4), False)),
        ("lazy_instnorm_conv3d", lambda: ops._InstNormConv.apply(g(_Z(1, 4, 6, 8, 8)), None, _Z(8, 4, 3, 3, 3), b8, 1e-5, True)),
        ("avgpool2", lambda: ops.avgpool2(_Z(4, 6, 8, 8))),
        ("pool_tee", lambda: ops.pool_tee(_Z(4, 6, 8, 8))),
        ("pool_tee_split", lambda: ops.pool_tee_split(_Z(4, 6, 8, 8), 1)),
        ("pool_tee_split", lambda: ops.pool_tee_split(_Z(2, 4, 6, 8, 8), 0)),
        ("instnorm_lrelu_pool_tee_split", lambda: ops.instnorm_lrelu_pool_tee_split(_Z(4, 6, 8, 8), None, 1)),
        ("instnorm_lrelu_pool_tee_split", lambda: ops.instnorm_lrelu_pool_tee_split(_Z(2, 4, 6, 8, 8), None, 2)),
        ("smilecode_amd", lambda: ops.instnorm_lrelu_pool_tee_split(_Z(2, 4, 6, 8, 8), _Z(64).cpu(), 1)),                   # statistics on the host
        ("smilecode_amd", lambda: ops.lazy_instnorm_conv3d(g(_Z(1, 4, 6, 8, 8)), _Z(64).cpu(), w88, b8)),
        ("smilecode_amd", lambda: ops.conv3d_forward_normin(x8, _Z(8).cpu(), _Z(8), w88, b8)),
        ("smilecode_amd", lambda: ops.conv3d_backward_data(x8, w88, 8, amax=_Z(64 * 32).cpu())),
        ("smilecode_amd", lambda: ops.conv3d_backward_weight(x8, x8, True, y_act=x8.cpu())),
        ("smilecode_amd", lambda: ops.conv3d_backward_weight(x8, x8, True, amax=_Z(64 * 32), norm=(_Z(8).cpu(), _Z(8)))),
        ("proj_ln", lambda: ops.proj_ln(_Z(1, 50, 8), _Z(6, 8, 1), *pw[1:])),                                              # a 3-D weight
        ("proj_ln", lambda: ops.proj_ln(_Z(1, 50, 8), pw[0], _Z(5), pw[2], pw[3])),                                        # bias
        ("proj_ln", lambda: ops.proj_ln(_Z(1, 50, 8), pw[0], pw[1], pw[2], _Z(5))),                                        # beta
        ("proj_ln_pair", lambda: ops._ProjLNPair.apply(_Z(1, 50, 8), _Z(1, 49, 8), *pw, 1e-5)),
        ("proj_ln_pair", lambda: ops._ProjLNPair.apply(_Z(1, 50, 8), _Z(1, 50, 8), _Z(6, 4), *pw[1:], 1e-5)),
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(1, 4, 4, 4, 6), _Z(1, 4, 4, 4, 6), _Z(1, 27), 0, 1.0)),     # no heads
        ("neighbourhood attention", lambda: ops.neighbourhood_attention(_Z(1, 4, 4, 4, 136), _Z(1, 4, 4, 4, 136), _Z(1, 27), 1, 1.0)),  # head_dim > 128
        ("level attention (bf16)", lambda: ops.level_attention_bf16(_Z(4, 6, 8, 8), _Z(4, 6, 8, 8), None, *pw, _Z(1, 27), 1, 1.0)),   # 4-D features
        ("level attention (bf16)", lambda: ops.level_attention_bf16(x8, x8, None, _Z(6, 4), *pw[1:], _Z(1, 27), 1, 1.0)),
        ("level attention (bf16)", lambda: ops.level_attention_bf16(_handle(x8, _Z(1, 4, 6, 7, 8, dtype=bf)), x8, None, *pw, _Z(1, 27), 1, 1.0)),
        ("level attention (bf16)", lambda: ops.level_attention_bf16(x8, _handle(x8, _Z(1, 4, 6, 8, 4, dtype=bf)), None, *pw, _Z(1, 27), 1, 1.0)),
        ("correlation3d", lambda: ops.correlation3d(_Z(4, 6, 8, 8), _Z(4, 6, 8, 8))),
        ("warp", lambda: ops.warp(_Z(4, 6, 8, 8), _Z(4, 6, 8, 3))),
        ("warp", lambda: ops.warp_tee(_Z(4, 6, 8, 8), _Z(4, 6, 8, 3))),
        ("upsample2", lambda: ops.upsample2(_Z(4, 6, 8, 8))),
        ("jacdet_nonpos_count", lambda: ops.jacdet_nonpos_count(_Z(4, 6, 8, 3))),
        ("adam_amsgrad_step_", lambda: ops.adam_amsgrad_step_(_Z(100), _Z(100), _Z(99), _Z(100), _Z(100), 1e-3, 1)),
        ("adam_amsgrad_step_", lambda: ops.adam_amsgrad_step_(_Z(100), _Z(100), _Z(100), _Z(99), _Z(100), 1e-3, 1)),
        ("adam_amsgrad_step_", lambda: ops.adam_amsgrad_step_(_Z(100), _Z(100), _Z(100), _Z(100), _Z(99), 1e-3, 1)),
        ("conv3d_bf16", lambda: ops.conv3d_bf16_forward(_Z(4, 6, 8, 8), w88, b8)),
        ("conv3d_bf16_backward_data", lambda: ops.conv3d_bf16_backward_data(_Z(4, 6, 8, 8, dtype=bf), w88, 8, True)),
        ("conv3d_bf16_backward_weight", lambda: ops.conv3d_bf16_backward_weight(_Z(4, 6, 8, 8), _Z(4, 6, 8, 8, dtype=bf))),
        ("instnorm bf16", lambda: ops._InstNormLReLUBF16PoolSplit.apply(_Z(2, 4, 6, 8, 8, dtype=bf), None, 1e-5, 1)),        # no statistics
        ("instnorm bf16", lambda: ops._InstNormLReLUBF16PoolSplit.apply(_Z(2, 4, 6, 8, 8, dtype=bf), _Z(64), 1e-5, 2)),      # split outside
        ("instnorm bf16", lambda: ops._InstNormLReLUBF16PoolSplit.apply(_Z(4, 6, 8, 8, dtype=bf), _Z(64), 1e-5, 1)),         # 4-D
        ("smilecode_amd", lambda: ops._InstNormLReLUBF16PoolSplit.apply(_Z(2, 4, 6, 8, 8, dtype=bf), _Z(64).cpu(), 1e-5, 1)),
        ("smilecode_amd", lambda: ops._InstNormLReLUBF16.apply(_Z(1, 4, 6, 8, 8, dtype=bf), _Z(64).cpu(), 1e-5, True)),
        ("modet_bw", lambda: fn.modet_bw(_Z(1, 4, 5, 6, 27), _Z(1, 4, 5, 6, 6), _Z(1, 6, 7, 8, 6), True)),                 # 5-D query
        ("kernel size", lambda: fn.modet_fw(q6, k6, _Z(27))),                                                             # a flat rpb
        # (the device comparisons of functional.modet_fw / modet_bw -- key, rpb, d_attn against query -- need two GPUs: a host
        #  tensor is refused by _check_input first; label_warp_counts' device rows above are the one-GPU form of that check)
        # ---- checks that were there already
        ("smilecode_amd", lambda: ops.instnorm_lrelu(torch.zeros(1, 4, 4, 4, 8))),                                         # CPU tensor: no fallback
        ("smilecode_amd", lambda: ops.avgpool2(_Z(1, 4, 4, 4, 8, dtype=torch.float64))),
        ("smilecode_amd", lambda: ops.upsample2(_Z(1, 4, 4, 4, 8).transpose(1, 2))),
        ("conv3d", lambda: ops.conv3d(x8, _Z(8, 4, 3, 3, 3), b8)),
        ("warp", lambda: ops.warp(x8, _Z(1, 4, 6, 8, 2))),
        ("warp", lambda: ops.warp_tee(x8, _Z(2, 4, 6, 8, 3))),
        ("correlation3d", lambda: ops.correlation3d(x8, _Z(1, 4, 6, 9, 8))),
        ("NCC", lambda: ops.ncc_loss(_Z(1, 1, 4, 6, 8), _Z(1, 1, 4, 6, 9))),
        ("NCC", lambda: losses.NCC_vxm()(_Z(1, 1, 4, 6, 8), _Z(1, 2, 4, 6, 8))),
        ("NCC", lambda: ops.ncc_value_and_grad(_Z(1, 1, 4, 6, 8), _Z(2, 1, 4, 6, 8))),
        ("Grad3d", lambda: ops.grad3d_loss(_Z(1, 2, 4, 6, 8))),
        ("Grad3d", lambda: ops.grad3d_value_and_grad_cl(_Z(1, 3, 4, 6, 8))),
        ("jacdet_nonpos_count", lambda: ops.jacdet_nonpos_count(_Z(1, 4, 6, 8, 2))),
        ("label_warp_counts", lambda: ops.label_warp_counts(lab.int(), _Z(1, 4, 6, 8, 3), lab)),
        ("key must be", lambda: fn.modet_fw(q6, _Z(1, 1, 6, 7, 7, 6))),
        ("kernel size", lambda: fn.modet_fw(q6, k6, _Z(1, 5, 5, 5))),
    ]


def test_errors_are_loud(ops, monkeypatch):
    """Mismatched arguments are refused on the host, by name, BEFORE a pointer reaches the library: the library object is
    replaced by a proxy in refuse mode (tests/guard.py), so a row whose host check is missing fails with the proxy's
    AssertionError instead of launching a kernel on bad arguments."""
    from smilecode_amd import _lib
    from tests import guard
    px = guard.LibProxy(_lib.load(), refuse=True)
    monkeypatch.setattr(_lib, "_lib", px)
    x = torch.zeros(1, 4, 4, 4, 8)
    with pytest.raises(RuntimeError):
        ops.instnorm_lrelu(x)                                # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        ops.neighbourhood_attention(torch.zeros(1, 4, 4, 4, 7, device="cuda"), torch.zeros(1, 4, 4, 4, 7, device="cuda"),
                                    torch.zeros(1, 27, device="cuda"), 1, 1.0)   # head_dim 7 unsupported
    for name, call in _refusals():
        with pytest.raises(RuntimeError, match=re.escape(name)):
            call()
    with pytest.raises(AssertionError, match="refuse mode"):          # the proxy itself: a good call does not get through either
        ops.avgpool2(_Z(1, 4, 4, 4, 8))
