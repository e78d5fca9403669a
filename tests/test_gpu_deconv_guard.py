"""-m gpu: WHERE the stride-2 4x4x4 transposed-convolution kernels read and write -- tests/test_gpu_convs2_guard.py's assertions
over the family's own table (_lib.FAMILIES["deconv"], include/modet_hip_deconv.h).  Every caller-supplied tensor sits between guard
bands (tests/guard.py), every workspace is exactly modet_deconv4s2_ws_bytes(..., pass) bytes, outputs and workspaces are poisoned,
and the library is reached through a recording proxy over the new table.  Per case: no band is damaged, every result is finite,
the results equal an unguarded run bit for bit, and a second guarded run with 0x00 instead of 0xFF bands and poison gives the same
bits.  The shapes: cases 1, 3, 4 and 6 of tests/test_gpu_deconv.py (a single input voxel, 3 -> 3 channels with scalar tails on both
sides, the 259-channel tail of x / d_x beside 16-byte loads of y, several tiles with a partial one in every axis) and cases 9, 10
and 12 (an activation with a Cout tail, so that y and d_y are read channel by channel up to the band, beside 16-byte rows of x at
20 -> 6 and 24 -> 13; the 35-channel tail of x beside 16-byte rows of y, the last row of workgroups partly empty)."""
import pytest
import torch

from tests import guard
from tests import rcn_oracle as orc
from tests.guard_family import DIM, UNSUP, Harness, StridedLayer

pytestmark = pytest.mark.gpu

H = Harness("deconv")
px = H.fixture()
S = StridedLayer(orc, "deconv4s2", "conv_transpose3d_k4s2", has_bias=lambda n: orc.OP_CASES[n][4], seed=4000)


CASES = {}
for _n in (1, 3, 4, 6):
    CASES["abi[case%d]" % _n] = S.abi_case(_n)
    CASES["ops[case%d]" % _n] = S.ops_case(_n)
for _n in (9, 10, 12):
    CASES["abi[case%d]" % _n] = S.abi_case(_n)
    CASES["ops[case%d]" % _n] = S.ops_case(_n)
CASES["abi[case6,no bias]"] = S.abi_case(6, bias=False)
CASES["abi[case3,bias]"] = S.abi_case(3, bias=True)
CASES["ops[case1,no bias]"] = S.ops_case(1, bias=False)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_deconv_between_guard_bands(px, tag):
    H.run_guarded(CASES[tag], px, tag)
    H.ran.add(tag)


def test_wrappers_refuse_before_any_launch(px):
    """the wrappers' argument checks run on the host: with the proxy in refuse mode nothing that launches may be reached"""
    from smilecode_amd import ops
    px.refuse = True
    x, w, b = torch.rand(1, 2, 3, 4, 8, device="cuda"), torch.rand(8, 16, 4, 4, 4, device="cuda"), torch.rand(16, device="cuda")
    f = ops.conv_transpose3d_k4s2
    for bad in (lambda: f(x.double(), w, b), lambda: f(x[0], w, b), lambda: f(x.cpu(), w, b), lambda: f(x.permute(0, 3, 2, 1, 4), w, b),
                lambda: f(x, w[:4].contiguous(), b), lambda: f(x, w, b[:8].contiguous()), lambda: f(x, w[..., :3].contiguous(), b),
                lambda: f(x, w.permute(1, 0, 2, 3, 4).contiguous(), b), lambda: f(x, w, b, -1.0), lambda: f(x, w, b, "relu"),
                lambda: f(x[:0], w, b), lambda: f(x, w[0], b)):
        with pytest.raises(RuntimeError):
            bad()
    assert not [n for n, _ in px.records if guard.is_launching(n)]
    px.refuse = False


def test_library_refuses_with_error_codes():
    """NULL pointers, channel counts outside the kernels', empty axes, a negative slope, a misaligned tensor and a short or misaligned
    workspace are answered with the library's error codes before any launch: the outputs keep their fill"""
    c = S.refusals((1, 2, 2, 2, 4, 8), (4, 8, 4, 4, 4), slope=0.1)
    ws_bytes = c.L.modet_deconv4s2_ws_bytes
    assert c.nb[0] == c.nb[1] == 64 * 4 * 8 * 4 and c.nb[2] == 2 * (64 * 4 * 8 + 8) * 4
    assert ws_bytes(*c.dims, 3) == 0 and ws_bytes(1, 2, 2, 2, 0, 8, 0) == 0
    assert ws_bytes(1, 2, 2, 2, 4, 1025, 0) == 0 and ws_bytes(1, 0, 2, 2, 4, 8, 0) == 0
    assert ws_bytes(1, 512, 512, 512, 4, 8, 0) == 0                                        # y of 2^33 elements
    assert ws_bytes(1, 2, 2, 2, 3, 3, 0) == 64 * 4 * 4 * 4                                 # the padded counts
    assert c.fwd(dims=(1, 2, 2, 2, 1025, 8)) == UNSUP and c.fwd(dims=(1, 2, 2, 2, 4, 0)) == DIM
    c.check()


def test_every_launching_deconv_entry_point_ran_between_guard_bands(px):
    """the coverage condition of tests/test_gpu_guard.py over the family's table; the NULL-able pointers -- the forward's bias, y
    of both backward entry points (absent without an activation) and the weight gradient's d_b -- were seen both present and absent"""
    H.check_coverage(px, CASES, {
        "modet_deconv4s2_fwd": ((2,), (0, 1, 3, 4)),                    # x w bias y ws | stream
        "modet_deconv4s2_bwd_data": ((1,), (0, 2, 3, 4)),               # d_y y w d_x ws | stream
        "modet_deconv4s2_bwd_weight": ((2, 4), (0, 1, 3, 5)),           # x d_y y d_w d_b ws | stream
    })
