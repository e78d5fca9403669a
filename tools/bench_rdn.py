"""The fused stride-2 convolution (ops.conv3d_s2, csrc/convs2.hip) beside ATen's F.conv3d(stride=2, padding=1) + leaky_relu(0.2) in
channels-last memory format, on the same GPU in the same process, the sides alternating -- per encoder layer of RDN with
channels = 16 at the [moving; fixed] batch of a 160x192x160 pair: forward (no gradient wanted) and forward + backward, time (HIP
events: median, minimum, maximum) and peak allocated memory above the inputs.  The fused side is timed twice per round (aten,
fused, fused_again): the ratio of its two medians is the spread of repeated runs of the same code.  The first layer's input is
the image: neither side computes a data gradient for it.  Then the RDN train step (channels = 16, one pass per level), eager and
captured, beside ModeT's.

    python tools/bench_rdn.py [--steps 30] [--shape 160,192,160] [--channels 16] [--train-steps 30] [--json profiles/bench_rdn.json]

tools/bench_layer.py has the measurement and says what each figure is."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops  # noqa: E402
from tools import bench_layer  # noqa: E402

SLOPE = 0.2


def layer_case(B, grid, Cin, Cout, steps, x_grad):
    D, H, W = grid
    g = torch.Generator(device="cuda").manual_seed(7 + Cin)
    x = torch.randn((B, D, H, W, Cin), device="cuda", generator=g)
    w = (torch.randn((Cout, Cin, 3, 3, 3), device="cuda", generator=g) / (27 * Cin) ** 0.5).requires_grad_(True)
    b = (torch.randn(Cout, device="cuda", generator=g) * 0.1).requires_grad_(True)
    Do, Ho, Wo = ops.conv3d_s2_out_shape(D, H, W)
    gy = torch.randn((B, Do, Ho, Wo, Cout), device="cuda", generator=g)
    # the same bytes as a (Cout,Cin,3,3,3) tensor in channels_last_3d memory format: what ATen's channels-last path takes
    w_cl = w.detach().contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    return bench_layer.layer_case(x, w, b, gy, lambda a, wt, bt: ops.conv3d_s2(a, wt, bt, SLOPE),
                                  lambda a, wt, bt: F.leaky_relu(F.conv3d(a, wt, bt, stride=2, padding=1), SLOPE),
                                  54.0 * Cin * Cout * (gy.numel() // Cout), steps, x_grad=x_grad, w_aten=w_cl)


def make_rdn(shape, channels):
    """the reference's initialisation except for the flow convolutions: Normal(0, 1e-5) leaves every field at zero, so they get
    weights that move the flow by a fraction of a voxel"""
    torch.manual_seed(24)
    m = models.RDN(shape, channels=channels).cuda()
    g = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for est in (m.est0[0], m.est1[0], m.est2[0], m.est3[0]):
            w = est.conv[4].weight
            w.copy_(torch.randn(w.shape, generator=g) * (0.3 / (27 * w.shape[1]) ** 0.5))
    return m


def layers(shape, c, steps):
    """(name, input grid, Cin, Cout, measured) of every encoder layer at the [moving; fixed] batch; the first reads the image"""
    for i, (cin, cout) in enumerate([(1, c), (c, 2 * c), (2 * c, 4 * c), (4 * c, 8 * c)]):
        grid = tuple(s // 2 ** i for s in shape)
        yield "conv%d" % i, grid, cin, cout, layer_case(2, grid, cin, cout, steps, x_grad=i > 0)


def main():
    args = bench_layer.parser("160,192,160", 16).parse_args()
    bench_layer.run("bench_rdn", args, layers, [("rdn", lambda s: make_rdn(s, args.channels))])


if __name__ == "__main__":
    main()
