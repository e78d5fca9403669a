"""The fused stride-2 4x4x4 transposed convolution (ops.conv_transpose3d_k4s2, csrc/deconv.hip) beside ATen's F.conv_transpose3d in
the reference's own form -- stride 2 without padding, then the crop [1:-1] of every axis and leaky_relu(0.1) -- on channels-last
memory, on the same GPU in the same process, the sides alternating -- per Upsamp*, Deconv* and Pred0 layer of VTN with channels = 8
on a 192^3 pair: forward (no gradient wanted) and forward + backward, time (HIP events: median, minimum, maximum) and peak
allocated memory above the inputs, and both sides' error against the same layer in ATen fp64 on the GPU.  The fused side is timed
twice per round (aten, fused, fused_again): the ratio of its two medians is the spread of repeated runs of the same code.  Then
the RCN train step (n_cascade 2 and 10), eager and captured, beside ModeT's in the same process.

    python tools/bench_rcn.py [--steps 30] [--shape 192,192,192] [--channels 8] [--train-steps 30] [--json profiles/bench_rcn.json]"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smilecode_amd import models, ops  # noqa: E402
from tools import bench_layer  # noqa: E402

SLOPE = 0.1


def layer_case(B, grid, Cin, Cout, bias, act, steps):
    D, H, W = grid
    g = torch.Generator(device="cuda").manual_seed(11 + Cin)
    x = torch.randn((B, D, H, W, Cin), device="cuda", generator=g)
    w = (torch.randn((Cin, Cout, 4, 4, 4), device="cuda", generator=g) / (8 * Cin) ** 0.5).requires_grad_(True)
    b = (torch.randn(Cout, device="cuda", generator=g) * 0.1).requires_grad_(True) if bias else None
    gy = torch.randn((B, 2 * D, 2 * H, 2 * W, Cout), device="cuda", generator=g)

    def ref_layer(a, wt, bt):
        y = F.conv_transpose3d(a, wt, bt, stride=2)[:, :, 1:-1, 1:-1, 1:-1]
        return F.leaky_relu(y, SLOPE) if act else y

    return bench_layer.layer_case(x, w, b, gy, lambda a, wt, bt: ops.conv_transpose3d_k4s2(a, wt, bt, SLOPE if act else None), ref_layer,
                                  128.0 * Cin * Cout * (x.numel() // Cin), steps, act=act)


def vtn_layers(shape, c):
    """(name, input grid, Cin, Cout, bias, act) of every transposed convolution of VTN"""
    g = lambda k: tuple(s // k for s in shape)          # noqa: E731
    out = [("Upsamp6to5", g(64), 3, 3, False, False), ("Deconv5", g(64), 32 * c, 16 * c, True, True)]
    for lvl, k in ((5, 16), (4, 8), (3, 4), (2, 2)):
        cin = 2 * k * c + 3
        out += [("Upsamp%dto%d" % (lvl, lvl - 1), g(2 ** lvl), 3, 3, False, False),
                ("Deconv%d" % (lvl - 1), g(2 ** lvl), cin, k * c // 2, True, True)]
    return out + [("Pred0", g(2), 2 * c + 3, 3, False, False)]


def layers(shape, c, steps):
    for name, grid, cin, cout, bias, act in vtn_layers(shape, c):
        yield name, grid, cin, cout, layer_case(1, grid, cin, cout, bias, act, steps)


def make_rcn(shape, channels, n_cascade):
    """the reference's initialisation except for Pred0: Normal(0, 1e-5) leaves every flow at zero, so it gets weights that move the
    flow by a fraction of a voxel"""
    torch.manual_seed(24)
    m = models.RCN(shape, flow_multiplier=2, channels=channels, n_cascade=n_cascade, return_subflows=True).cuda()
    g = torch.Generator().manual_seed(24)
    with torch.no_grad():
        for v in m.vtn:
            w = v.Pred0.upconv.weight
            w.copy_(torch.randn(w.shape, generator=g) * (0.05 / (8 * w.shape[0]) ** 0.5))
    return m


def main():
    ap = bench_layer.parser("192,192,192", 8)
    ap.add_argument("--cascades", default="2,10")
    args = ap.parse_args()
    nets = [("rcn%d" % int(n), (lambda s, n=int(n): make_rcn(s, args.channels, n))) for n in args.cascades.split(",") if n]
    bench_layer.run("bench_rcn", args, layers, nets, form="plain fp32 FMA on LDS tiles (no matrix-instruction form is built)")


if __name__ == "__main__":
    main()
