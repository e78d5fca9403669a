"""``NCC_vxm`` and ``Grad3d`` with the reference's class names and call signatures
(ModeT/losses.py:6-94), computed by the HIP kernels of csrc/losses.hip; ``MIND_loss`` (Baseline methods/RCN/losses.py:333-399)
by those of csrc/mind.hip; ``MutualInformation`` and ``localMutualInformation`` (the same file, 401-556) by those of csrc/mi.hip;
``SSIM3D`` and ``ssim3D`` (the same file, 103-148) by those of csrc/ssim.hip; ``Grad3DiTV`` and ``DisplacementRegularizer``
(the same file, 203-268) by those of csrc/reg.hip; ``LabelDice``, the label-overlap term of weakly supervised training, by those of
csrc/segdice.hip."""
from __future__ import annotations

from functools import partial

import torch

from . import ops


class Grad3d(torch.nn.Module):
    """N-D gradient loss (reference losses.py:6-31): penalty 'l1' (the class default) or 'l2' (what train.py:104 uses)."""

    def __init__(self, penalty="l1", loss_mult=None):
        super().__init__()
        if penalty not in ("l1", "l2"):
            raise RuntimeError(f"Grad3d: unknown penalty {penalty!r} (the reference knows 'l1' and 'l2', losses.py:21)")
        self.penalty = penalty
        self.loss_mult = loss_mult

    def forward(self, y_pred, y_true=None):
        grad = ops.grad3d_loss(y_pred.contiguous(), self.penalty)
        if self.loss_mult is not None:
            grad = grad * self.loss_mult
        return grad

    def seedable(self):
        return self.loss_mult is None

    def value_and_grad_cl(self, flow_cl, grad_scale):
        return ops.grad3d_value_and_grad_cl(flow_cl, self.penalty, grad_scale)


class NCC_vxm(torch.nn.Module):
    """local normalized cross correlation loss over windows of ``win`` voxels (reference losses.py:34-94); ``win`` = None (the
    reference's default [9, 9, 9], what train.py:103 uses) or any [wz, wy, wx].  The reference pads EVERY axis by
    floor(win[0] / 2) (losses.py:57), so an even or anisotropic window averages cc over a grid that differs from the volume's
    by a voxel or more per axis -- reproduced as is.  Cubic windows of 3 / 5 / 7 / 9 voxels run the z-marching kernel, all
    others the general separable path (csrc/losses.hip)."""

    def __init__(self, win=None):
        super().__init__()
        w = [9, 9, 9] if win is None else [int(v) for v in win]
        if len(w) != 3 or min(w) < 1:
            raise RuntimeError(f"NCC_vxm: 3-D volumes take a window of three positive sizes, got {win}")
        self.win = win
        self._w = w

    def forward(self, y_true, y_pred):
        return ops.ncc_loss(y_true.contiguous(), y_pred.contiguous(), self._w)

    def seedable(self):
        """a cubic window of 3 / 5 / 7 / 9 voxels: what the scaled entry point has"""
        return len(set(self._w)) == 1 and self._w[0] in (3, 5, 7, 9)

    def value_and_grad(self, fixed, moved, grad_scale):
        return ops.ncc_value_and_grad(fixed, moved, self._w[0], grad_scale)


class MIND_loss(torch.nn.Module):
    """MIND-SSC descriptor distance (reference Baseline methods/RCN/losses.py:333-399): mean((MINDSSC(y_pred) - MINDSSC(y_true))^2)
    with radius 2 and dilation 2, the similarity for multi-modal pairs.  ``win`` is accepted and unused, as in the reference."""

    def __init__(self, win=None):
        super().__init__()
        self.win = win

    def MINDSSC(self, img, radius=2, dilation=2):
        return ops.mind_ssc(img.contiguous(), radius, dilation)

    def forward(self, y_pred, y_true):
        ops._pair_shapes("MIND_loss", y_pred, y_true, "y_pred", "y_true")
        return ops.mind_loss(y_pred.contiguous(), y_true.contiguous())

    def seedable(self):
        return True

    def value_and_grad(self, fixed, moved, grad_scale):
        return ops.mind_value_and_grad(fixed, moved, grad_scale)


class _ParzenMI(torch.nn.Module):
    """what the two mutual-information terms share: the bins' parameters and their checks"""

    def __init__(self, sigma_ratio, minval, maxval, num_bin):
        super().__init__()
        if int(num_bin) != ops.MI_BINS:
            raise RuntimeError(f"{type(self).__name__}: only num_bin = {ops.MI_BINS} exists, got {num_bin}")
        if not (maxval > 0 and maxval > minval and sigma_ratio > 0):
            raise RuntimeError(f"{type(self).__name__}: needs maxval > 0, maxval > minval and sigma_ratio > 0, got minval {minval}, "
                               f"maxval {maxval}, sigma_ratio {sigma_ratio}")
        self.sigma_ratio, self.minval, self.maxval, self.num_bins = sigma_ratio, minval, maxval, int(num_bin)
        self.max_clip = maxval


class MutualInformation(_ParzenMI):
    """-mutual information over 32 Gaussian Parzen-window bins between ``minval`` and ``maxval`` (reference Baseline
    methods/RCN/losses.py:401-457), the first choice for CT / MR or T1 / T2 pairs.  Intensities are clamped to [0, maxval] as in
    the reference; only ``num_bin`` = 32 exists (the kernels' tile)."""

    def __init__(self, sigma_ratio=1, minval=0., maxval=1., num_bin=32):
        super().__init__(sigma_ratio, minval, maxval, num_bin)

    def forward(self, y_true, y_pred):
        ops._pair_shapes("MutualInformation", y_true, y_pred, "y_true", "y_pred")
        return ops.mi_loss(y_true.contiguous(), y_pred.contiguous(), self.sigma_ratio, self.minval, self.maxval, self.num_bins)

    def seedable(self):
        return True

    def value_and_grad(self, fixed, moved, grad_scale):
        return ops.mi_value_and_grad(fixed, moved, self.sigma_ratio, self.minval, self.maxval, self.num_bins, grad_scale)


class localMutualInformation(_ParzenMI):
    """the same per non-overlapping patch of ``patch_size``^3 voxels of the zero-padded volumes, averaged over all patches
    (reference Baseline methods/RCN/losses.py:459-556); patch sizes 1..16."""

    def __init__(self, sigma_ratio=1, minval=0., maxval=1., num_bin=32, patch_size=5):
        super().__init__(sigma_ratio, minval, maxval, num_bin)
        if int(patch_size) != patch_size or not 1 <= int(patch_size) <= ops.MI_MAX_PATCH:
            raise RuntimeError(f"localMutualInformation: patch_size must be an integer in 1..{ops.MI_MAX_PATCH}, got {patch_size}")
        self.patch_size = int(patch_size)

    def forward(self, y_true, y_pred):
        ops._pair_shapes("localMutualInformation", y_true, y_pred, "y_true", "y_pred")
        return ops.lmi_loss(y_true.contiguous(), y_pred.contiguous(), self.sigma_ratio, self.minval, self.maxval, self.num_bins,
                            self.patch_size)

    def seedable(self):
        return True

    def value_and_grad(self, fixed, moved, grad_scale):
        return ops.lmi_value_and_grad(fixed, moved, self.sigma_ratio, self.minval, self.maxval, self.num_bins, self.patch_size,
                                      grad_scale)


def _ssim_check(name, img1, img2, window_size, size_average):
    if not size_average:
        raise RuntimeError(f"{name}: size_average=False is not built (the reference's per-axis means of a 5-D map yield a (B, W) "
                           "tensor)")
    if not (int(window_size) == window_size and 1 <= int(window_size) <= ops.SSIM_MAX_WINDOW and int(window_size) % 2 == 1):
        raise RuntimeError(f"{name}: window_size must be an odd integer in 1..{ops.SSIM_MAX_WINDOW}, got {window_size}")
    if img1 is not None:
        ops._pair_shapes(name, img1, img2, "img1", "img2")


class SSIM3D(torch.nn.Module):
    """1 - mean structural similarity under a zero-padded Gaussian window (sigma 1.5) of ``window_size``^3 voxels (reference
    Baseline methods/RCN/losses.py:103-126).  Odd windows 1..11, one channel, ``size_average=True`` only."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        _ssim_check("SSIM3D", None, None, window_size, size_average)
        self.window_size, self.size_average, self.channel = int(window_size), True, 1

    def forward(self, img1, img2):
        _ssim_check("SSIM3D", img1, img2, self.window_size, self.size_average)
        return ops.ssim_loss(img1.contiguous(), img2.contiguous(), self.window_size)

    def seedable(self):
        return True

    def value_and_grad(self, fixed, moved, grad_scale):
        return ops.ssim_value_and_grad(fixed, moved, self.window_size, grad_scale)


def ssim3D(img1, img2, window_size=11, size_average=True):
    """the mean structural similarity itself, 1 - SSIM3D (reference Baseline methods/RCN/losses.py:140-148)"""
    _ssim_check("ssim3D", img1, img2, window_size, size_average)
    return 1.0 - ops.ssim_loss(img1.contiguous(), img2.contiguous(), int(window_size))


def _flow_check(name, flow, kind):
    if not torch.is_tensor(flow) or flow.dim() != 5 or (kind != "itv" and flow.shape[1] != 3):
        want = "(B,C,D,H,W)" if kind == "itv" else "(B,3,D,H,W)"
        raise RuntimeError(f"{name}: expects a planar {want} flow, got {tuple(flow.shape) if torch.is_tensor(flow) else type(flow)}")
    if flow.shape[0] < 1 or flow.shape[1] < 1 or min(flow.shape[2:]) < ops.REG_MIN_SIZE[kind]:
        raise RuntimeError(f"{name}: '{kind}' needs D, H, W >= {ops.REG_MIN_SIZE[kind]} (the reference's mean of no points is NaN), "
                           f"got {tuple(flow.shape)}")


class Grad3DiTV(torch.nn.Module):
    """isotropic total variation of a flow (reference Baseline methods/RCN/losses.py:203-221): the mean over the points with
    z, y, x >= 1 of sqrt(|backward differences|^2 + 1e-6), divided by 3.  Any channel count; ``y_true`` is unused."""

    def forward(self, y_pred, y_true=None):
        _flow_check("Grad3DiTV", y_pred, "itv")
        return ops.reg_loss(y_pred.contiguous(), "itv")

    def seedable(self):
        return True

    def value_and_grad_cl(self, flow_cl, grad_scale):
        return ops.reg_value_and_grad_cl(flow_cl, "itv", grad_scale)


class DisplacementRegularizer(torch.nn.Module):
    """'bending', 'gradient-l2' or 'gradient-l1' energy of a 3-channel displacement field from central differences on its
    interior (reference Baseline methods/RCN/losses.py:223-268).  An unknown ``energy_type`` is refused here, not at the first
    call, and so is a field that does not have exactly 3 channels (the reference reads channels 0..2 of a wider one)."""

    def __init__(self, energy_type):
        super().__init__()
        if energy_type not in ("bending", "gradient-l2", "gradient-l1"):
            raise RuntimeError(f"DisplacementRegularizer: unknown energy_type {energy_type!r} (the reference knows 'bending', "
                               "'gradient-l2' and 'gradient-l1', losses.py:259-267)")
        self.energy_type = energy_type

    def forward(self, disp, _=None):
        _flow_check("DisplacementRegularizer", disp, self.energy_type)
        return ops.reg_loss(disp.contiguous(), self.energy_type)

    def seedable(self):
        return True

    def value_and_grad_cl(self, flow_cl, grad_scale):
        return ops.reg_value_and_grad_cl(flow_cl, self.energy_type, grad_scale)


class LabelDice(torch.nn.Module):
    """1 - mean soft Dice over the labels 1..``nlabels`` of the moving label map warped TRILINEARLY by the flow against the fixed
    one: the overlap term of weakly supervised training, the differentiable form of the Dice that ``infer`` reports (reference
    utils.py:86-106 for the score and its 1e-5).  ``flow`` (B,3,D,H,W) float32, label maps (B,1,D,H,W) int16; the gradient is
    with respect to the flow.  No one-hot volume exists at any point (csrc/segdice.hip)."""

    def __init__(self, nlabels=54):
        super().__init__()
        if isinstance(nlabels, bool) or not isinstance(nlabels, int) or not 1 <= nlabels <= ops.SEGDICE_MAX_LABELS:
            raise RuntimeError(f"LabelDice: nlabels must be an integer in 1..{ops.SEGDICE_MAX_LABELS}, got {nlabels!r}")
        self.nlabels = nlabels

    def forward(self, flow, moving_labels, fixed_labels):
        if not torch.is_tensor(flow) or flow.dim() != 5 or flow.shape[1] != 3:
            raise RuntimeError(f"LabelDice: expects a planar (B,3,D,H,W) flow, got "
                               f"{tuple(flow.shape) if torch.is_tensor(flow) else type(flow)}")
        return ops.seg_dice_loss(moving_labels, flow.contiguous(), fixed_labels, self.nlabels)

    def seedable(self):
        return True

    def value_and_grad_cl(self, flow_cl, moving_labels, fixed_labels, grad_scale, d_flow_add=None):
        return ops.seg_dice_value_and_grad_cl(flow_cl, moving_labels, fixed_labels, self.nlabels, grad_scale, d_flow_add)


def seeds(term):
    """the step may start its backward from the term's own gradient (``value_and_grad`` of a similarity term,
    ``value_and_grad_cl`` of a regulariser or a label term): the term is, by exact type, one of the classes of SIM_TERMS /
    REG_TERMS / SEG_TERMS below, and says that this configuration is seedable.  A subclass or a foreign module goes through
    autograd."""
    known = set(SIM_TERMS.values()) | {getattr(make, "func", make) for make in REG_TERMS.values()} | set(SEG_TERMS.values())
    return type(term) in known and term.seedable()


# the terms by the names train.py's --sim, --reg and --seg know: name -> what builds the term with the script's settings
SIM_TERMS = {"ncc": NCC_vxm, "mind": MIND_loss, "mi": MutualInformation, "lmi": localMutualInformation, "ssim": SSIM3D}
REG_TERMS = {"grad3d": partial(Grad3d, penalty="l2"), "itv": Grad3DiTV, "gradient-l2": partial(DisplacementRegularizer, "gradient-l2"),
             "gradient-l1": partial(DisplacementRegularizer, "gradient-l1"), "bending": partial(DisplacementRegularizer, "bending")}
SEG_TERMS = {"dice": LabelDice}
