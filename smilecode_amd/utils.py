"""Evaluation helpers with the reference's names (ModeT/utils.py:8-106): ``AverageMeter``,
``register_model`` (label / image warp) and ``dice_val_VOI`` -- the Dice-parity harness of
train.py:143-155 / infer.py:86-92, with the label warp and the per-label counting on the GPU."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import ops
from .models import SpatialTransformer


class AverageMeter(object):
    """Computes and stores the average and current value (reference utils.py:8-27)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0
        self.vals = []
        self.std = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        self.vals.append(val)
        self.std = np.std(self.vals)


class register_model(nn.Module):
    """``register_model(img_size, mode)([img, flow])`` (reference utils.py:74-83)."""

    def __init__(self, img_size=(64, 256, 256), mode="bilinear"):
        super().__init__()
        self.spatial_trans = SpatialTransformer(img_size, mode)

    def forward(self, x):
        img = x[0].cuda().float()
        flow = x[1].cuda()
        return self.spatial_trans(img, flow)


def dice_from_counts(counts, nlabels=54):
    """mean over labels 1..nlabels of 2*n(A&B)/(n(A)+n(B)+1e-5) (arithmetic of reference utils.py:95-105)."""
    c = counts.detach().cpu().numpy().astype(np.float64)
    pred, true, inter = c[0, 1:nlabels + 1], c[1, 1:nlabels + 1], c[2, 1:nlabels + 1]
    return float(np.mean(2.0 * inter / (pred + true + 1e-5)))


def dice_val_VOI(y_pred, y_true, nlabels=54):
    """Dice over the 54 LPBA VOIs of the first batch element (reference utils.py:86-106).
    Inputs are label tensors (B,1,D,H,W); counting runs on the GPU with a zero flow."""
    p = y_pred[0, 0].to(torch.int16).cuda().contiguous()
    t = y_true[0, 0].to(torch.int16).cuda().contiguous()
    zero = torch.zeros((1,) + tuple(p.shape) + (3,), dtype=torch.float32, device=p.device)
    _, counts = ops.label_warp_counts(p, zero, t, nlabels, want_warped=False)
    return np.float64(dice_from_counts(counts, nlabels))


def warp_labels_and_dice(x_seg, flow, y_seg, nlabels=54):
    """fused evaluation tail: nearest-warp ``x_seg`` by ``flow`` (B=1, NCDHW) and score against ``y_seg``.
    Returns (warped labels (1,1,D,H,W) int16, dice).  Equivalent to reg_model([x_seg.float(), flow]) followed by
    dice_val_VOI (train.py:152-153) without the float round trip and the 54 numpy passes."""
    flow_cl = ops.to_channels_last(flow.float().contiguous())
    warped, counts = ops.label_warp_counts(x_seg[0, 0].to(torch.int16).cuda(), flow_cl[:1].contiguous(),
                                           y_seg[0, 0].to(torch.int16).cuda(), nlabels)
    return warped[None, None], dice_from_counts(counts, nlabels)


def jacobian_nonpositive_fraction(flow):
    """fraction of voxels with det(J) <= 0 per sample, as infer.py:89-90 reports it (np.sum(jac_det <= 0) / n_voxels),
    computed on the GPU from the model's flow (B,3,D,H,W): no D2H of the field, one integer per sample comes back."""
    flow_cl = ops.to_channels_last(flow.float().contiguous())
    counts, _ = ops.jacdet_nonpos_count(flow_cl)
    nvox = float(flow.shape[2] * flow.shape[3] * flow.shape[4])
    return [float(c) / nvox for c in counts.tolist()]


def jacobian_determinant_vxm(disp):
    """Jacobian determinant of a (3,D,H,W) displacement field (reference utils.py:108-150): float64 (D,H,W) numpy array,
    computed by the HIP kernel in the reference's operation order (np.gradient differences of flow + identity grid,
    first-row expansion).  Accepts a numpy array or a tensor, as the reference's callers pass `flow.cpu().numpy()[0]`."""
    t = torch.as_tensor(np.ascontiguousarray(disp) if isinstance(disp, np.ndarray) else disp).float().cuda()
    flow_cl = t.permute(1, 2, 3, 0).contiguous()[None]
    _, det = ops.jacdet_nonpos_count(flow_cl, want_det=True)
    return det[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ surface distances
# hd_val, hd95_val and assd_val of the reference's Baseline methods/RDN/utils.py:94-116 (medpy's metric.hd / hd95 / assd per label)
# from ONE device call (ops.surface_distances): nothing but the (nlabels, 5) and (nlabels, 7) result tables comes back.
_SURFACE_COLUMN = {"hd": 0, "hd95": 1, "assd": 2}
_SURFACE_EMPTY = ("The first supplied array does not contain any binary object.",
                  "The second supplied array does not contain any binary object.")


def _label_volume(name, a):
    """one (D,H,W) int16 label map on the GPU from a numpy array or a tensor; leading singleton axes of (1,1,D,H,W) are dropped"""
    t = torch.as_tensor(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if not torch.is_tensor(t):
        raise RuntimeError(f"surface distances: {name} must be a numpy array or a tensor, got {type(a).__name__}")
    if t.dim() > 3 and any(int(s) != 1 for s in t.shape[:-3]):
        raise RuntimeError(f"surface distances: {name} {tuple(t.shape)} holds more than one volume (B > 1 is not supported: "
                           "score one pair at a time)")
    if t.dim() < 3:
        raise RuntimeError(f"surface distances: {name} {tuple(t.shape)} is not a (D,H,W) volume (2-D maps are not supported)")
    return t.reshape(t.shape[-3:]).to(torch.int16).cuda().contiguous()


def _surface_tables(y_pred, y_true, nlabels, voxelspacing=None, connectivity=1):
    if voxelspacing is not None:
        raise RuntimeError("surface distances: voxelspacing other than None (unit spacing) is not supported")
    if connectivity != 1:
        raise RuntimeError(f"surface distances: connectivity {connectivity!r} is not supported (only 1, the 6 face neighbours)")
    p, t = _label_volume("y_pred", y_pred), _label_volume("y_true", y_true)
    metrics, counts = ops.surface_distances(p, t, int(nlabels), 95.0)
    return metrics.cpu().numpy(), counts.cpu().numpy()


def surface_vals(y_pred, y_true, C=None, *, voxelspacing=None, connectivity=1):
    """{"hd": [...], "hd95": [...], "assd": [...]}: the three lists of hd_val, hd95_val and assd_val from one device call.  Each
    is the reference's: one value per label 1..C with their mean appended; C defaults to the number of distinct values of y_true
    (np.unique(y_true).shape[0], as there).  A label in 1..C that is empty in y_pred (the first array medpy is handed) or y_true
    (the second) raises RuntimeError with medpy's message."""
    if not C:
        yt = torch.as_tensor(np.ascontiguousarray(y_true)) if isinstance(y_true, np.ndarray) else y_true
        C = int(torch.unique(yt).numel())
    metrics, counts = _surface_tables(y_pred, y_true, C, voxelspacing, connectivity)
    for i in range(C):
        for side in (0, 1):
            if counts[i, side] == 0:
                raise RuntimeError(_SURFACE_EMPTY[side])
    out = {}
    for name, col in _SURFACE_COLUMN.items():
        total = [np.float64(v) for v in metrics[:, col]]
        total.append(np.mean(total))
        out[name] = total
    return out


def assd_val(y_pred, y_true, C=None, *, voxelspacing=None, connectivity=1):
    """average symmetric surface distance per label 1..C and their mean (reference Baseline methods/RDN/utils.py:94-100)"""
    return surface_vals(y_pred, y_true, C, voxelspacing=voxelspacing, connectivity=connectivity)["assd"]


def hd_val(y_pred, y_true, C=None, *, voxelspacing=None, connectivity=1):
    """Hausdorff distance per label 1..C and their mean (reference Baseline methods/RDN/utils.py:102-108)"""
    return surface_vals(y_pred, y_true, C, voxelspacing=voxelspacing, connectivity=connectivity)["hd"]


def hd95_val(y_pred, y_true, C=None, *, voxelspacing=None, connectivity=1):
    """95th-percentile Hausdorff distance per label 1..C and their mean (reference Baseline methods/RDN/utils.py:110-116)"""
    return surface_vals(y_pred, y_true, C, voxelspacing=voxelspacing, connectivity=connectivity)["hd95"]


def surface_val_VOI(y_pred, y_true, nlabels=54):
    """{"hd95", "assd", "hd", "n_skipped"}: each metric's mean over the labels 1..nlabels present in BOTH maps, and how many labels
    were left out because one map lacks them (a small structure can vanish under a nearest-neighbour warp; that must not end an
    evaluation run).  All labels missing: the means are NaN.  Inputs as _label_volume takes them, e.g. (1,1,D,H,W) label tensors."""
    metrics, counts = _surface_tables(y_pred, y_true, nlabels)
    present = (counts[:, 0] > 0) & (counts[:, 1] > 0)
    out = {name: (float(np.mean(metrics[present, col])) if present.any() else float("nan")) for name, col in _SURFACE_COLUMN.items()}
    out["n_skipped"] = int((~present).sum())
    return out
