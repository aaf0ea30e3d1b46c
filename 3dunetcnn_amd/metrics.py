"""Scoring a predicted mask against the ground truth on the device (csrc/metrics.hip): what BraTS and SPPIN are ranked by.

  confusion_counts / dice_score / iou / sensitivity / precision   hard-mask overlap, from exact integer counts
  mask_edges                 mask ^ scipy.ndimage.binary_erosion(mask) (faces; outside the volume = background)
  distance_transform_edt     scipy.ndimage.distance_transform_edt(mask, sampling=...): exact, brute-force separable
  distance_to                distance from every voxel to the nearest nonzero voxel of `sites`
  surface_distances          Hausdorff, percentile Hausdorff (numpy's linear percentile) and average surface distance
  evaluate                   all of them in one call, e.g. on the mask prepost.finish_prediction returns

Masks are [D, H, W] or [C, D, H, W] of any dtype, nonzero = foreground, every channel on its own; results have a leading [C] ([1] for a
3-D mask). The symmetric forms -- hausdorff = max of the two directed values, average_surface_distance = (sum_ab + sum_ba) / (n_a + n_b)
-- and the empty-set rules (both edge sets empty: 0; exactly one empty: +inf) are this project's convention. They follow what MONAI
documents for compute_hausdorff_distance(percentile=...) and the symmetric compute_average_surface_distance; MONAI is not installed
here and no parity with a MONAI release is claimed.

Inputs and outputs live on the GPU; nothing here waits for the device or reads a value back. There is no CPU fallback.
"""
from typing import NamedTuple

import torch

from . import ops as _ops
from .prepost import _mask4


def _be(t, be=None):
    if be is not None:
        return be
    if t.device.type != "cuda":
        raise RuntimeError("3dunetcnn_amd.metrics runs on an MI355X only (no CPU fallback)")
    return _ops.default_backend(t.device)


def _pair(pred, truth):
    p, t = _mask4(pred), _mask4(truth)
    if p.shape != t.shape:
        raise ValueError(f"pred {tuple(p.shape)} and truth {tuple(t.shape)} differ in shape")
    return p, t


def _spacing(sampling):
    if sampling is None:
        return (1.0, 1.0, 1.0)
    if isinstance(sampling, (int, float)):
        return (float(sampling),) * 3
    s = tuple(float(v) for v in sampling)
    if len(s) != 3:
        raise ValueError("sampling / spacing: one value per axis (z, y, x)")
    return s


class SurfaceDistances(NamedTuple):
    hausdorff: torch.Tensor                   # fp32 [C]: max(hd_ab, hd_ba)
    hausdorff_percentile: torch.Tensor        # fp32 [C]: max(pct_ab, pct_ba)
    average_surface_distance: torch.Tensor    # fp32 [C]: (sum_ab + sum_ba) / (n_a + n_b)
    directed: torch.Tensor                    # fp32 [C, 5]: hd_ab, hd_ba, pct_ab, pct_ba, asd_ab (a = pred, b = truth)
    edge_counts: torch.Tensor                 # int32 [C, 2]: edge voxels of pred, of truth


class Evaluation(NamedTuple):
    counts: torch.Tensor                      # int32 [C, 4]: TP, FP, FN, TN
    dice: torch.Tensor
    iou: torch.Tensor
    sensitivity: torch.Tensor
    precision: torch.Tensor
    hausdorff: torch.Tensor
    hausdorff_percentile: torch.Tensor
    average_surface_distance: torch.Tensor
    directed: torch.Tensor
    edge_counts: torch.Tensor


def confusion_counts(pred, truth, _backend=None):
    """-> int32 [C, 4] = (TP, FP, FN, TN) per channel, exact."""
    p, t = _pair(pred, truth)
    return _be(p, _backend).seg_counts(p, t)


def _ratio(num, den, empty):
    """num / den of exact int64 counts, divided in float64 and rounded to fp32; `empty` where den == 0."""
    q = (num.to(torch.float64) / den.to(torch.float64)).to(torch.float32)
    return torch.where(den == 0, torch.full_like(q, empty), q)


def dice_from_counts(counts):
    c = counts.to(torch.int64)                # 2 TP + FP + FN of a 2^31-voxel volume does not fit int32
    return _ratio(2 * c[:, 0], 2 * c[:, 0] + c[:, 1] + c[:, 2], 1.0)


def iou_from_counts(counts):
    c = counts.to(torch.int64)
    return _ratio(c[:, 0], c[:, 0] + c[:, 1] + c[:, 2], 1.0)


def sensitivity_from_counts(counts):
    c = counts.to(torch.int64)
    return _ratio(c[:, 0], c[:, 0] + c[:, 2], float("nan"))


def precision_from_counts(counts):
    c = counts.to(torch.int64)
    return _ratio(c[:, 0], c[:, 0] + c[:, 1], float("nan"))


def dice_score(pred, truth, _backend=None):
    """2 TP / (2 TP + FP + FN) per channel, fp32 [C]; 1.0 when both masks are empty."""
    return dice_from_counts(confusion_counts(pred, truth, _backend))


def iou(pred, truth, _backend=None):
    """TP / (TP + FP + FN) per channel; 1.0 when both masks are empty."""
    return iou_from_counts(confusion_counts(pred, truth, _backend))


def sensitivity(pred, truth, _backend=None):
    """TP / (TP + FN) per channel; NaN when the truth is empty."""
    return sensitivity_from_counts(confusion_counts(pred, truth, _backend))


def precision(pred, truth, _backend=None):
    """TP / (TP + FP) per channel; NaN when the prediction is empty."""
    return precision_from_counts(confusion_counts(pred, truth, _backend))


def mask_edges(mask, _backend=None):
    """Foreground voxels with at least one background face neighbour (a neighbour outside the volume is background) -> uint8, same shape."""
    m = _mask4(mask)
    e = _be(m, _backend).mask_edges(m)
    return e if mask.dim() == 4 else e[0]


def distance_transform_edt(mask, sampling=None, _backend=None):
    """scipy.ndimage.distance_transform_edt(mask, sampling=sampling): the distance from every nonzero voxel to the nearest zero voxel, 0 on
    the background; +inf in a channel without a zero voxel (scipy has no answer there). fp32, same shape."""
    m = _mask4(mask)
    d = _be(m, _backend).edt(m, _spacing(sampling), invert=True, sqrt=True)
    return d if mask.dim() == 4 else d[0]


def distance_to(sites, sampling=None, squared=False, _backend=None):
    """The distance (squared=True: its square, integers for unit sampling) from every voxel to the nearest nonzero voxel of `sites`; +inf
    in a channel without one."""
    m = _mask4(sites)
    d = _be(m, _backend).edt(m, _spacing(sampling), invert=False, sqrt=not squared)
    return d if sites.dim() == 4 else d[0]


def surface_distances(pred, truth, spacing=(1, 1, 1), percentile=95.0, _backend=None):
    """Distances between the edge voxels (mask_edges) of pred and of truth: two mask_edges, two distance transforms, one statistics op."""
    p, t = _pair(pred, truth)
    be, sp = _be(p, _backend), _spacing(spacing)
    ea, eb = be.mask_edges(p), be.mask_edges(t)
    to_b, to_a = be.edt(eb, sp, sqrt=False), be.edt(ea, sp, sqrt=False)
    out, n = be.surface_stats(ea, eb, to_b, to_a, percentile)
    return SurfaceDistances(out[:, 0], out[:, 1], out[:, 2], out[:, 3:8], n)


def evaluate(pred, truth, spacing=(1, 1, 1), percentile=95.0, _backend=None):
    """Overlap and surface metrics of pred against truth in one call -> Evaluation."""
    p, t = _pair(pred, truth)
    counts = confusion_counts(p, t, _backend)
    s = surface_distances(p, t, spacing, percentile, _backend)
    return Evaluation(counts, dice_from_counts(counts), iou_from_counts(counts), sensitivity_from_counts(counts),
                      precision_from_counts(counts), s.hausdorff, s.hausdorff_percentile, s.average_surface_distance, s.directed,
                      s.edge_counts)
