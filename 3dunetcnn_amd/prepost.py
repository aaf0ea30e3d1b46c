"""On-device versions of the steps either side of the network, same signatures as the reference's.

  compile_one_hot_encoding      unet3d/utils/one_hot.py:7-37   (LabelMapToOneHot, transforms/one_hot.py:7-16)
  convert_one_hot_to_label_map  unet3d/utils/one_hot.py:44-118 (threshold / argmax / hierarchy decode)
  activate_and_decode           unet3d/predict/volumetric.py:151-156 + the decode above, one pass over the logits
  normalize_intensity           MONAI NormalizeIntensityD(channel_wise=True, nonzero=False | True), datasets/segmentation.py:77-86

  resize                        MONAI ResizeD(spatial_size, mode=("trilinear", "nearest")) = F.interpolate(size=...,
                                align_corners=False), datasets/segmentation.py:63-68
  resample_to_match             MONAI ResampleToMatch(mode) of a prediction onto the source image grid,
                                predict/volumetric.py:135-136, 168-170 (voxel map inv(A_src) @ A_dst; parity unpinned: MONAI absent)

  ensemble_mean / connected_components / keep_largest_component / finish_prediction
                                examples/sppin/process.py:258-274: np.mean over the cross-validation models' outputs, BinaryThreshold(0.5),
                                ConnectedComponent, RelabelComponent(sortByObjectSize=True), == 1

Inputs and outputs live on the GPU; there is no CPU fallback.
"""
import torch

from . import _lib
from . import ops as _ops


def _be(t, be=None):
    if be is not None:
        return be
    if t.device.type != "cuda":
        raise RuntimeError("3dunetcnn_amd.prepost runs on an MI355X only (no CPU fallback)")
    return _ops.default_backend(t.device)


def compile_one_hot_encoding(data, n_labels, labels=None, dtype=torch.uint8, return_4d=True, round=True, _backend=None):
    be = _be(data, _backend)
    while data.dim() < 5:
        data = data[None]
    assert data.shape[1] == 1
    if not round:
        raise NotImplementedError("round=False")
    groups = []
    for i in range(n_labels):
        if labels is not None:
            groups.append(list(labels[i]) if isinstance(labels[i], (list, tuple)) else [labels[i]])
        else:
            groups.append([i + 1])
    outs = [be.one_hot(data[n, 0].float().contiguous(), groups) for n in range(data.shape[0])]
    y = torch.stack(outs).to(dtype)
    if return_4d:
        assert y.shape[0] == 1
        y = y[0]
    return y


def convert_one_hot_to_label_map(one_hot_encoding, labels, axis=0, threshold=0.5, sum_then_threshold=False, dtype=torch.int16,
                                 label_hierarchy=False, _backend=None):
    if axis != 0:
        raise NotImplementedError("axis != 0")
    be = _be(one_hot_encoding, _backend)
    if not label_hierarchy and all(isinstance(l, (list, tuple)) for l in labels):
        maps, i = [], 0
        for sub in labels:                                   # one label-map volume per label group (one_hot.py:51-61)
            maps.append(convert_one_hot_to_label_map(one_hot_encoding[i:i + len(sub)], sub, axis, threshold, sum_then_threshold, dtype,
                                                     False, be))
            i += len(sub)
        return torch.stack(maps, dim=0)
    x = one_hot_encoding[:len(labels)].float().contiguous()
    _, lm = be.postprocess(x, None, threshold, labels, label_hierarchy, sum_then_threshold, want_probs=False, want_labels=True)
    return lm.to(dtype)


def activate_and_decode(logits, activation, labels, threshold=0.5, label_hierarchy=False, sum_then_threshold=False, _backend=None):
    """logits [C, D, H, W] of one sample -> (probabilities [C, D, H, W], int16 label map [D, H, W]) in one kernel."""
    be = _be(logits, _backend)
    return be.postprocess(logits.float().contiguous(), activation, threshold, labels, label_hierarchy, sum_then_threshold)


def normalize_intensity(image, channel_wise=True, nonzero=False, _backend=None):
    """image [C, D, H, W] (one sample) or [N, C, D, H, W]. nonzero=True (the usual setting for skull-stripped MR): the mean and the
    standard deviation (ddof 0) are those of the nonzero voxels of a channel and only those voxels change; a standard deviation of 0
    counts as 1 (MONAI's rule)."""
    if not channel_wise:
        raise NotImplementedError("only channel_wise=True (the shipped configs: brats2020_config.json:140-144)")
    be = _be(image, _backend)
    if nonzero:
        one = lambda x: be.zscore_select(x.float().contiguous(), _lib.SELECT_NONZERO, center=True, ddof=0, zero_std_to_one=True)[0]  # noqa: E731
    else:
        one = lambda x: be.zscore(x.float().contiguous())                                                                          # noqa: E731
    if image.dim() == 5:
        return torch.stack([one(image[n]) for n in range(image.shape[0])])
    return one(image)


def resize(img, spatial_size, mode="trilinear", _backend=None):
    """img [C, D, H, W] -> [C, *spatial_size]. "trilinear": F.interpolate(size=spatial_size, mode="trilinear",
    align_corners=False); "nearest": F.interpolate(mode="nearest") (source index floor(dst * in/out))."""
    be = _be(img, _backend)
    if mode not in ("trilinear", "nearest"):
        raise NotImplementedError(f"resize mode {mode!r}")
    x = img.float().contiguous()
    m = [0.0] * 12
    for i in range(3):
        sc = x.shape[1 + i] / float(spatial_size[i])
        m[4 * i + i] = sc
        m[4 * i + 3] = 0.5 * sc - 0.5 if mode == "trilinear" else 0.0
    return be.resample_affine(x, tuple(int(v) for v in spatial_size), m, "trilinear" if mode == "trilinear" else "nearest_floor", "border")


def resample_to_match(img, src_affine, dst_affine, dst_shape, mode="trilinear", padding_mode="border", _backend=None):
    """img [C, D, H, W] with voxel->world affine src_affine (4x4) resampled onto the grid (dst_shape, dst_affine):
    dst[c, v] = interp(img[c], inv(src_affine) @ dst_affine @ v). mode "trilinear"/"bilinear"/"nearest"; padding_mode
    "border"/"zeros"."""
    be = _be(img, _backend)
    a_src = torch.as_tensor(src_affine, dtype=torch.float64).cpu()
    a_dst = torch.as_tensor(dst_affine, dtype=torch.float64).cpu()
    m = (torch.linalg.inv(a_src) @ a_dst)[:3, :].reshape(-1).tolist()
    return be.resample_affine(img.float().contiguous(), tuple(int(v) for v in dst_shape), m, mode, padding_mode)


def _stacked(probabilities):
    if isinstance(probabilities, (list, tuple)):
        probabilities = torch.stack([p.float() for p in probabilities])
    if probabilities.dim() != 5:
        raise ValueError("probabilities: [M, C, D, H, W] or a list of [C, D, H, W]")
    return probabilities.float().contiguous()


def _connectivity(connectivity):
    """scipy.ndimage.generate_binary_structure(3, k): 1 = faces (ITK fullyConnected=False), 3 = faces + edges + corners (True)."""
    if connectivity == 2:
        raise NotImplementedError("connectivity=2 (18 neighbours): only 1 (faces) and 3 (full)")
    if connectivity not in (1, 3):
        raise ValueError(f"connectivity {connectivity!r}: 1 or 3")
    return 6 if connectivity == 1 else 26


def _mask4(mask):
    if mask.dim() not in (3, 4):
        raise ValueError("mask: [D, H, W] or [C, D, H, W]")
    m = mask if mask.dim() == 4 else mask[None]
    if m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8)
    return m.contiguous()


def ensemble_mean(probabilities, _backend=None):
    """[M, C, D, H, W] or a list of M [C, D, H, W] -> their mean [C, D, H, W] (np.mean(np.stack(...), axis=0), process.py:258-262):
    fp32 sum in index order, then a division by M."""
    x = _stacked(probabilities)
    return _be(x, _backend).ensemble_threshold(x, 0.5, want_mean=True, want_mask=False)[0]


def connected_components(mask, connectivity=1, _backend=None):
    """mask [D, H, W] or [C, D, H, W] (bool / uint8 / any: nonzero = foreground), every channel on its own -> (int32 labels of the same
    shape, int64 number of components per channel [C], or a 0-dim tensor for a 3-D mask). A label is 0 for background, otherwise
    1 + the smallest linear index (z*H + y)*W + x of its component: canonical, hence bitwise reproducible (ITK and scipy number
    components 1, 2, ... in raster order of their first voxel: the same ORDER). connectivity as generate_binary_structure(3, k)."""
    be, conn, m = _be(mask, _backend), _connectivity(connectivity), _mask4(mask)
    labels = be.cc_label(m, conn)
    v = m[0].numel()
    count = (labels.reshape(m.shape[0], v) == torch.arange(1, v + 1, dtype=torch.int32, device=labels.device)).sum(dim=1)
    return (labels, count) if mask.dim() == 4 else (labels[0], count[0])


def keep_largest_component(mask, connectivity=1, min_size=0, _backend=None):
    """The largest connected component of every channel (components smaller than min_size voxels never survive) -> uint8, same shape.
    Ties in size go to the component met first in raster order -- this project's rule (what a stable size sort of raster-order labels,
    and np.bincount(labels)[1:].argmax(), give; ITK itself is not installed here to compare against)."""
    be, conn, m = _be(mask, _backend), _connectivity(connectivity), _mask4(mask)
    out, _ = be.cc_filter(m, be.cc_label(m, conn), True, min_size)
    return out if mask.dim() == 4 else out[0]


def finish_prediction(probabilities, threshold=0.5, connectivity=1, keep_largest=True, min_size=0, _backend=None):
    """examples/sppin/process.py:258-274 in one call: mean of the M models' probabilities, mask = mean >= threshold (inclusive, as
    SimpleITK.BinaryThreshold's lower bound is -- activate_and_decode / convert_one_hot_to_label_map compare with >, as the
    reference's decode does; both are kept), connected components (ConnectedComponent: faces = connectivity 1), and the largest one
    per channel (RelabelComponent(sortByObjectSize=True) == 1) and / or those of at least min_size voxels.
    Returns (mean probabilities [C, D, H, W] fp32, uint8 mask [C, D, H, W]). ITK is not installed here: the tie rule between
    components of equal size is this project's (see keep_largest_component)."""
    x = _stacked(probabilities)
    be, conn = _be(x, _backend), _connectivity(connectivity)
    mean, mask = be.ensemble_threshold(x, threshold)
    if not keep_largest and min_size <= 1:
        return mean, mask
    out, _ = be.cc_filter(mask, be.cc_label(mask, conn), keep_largest, min_size)
    return mean, out
