"""On-device intensity normalisers, with the names and signatures of the reference's unet3d/utils/normalize.py and
unet3d/utils/threshold.py. Everything runs in the kernels of csrc/intensity.hip; thresholds stay on the device from the percentile
kernel that finds them to the window kernel that applies them, so nothing here waits for the host. There is no CPU fallback.

  percentiles                                 np.percentile(flat, q, axis=1): the building block, device fp32 [C, len(q)]
  percentile_threshold                        threshold.py:6-15 (the SPPIN config's "foreground_percentile")
  percentile_window                           normalize.py:16-20
  zero_one_window                             normalize.py:61-99
  zero_floor_normalize_image_data             normalize.py:46-58
  foreground_zero_mean_normalize_image_data   normalize.py:23-43
  window_data, radiology_style_windowing, static_windows      normalize.py:112-142

THE PERCENTILE RULE is numpy's default ("linear"), evaluated in double: position p = q / 100 * (n - 1), the two order statistics of rank
floor(p) and floor(p) + 1 found exactly, lo + (p - floor(p)) * (hi - lo) rounded once to fp32. That is what np.percentile gives for
float64 input. The reference's percentile_window / percentile_threshold hand numpy a float32 array, for which numpy 2.x evaluates the
position in float32 and lands tens of fp32 ulps away; zero_one_window and zero_floor_normalize_image_data call torch.percentile, which
does not exist (they were ported from numpy and raise AttributeError as written). All four follow the double rule here.

Not here: hist_match and histogram_normalize (they need unique / sort and MONAI).
"""
import torch

from . import _lib
from . import ops as _ops


def _be(t, be=None):
    if be is not None:
        return be
    if t.device.type != "cuda":
        raise RuntimeError("3dunetcnn_amd.normalize runs on an MI355X only (no CPU fallback)")
    return _ops.default_backend(t.device)


def _volume(data):
    return data.detach().float().contiguous()


def _per_channel(value, c, like):
    """A scalar or a length-c sequence / tensor of thresholds -> device fp32 [c]."""
    t = torch.as_tensor(value, dtype=torch.float32, device=like.device).reshape(-1)
    if t.numel() == 1:
        t = t.expand(c)
    if t.numel() != c:
        raise ValueError(f"{t.numel()} thresholds for {c} channels")
    return t.contiguous()


def percentiles(image, q, above=None, _backend=None):
    """image [C, ...] -> device fp32 [C, len(q)]: the q-th percentiles (0 .. 100) of every channel. above: None or device fp32 [C]: only
    the values strictly greater than above[c] take part. A channel with no participating value gives NaN; so does one with a NaN in it."""
    be = _be(image, _backend)
    q = [float(v) for v in (q if isinstance(q, (list, tuple)) else [q])]
    x = _volume(image)
    outs = [be.percentiles(x, q[i:i + _lib.PERCENTILE_MAX_Q], above)[0] for i in range(0, len(q), _lib.PERCENTILE_MAX_Q)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


def percentile_threshold(image, percentile, _backend=None):
    """image [C, D, H, W], percentile a FRACTION (0.9 = the 90th) -> bool [1, D, H, W]: voxels above their channel's percentile in any
    channel. The percentile handed on is percentile * 100 in Python double, as the reference computes it (0.9 * 100 = 90.00000000000001)."""
    be = _be(image, _backend)
    x = _volume(image)
    thr = be.percentiles(x, [percentile * 100])[0].reshape(-1)
    return be.threshold_any(x, thr)[None].bool()


def percentile_window(data, floor_percentile=5, ceiling_percentile=95, _backend=None):
    """torch.clamp(data, floor, ceiling) with the per-channel percentiles of data [C, ...] as bounds."""
    be = _be(data, _backend)
    x = _volume(data)
    thr = be.percentiles(x, [floor_percentile, ceiling_percentile])[0]
    return be.window(x, thr[:, 0].contiguous(), thr[:, 1].contiguous(), _lib.WINDOW_CLAMP)


def window_data(data, floor_threshold, ceiling_threshold, floor, ceiling, _backend=None):
    """(data - floor_threshold) / (ceiling_threshold - floor_threshold), values below `floor` set to it, values above `ceiling` set to it.
    data [C, ...]; the thresholds are scalars or one per channel (numbers or device tensors)."""
    be = _be(data, _backend)
    x = _volume(data)
    c = x.shape[0]
    return be.window(x, _per_channel(floor_threshold, c, x), _per_channel(ceiling_threshold, c, x), _lib.WINDOW_RESCALE, floor, ceiling)


def radiology_style_windowing(data, l, w, floor=0, ceiling=1, _backend=None):  # noqa: E741 -- the reference's argument names
    """Window of level l and width w: [l - w / 2, l + w / 2] -> [floor, ceiling]. data [D, H, W] or [C, D, H, W]."""
    x = data if data.dim() > 3 else data[None]
    y = window_data(x, l - w / 2, l + w / 2, floor, ceiling, _backend)
    return y if data.dim() > 3 else y[0]


def static_windows(data, windows, floor=0, ceiling=1, _backend=None):
    """data [D, H, W] (singleton axes are squeezed, as the reference does), windows a list of (level, width) -> [D, H, W, len(windows)],
    the windows in the last axis: one launch in which every output channel reads the one input volume."""
    be = _be(data, _backend)
    x = _volume(torch.squeeze(data))[None]
    lo = torch.tensor([l - w / 2 for l, w in windows], dtype=torch.float32, device=x.device)      # noqa: E741
    hi = torch.tensor([l + w / 2 for l, w in windows], dtype=torch.float32, device=x.device)      # noqa: E741
    return be.window(x, lo, hi, _lib.WINDOW_RESCALE, floor, ceiling, channels=len(windows)).movedim(0, -1)


def _channel_first(data, axis, what):
    """[C, D, H, W] with axis (1, 2, 3) -> (data, False); [D, H, W] with every axis -> (data[None], True)."""
    axis = tuple(int(a) % data.dim() for a in axis)
    if data.dim() == 4 and axis == (1, 2, 3):
        return data, False
    if data.dim() == 3 and axis == (0, 1, 2):
        return data[None], True
    raise NotImplementedError(f"{what}: [C, D, H, W] with axis=(1, 2, 3) or [D, H, W] with every axis, not {tuple(data.shape)} with {axis}")


def zero_one_window(data, axis=(1, 2, 3), ceiling_percentile=99, floor_percentile=1, floor=0, ceiling=1, channels_axis=None,
                    _backend=None):
    """Per channel: the floor threshold is the floor_percentile of all values, the ceiling threshold the ceiling_percentile of the values
    strictly above the floor threshold (the foreground), and the result window_data between the two. The first percentile call's output
    is the second one's `above`: the thresholds never leave the device.
    A constant channel has no value above its floor threshold: no foreground, a NaN ceiling threshold and a NaN channel -- what the
    formula gives (numpy's percentile of an empty array is NaN too)."""
    if channels_axis not in (None, 0):
        raise NotImplementedError("channels_axis other than 0")
    x4, squeeze = _channel_first(data, axis, "zero_one_window")
    be = _be(data, _backend)
    x = _volume(x4)
    lo = be.percentiles(x, [floor_percentile])[0].reshape(-1)
    hi = be.percentiles(x, [ceiling_percentile], above=lo)[0].reshape(-1)
    y = be.window(x, lo, hi, _lib.WINDOW_RESCALE, floor, ceiling)
    return y[0] if squeeze else y


def zero_floor_normalize_image_data(data, axis=(1, 2, 3), floor_percentile=1, floor=0, _backend=None):
    """Per channel: values at or below the floor_percentile become `floor`, the others are moved down by it, and the result is divided
    by its standard deviation (ddof 1, as torch.std; the mean is not removed)."""
    x4, squeeze = _channel_first(data, axis, "zero_floor_normalize_image_data")
    be = _be(data, _backend)
    x = _volume(x4)
    thr = be.percentiles(x, [floor_percentile])[0].reshape(-1)
    shifted = be.window(x, thr, None, _lib.WINDOW_SHIFT_FLOOR, floor)
    y = be.zscore_select(shifted, _lib.SELECT_ALL, center=False, ddof=1, zero_std_to_one=False)[0]
    return y[0] if squeeze else y


def foreground_zero_mean_normalize_image_data(data, channel_dim=0, background_value=0, tolerance=1e-5, _backend=None):
    """Per channel (along dim 0): the voxels with |x| > background_value + tolerance are the foreground; they become
    (x - mean) / std of the foreground (ddof 1, as torch.std), the others stay as they are, bit for bit.
    The reference's multi-channel branch indexes the LAST axis by the channel number of channel_dim, which is not what its comment
    intends; this is the per-channel intent. Only the single-channel branch is pinned to the reference (tests/golden)."""
    if channel_dim != 0:
        raise NotImplementedError("channel_dim other than 0")
    be = _be(data, _backend)
    x = _volume(data if data.dim() > 3 else data[None])
    y = be.zscore_select(x, _lib.SELECT_ABS_ABOVE, background_value + tolerance, center=True, ddof=1, zero_std_to_one=False)[0]
    return y if data.dim() > 3 else y[0]
