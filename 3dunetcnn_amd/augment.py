"""Training augmentation on the device: the `dataset.training` block of a reference config (unet3d/datasets/segmentation.py:75-94)
applied to a whole batch by two kernel launches (csrc/augment.hip, `Backend.augment_batch`).

The reference composes, per sample and on the CPU: [RandSpatialCropD] -> spatial augmentations on image and label together ->
NormalizeIntensityD on the image -> intensity augmentations on the image. `HipAugmenter` takes the same config entries, draws every
random number on the host from one `torch.Generator`, folds a sample's spatial transforms into ONE 3x4 voxel map and its intensity
transforms into one (gain, offset) per channel, and hands the batch to the device:

    aug = HipAugmenter.from_config(config["dataset"])          # or HipAugmenter(spatial_augmentations=[...], ...)
    image, label = aug(image, label)                           # [N, C, D, H, W] device tensors

Conventions (chosen here and pinned to torch, NOT to a MONAI release -- MONAI is not a dependency of this project and its sub-voxel
and angle conventions are not checked):
  * a spatial axis is a dimension of the array: axis 0 / 1 / 2 = D / H / W of [C, D, H, W], which the kernels call z / y / x;
  * every transform is a pull-back about the centre c = (size - 1) / 2 of the volume it acts on: out(v) = in(c + A (v - c));
    RandFlipD: A = diag(+-1) (src = size - 1 - v on a flipped axis); RandZoomD with factor f: A = diag(1 / f) (f > 1 magnifies);
    RandRotateD: A = R0(range_x) @ R1(range_y) @ R2(range_z), Rk = the right-handed rotation about array axis k
    (R0 = [[1, 0, 0], [0, c, -s], [0, s, c]], R1 = [[c, 0, s], [0, 1, 0], [-s, 0, c]], R2 = [[c, -s, 0], [s, c, 0], [0, 0, 1]]);
  * transforms apply in the order the config lists them, the random crop first (as the reference builds its pipeline), so the
    map of a sample is M = M_crop @ M_1 @ ... @ M_K; all transforms keep the size (keep_size=True), only the crop changes it;
  * image: trilinear; label: nearest (round half to even); one padding mode per augmenter ("border" unless a RandRotateD asks "zeros");
  * RandScaleIntensityD: v * (1 + u), u ~ U(-factors, factors) (or U(a, b) for a pair); RandShiftIntensityD: v + u likewise; one
    draw per sample, or per channel with channel_wise=True.
The random streams do not agree with MONAI's.

There is no CPU fallback: construction and `sample_params` are host code, `__call__` needs an MI355X.
"""
import math
from dataclasses import dataclass

import torch

from . import ops as _ops

_SPATIAL = {"RandFlipD": {"spatial_axis", "prob"},
            "RandRotateD": {"range_x", "range_y", "range_z", "prob", "padding_mode", "keep_size"},
            "RandZoomD": {"min_zoom", "max_zoom", "prob", "keep_size"}}
_INTENSITY = {"RandScaleIntensityD": {"factors", "prob", "channel_wise"},
              "RandShiftIntensityD": {"offsets", "prob", "channel_wise"}}


@dataclass
class AugmentParams:
    """What `sample_params` drew: matrices [N, 3, 4] fp32 (output voxel -> source voxel, (z, y, x)), gains / offsets [N, C] fp32,
    the output extent, and whether every gain is 1 and every offset 0."""
    matrices: torch.Tensor
    gains: torch.Tensor
    offsets: torch.Tensor
    out_shape: tuple
    trivial_intensity: bool


def _check_entries(entries, known, what):
    out = []
    for e in entries or []:
        e = dict(e)
        name = e.pop("name", None)
        if name not in known:
            raise NotImplementedError(f"{what} augmentation {name!r} is not implemented on the device (supported: {sorted(known)})")
        for k in e:
            if k not in known[name]:
                raise NotImplementedError(f"{name}: option {k!r} is not implemented")
        if e.get("keep_size", True) is not True:
            raise NotImplementedError(f"{name}: keep_size=False is not implemented (per-sample output shapes)")
        out.append((name, e))
    return out


def _range(v, symmetric=True):
    """A scalar r -> (-r, r) (MONAI's reading of a scalar range); a pair -> (min, max)."""
    if isinstance(v, (list, tuple)):
        if len(v) != 2:
            raise ValueError(f"a range is a scalar or a pair, got {v!r}")
        return (min(float(v[0]), float(v[1])), max(float(v[0]), float(v[1])))
    return (-abs(float(v)), abs(float(v))) if symmetric else (float(v), float(v))


def _about_centre(a, size):
    """4x4 pull-back: v -> c + a (v - c), c = (size - 1) / 2."""
    c = (torch.tensor(size, dtype=torch.float64) - 1.0) / 2.0
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = a
    m[:3, 3] = c - a @ c
    return m


def rotation(ax, ay, az):
    """R0(ax) @ R1(ay) @ R2(az) in array-axis order (float64 3x3): the convention of the module docstring."""
    c, s = math.cos(ax), math.sin(ax)
    r0 = torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=torch.float64)
    c, s = math.cos(ay), math.sin(ay)
    r1 = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    c, s = math.cos(az), math.sin(az)
    r2 = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float64)
    return r0 @ r1 @ r2


class HipAugmenter:
    def __init__(self, spatial_augmentations=None, intensity_augmentations=None, random_crop=None, normalize=False, generator=None):
        self.spatial = _check_entries(spatial_augmentations, _SPATIAL, "spatial")
        self.intensity = _check_entries(intensity_augmentations, _INTENSITY, "intensity")
        self.random_crop = None if random_crop is None else tuple(int(v) for v in random_crop)
        if self.random_crop is not None and len(self.random_crop) != 3:
            raise ValueError(f"random_crop is a 3-D roi, got {random_crop!r}")
        self.normalize = bool(normalize)
        self.generator = generator if generator is not None else torch.Generator()
        self.padding = "border"
        for name, e in self.spatial:
            if name == "RandFlipD":
                ax = e.get("spatial_axis")
                axes = [0, 1, 2] if ax is None else ([int(ax)] if isinstance(ax, int) else [int(a) for a in ax])
                if any(a not in (0, 1, 2) for a in axes):
                    raise ValueError(f"RandFlipD: spatial_axis {ax!r} is not an axis of a 3-D volume")
                e["_axes"] = axes
            elif name == "RandRotateD":
                pm = e.get("padding_mode", "border")
                if pm not in ("border", "zeros"):
                    raise NotImplementedError(f"RandRotateD: padding_mode {pm!r} is not implemented ('border' or 'zeros')")
                if pm == "zeros":
                    self.padding = "zeros"
                e["_ranges"] = [_range(e.get(k, 0.0)) for k in ("range_x", "range_y", "range_z")]
            elif name == "RandZoomD":
                lo, hi = e.get("min_zoom", 0.9), e.get("max_zoom", 1.1)
                lo = [float(v) for v in lo] if isinstance(lo, (list, tuple)) else [float(lo)] * 3
                hi = [float(v) for v in hi] if isinstance(hi, (list, tuple)) else [float(hi)] * 3
                if len(lo) != 3 or len(hi) != 3 or min(lo) <= 0.0:
                    raise ValueError("RandZoomD: min_zoom / max_zoom are positive scalars or 3 values")
                e["_lo"], e["_hi"], e["_per_axis"] = lo, hi, isinstance(e.get("min_zoom"), (list, tuple)) or isinstance(e.get("max_zoom"), (list, tuple))
        if self.padding == "zeros" and any(n == "RandRotateD" and e.get("padding_mode", "border") == "border" for n, e in self.spatial):
            raise NotImplementedError("RandRotateD entries with different padding_mode: one launch has one padding mode")
        for name, e in self.intensity:
            e["_range"] = _range(e.get("factors" if name == "RandScaleIntensityD" else "offsets", 0.0))
        self._be = None               # tests hand the emulator backend in here, as the loss modules allow

    @classmethod
    def from_config(cls, dataset, generator=None):
        """From a reference `dataset` block (examples/*/..._config.json): training.spatial_augmentations,
        training.intensity_augmentations, random_crop (+ desired_shape) and normalization."""
        tr = dataset.get("training") or {}
        crop = None
        if dataset.get("random_crop"):
            if not dataset.get("desired_shape"):
                raise ValueError("random_crop needs desired_shape (the roi of RandSpatialCropD)")
            crop = dataset["desired_shape"]
        norm = dataset.get("normalization", "zero_mean")        # the reference's default (SegmentationDataset.__init__)
        normalize = norm is not None
        if normalize:
            kw = dataset.get("normalization_kwargs") or {}
            if norm not in ("zero_mean", "NormalizeIntensityD") or not kw.get("channel_wise", False) or kw.get("nonzero", False) \
                    or set(kw) - {"channel_wise", "nonzero"}:
                raise NotImplementedError(f"normalization {norm!r} with {kw!r}: only NormalizeIntensityD(channel_wise=True, nonzero=False) "
                                          "is implemented on the device")
        return cls(tr.get("spatial_augmentations"), tr.get("intensity_augmentations"), crop, normalize, generator)

    # -- host side -------------------------------------------------------------------------------------------------
    def _u(self, lo=0.0, hi=1.0):
        return lo + (hi - lo) * float(torch.rand((), generator=self.generator, dtype=torch.float64))

    def sample_params(self, n, src_shape):
        """Draw the parameters of `n` samples. src_shape: (D, H, W), (C, D, H, W) or (N, C, D, H, W); without a channel count the
        gains / offsets come back as [n, 1]. Host code only: no device is touched."""
        src_shape = tuple(int(v) for v in src_shape)
        channels = src_shape[-4] if len(src_shape) >= 4 else 1
        size = src_shape[-3:]
        out = size if self.random_crop is None else tuple(min(r, s) if r > 0 else s for r, s in zip(self.random_crop, size))
        mats = torch.empty(n, 3, 4, dtype=torch.float64)
        gains, offsets = torch.ones(n, channels, dtype=torch.float64), torch.zeros(n, channels, dtype=torch.float64)
        for i in range(n):
            m = torch.eye(4, dtype=torch.float64)
            if self.random_crop is not None:                     # RandSpatialCropD(random_size=False): a uniform integer start per axis
                for a in range(3):
                    m[a, 3] = float(torch.randint(0, size[a] - out[a] + 1, (), generator=self.generator))
            for name, e in self.spatial:
                do = self._u() < float(e.get("prob", 0.1))
                if name == "RandFlipD":
                    if do:
                        d = torch.ones(3, dtype=torch.float64)
                        d[e["_axes"]] = -1.0
                        f = torch.eye(4, dtype=torch.float64)
                        f[:3, :3] = torch.diag(d)
                        for a in e["_axes"]:
                            f[a, 3] = float(out[a] - 1)           # integers: flips stay exact
                        m = m @ f
                elif name == "RandRotateD":
                    ang = [self._u(lo, hi) for lo, hi in e["_ranges"]]
                    if do:
                        m = m @ _about_centre(rotation(*ang), out)
                elif name == "RandZoomD":
                    if e["_per_axis"]:
                        z = [self._u(lo, hi) for lo, hi in zip(e["_lo"], e["_hi"])]
                    else:
                        z = [self._u(e["_lo"][0], e["_hi"][0])] * 3
                    if do:
                        m = m @ _about_centre(torch.diag(1.0 / torch.tensor(z, dtype=torch.float64)), out)
            mats[i] = m[:3]
            for name, e in self.intensity:
                do = self._u() < float(e.get("prob", 0.1))
                k = channels if e.get("channel_wise", False) else 1
                u = torch.tensor([self._u(*e["_range"]) for _ in range(k)], dtype=torch.float64)
                if not do:
                    continue
                if name == "RandScaleIntensityD":
                    gains[i] *= 1.0 + u
                    offsets[i] *= 1.0 + u
                else:
                    offsets[i] += u
        trivial = bool((gains == 1.0).all() and (offsets == 0.0).all())
        return AugmentParams(mats.float(), gains.float(), offsets.float(), tuple(out), trivial)

    # -- device side -----------------------------------------------------------------------------------------------
    def __call__(self, image, label=None, params=None, normalize=None, _backend=None):
        """image [N, C, D, H, W] fp32, label None or [N, Cl, D, H, W] uint8 / fp32, both on the device. Returns (image', label').
        params: an `AugmentParams` to apply instead of drawing one; normalize: overrides the augmenter's own setting."""
        be = _backend if _backend is not None else self._be
        if be is None:
            if image.device.type != "cuda":
                raise RuntimeError("3dunetcnn_amd.augment runs on an MI355X only (no CPU fallback)")
            be = _ops.default_backend(image.device)
        if image.dim() != 5:
            raise ValueError(f"image must be [N, C, D, H, W], got {tuple(image.shape)}")
        p = params if params is not None else self.sample_params(image.shape[0], image.shape[1:])
        n, c = image.shape[:2]
        gains, offsets = p.gains.expand(n, c), p.offsets.expand(n, c)
        # one small host buffer, one copy: [n][12] maps, then [n][c] gains and offsets
        host = torch.cat([p.matrices.reshape(-1), gains.reshape(-1), offsets.reshape(-1)]).contiguous()
        if image.device.type == "cuda":
            host = host.pin_memory()
        dev = host.to(image.device, non_blocking=True)
        m, g, o = dev[:12 * n], dev[12 * n:12 * n + n * c], dev[12 * n + n * c:]
        if p.trivial_intensity:
            g = o = None
        if label is not None and label.dtype not in (torch.uint8, torch.float32):
            label = label.float()
        return be.augment_batch(image.float().contiguous(), None if label is None else label.contiguous(), m, g, o, p.out_shape, self.padding,
                                self.normalize if normalize is None else bool(normalize))
