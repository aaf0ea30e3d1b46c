"""TEST INFRASTRUCTURE: float64 oracle of mi355_augment_batch and the cases shared by the emulator and the GPU tests.

`oracle` evaluates the three steps of include/mi355_unet3d.h (resample through the voxel map, channel-wise z-score, gain / offset) on the
CPU with plain torch indexing, from the SAME fp32 maps, gains and offsets the kernel gets. tests/test_augment_emu.py checks it once against
F.grid_sample(align_corners=True) on the voxel grid (the form oracle/prepost_ref.py::resample_to_match_ref uses) and against torch.flip /
slicing. It reads nothing outside the repository.

Bounds: images max|got - want| <= TOL * max|want| (TOL = 1e-3, tests/op_cases.py), before and after the statistics; labels equal on every
voxel whose float64 source coordinates are all more than TIE_MARGIN = 1e-3 away from a rounding tie (x.5), and the excluded share of a
case stays <= 2 % (asserted). An fp32 evaluation of a map differs from float64 by ~1e-5 voxels at most, far inside the margin.
"""
import importlib

import torch

from op_cases import TOL

aug = importlib.import_module("3dunetcnn_amd.augment")
TIE_MARGIN = 1e-3
MAX_TIE_SHARE = 0.02
EXTENTS = ((15, 13, 10), (24, 20, 28), (32, 32, 32))
ROTATIONS = ((0.2, -0.13, 0.07), (0.05, 0.2, -0.2))


# -- maps (float64 4x4, output voxel -> source voxel, (z, y, x)) ------------------------------------------------------------------
def eye():
    return torch.eye(4, dtype=torch.float64)


def flip_map(size, axes):
    m = eye()
    for a in axes:
        m[a, a], m[a, 3] = -1.0, float(size[a] - 1)
    return m


def crop_map(start):
    m = eye()
    m[:3, 3] = torch.tensor(start, dtype=torch.float64)
    return m


def about_centre(a, size):
    c = (torch.tensor(size, dtype=torch.float64) - 1.0) / 2.0
    m = eye()
    m[:3, :3] = a
    m[:3, 3] = c - a @ c
    return m


def rot_map(angles, size):
    return about_centre(aug.rotation(*angles), size)


def zoom_map(f, size):
    return about_centre(torch.eye(3, dtype=torch.float64) / f, size)


def as_m(maps):
    """list of 4x4 float64 -> [N, 3, 4] fp32 (what the kernel reads)."""
    return torch.stack([m[:3] for m in maps]).float().contiguous()


# -- oracle --------------------------------------------------------------------------------------------------------------------------
def source_coords(m, out_shape):
    dd, dh, dw = out_shape
    zz, yy, xx = torch.meshgrid(torch.arange(dd, dtype=torch.float64), torch.arange(dh, dtype=torch.float64),
                                torch.arange(dw, dtype=torch.float64), indexing="ij")
    v = torch.stack([zz, yy, xx, torch.ones_like(zz)], dim=-1)
    return v @ m.double().T                                              # [dd, dh, dw, 3]


def _gather(vol, iz, iy, ix):
    """vol [C, D, H, W]; integer index tensors (any, clamped here) -> ([C, ...] values, inside mask)."""
    sd, sh, sw = vol.shape[1:]
    inside = (iz >= 0) & (iy >= 0) & (ix >= 0) & (iz < sd) & (iy < sh) & (ix < sw)
    return vol[:, iz.clamp(0, sd - 1), iy.clamp(0, sh - 1), ix.clamp(0, sw - 1)], inside


def trilinear(vol, coords, padding):
    vol = vol.double()
    c = coords.clone()
    if padding == "border":
        for a in range(3):
            c[..., a] = c[..., a].clamp(0, vol.shape[1 + a] - 1)
    f = torch.floor(c)
    l = c - f
    i0 = f.long()
    out = torch.zeros(vol.shape[0], *coords.shape[:-1], dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            for e in (0, 1):
                w = (l[..., 0] if a else 1 - l[..., 0]) * (l[..., 1] if b else 1 - l[..., 1]) * (l[..., 2] if e else 1 - l[..., 2])
                val, inside = _gather(vol, i0[..., 0] + a, i0[..., 1] + b, i0[..., 2] + e)
                if padding == "zeros":
                    w = w * inside
                out += w * val
    return out


def nearest(vol, coords, padding):
    r = torch.round(coords).long()                                       # torch.round: half to even
    val, inside = _gather(vol, r[..., 0], r[..., 1], r[..., 2])
    if padding == "zeros":
        val = val * inside.to(val.dtype)
    return val


def tie_mask(coords):
    """True where some coordinate is within TIE_MARGIN of x.5: the nearest voxel there depends on the last bits of the coordinate."""
    frac = coords - torch.floor(coords)
    return ((frac - 0.5).abs() <= TIE_MARGIN).any(dim=-1)


def oracle(image, label, m, gain, offset, out_shape, padding, normalize):
    """image [N, C, D, H, W], label None or [N, Cl, D, H, W], m [N, 3, 4] fp32, gain / offset None or [N, C].
    Returns (float64 image', label' in the label's dtype or None, tie mask [N, dd, dh, dw])."""
    imgs, labs, ties = [], [], []
    for s in range(image.shape[0]):
        co = source_coords(m[s], out_shape)
        x = trilinear(image[s], co, padding)
        if normalize:
            mean = x.mean(dim=(1, 2, 3), keepdim=True)
            sd = x.std(dim=(1, 2, 3), keepdim=True, unbiased=False)
            sd = torch.where(sd == 0, torch.ones_like(sd), sd)
            x = (x - mean) / sd
        if gain is not None:
            x = x * gain[s].double().view(-1, 1, 1, 1)
        if offset is not None:
            x = x + offset[s].double().view(-1, 1, 1, 1)
        imgs.append(x)
        ties.append(tie_mask(co))
        if label is not None:
            labs.append(nearest(label[s], co, padding))
    return torch.stack(imgs), (torch.stack(labs) if label is not None else None), torch.stack(ties)


# -- data and checks -----------------------------------------------------------------------------------------------------------------
def make_batch(n, ci, cl, dhw, label_dtype, seed, constant_channel=False):
    """Images with per-channel level and spread (the statistics have something to remove); labels: cl one-hot-like channels (uint8) or
    label values (fp32), None when cl == 0. constant_channel: channel 2 is constant (std 0 -> divisor 1) -- for the transforms that copy
    voxels only: an interpolated constant is constant up to rounding, and dividing by the spread of that rounding is noise in any
    implementation, the oracle's float64 included."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(n, ci, *dhw, generator=g) * (1.0 + 3.0 * torch.arange(ci).view(1, ci, 1, 1, 1)) + 50.0 * torch.arange(ci).view(1, ci, 1, 1, 1)
    if constant_channel and ci >= 3:
        img[:, 2] = 7.0
    if cl == 0:
        return img, None
    if label_dtype == torch.uint8:
        lab = (torch.rand(n, cl, *dhw, generator=g) < 0.4).to(torch.uint8)
    else:
        lab = torch.randint(0, 5, (n, cl, *dhw), generator=g).float()
    return img, lab


def run(be, dev, img, lab, m, gain, offset, out_shape, padding, normalize):
    d = lambda t: None if t is None else t.to(dev).contiguous()
    out, lout = be.augment_batch(d(img), d(lab), d(m), d(gain), d(offset), out_shape, padding, normalize)
    return out.cpu(), (None if lout is None else lout.cpu())


def image_err(got, want):
    return float((got.double() - want).abs().max() / max(float(want.abs().max()), 1e-30))


def check_against_oracle(be, dev, img, lab, m, gain, offset, out_shape, padding, normalize, what=""):
    got, glab = run(be, dev, img, lab, m, gain, offset, out_shape, padding, normalize)
    want, wlab, ties = oracle(img, lab, m, gain, offset, out_shape, padding, normalize)
    assert got.shape == want.shape
    e = image_err(got, want)
    share = float(ties.float().mean())
    print(f"augment case {what} {tuple(img.shape)} -> {tuple(out_shape)} {padding} normalize={normalize}: image err {e:.2e}, tie share {share:.4f}")
    assert e <= TOL, (what, e)
    if lab is not None:
        assert share <= MAX_TIE_SHARE, (what, share)
        keep = ~ties[:, None].expand_as(wlab)
        assert glab.dtype == lab.dtype and torch.equal(glab[keep], wlab[keep]), (what, int((glab[keep] != wlab[keep]).sum()))
    return got, glab


def exact_cases(dhw):
    """(name, float64 map, output extent, torch reference of one [.., D, H, W] tensor) for the transforms that must copy voxels."""
    d, h, w = dhw
    crop, start = (d - 4, h - 3, w - 5), (2, 1, 3)
    sl = lambda t: t[..., start[0]:start[0] + crop[0], start[1]:start[1] + crop[1], start[2]:start[2] + crop[2]]
    return [("identity", eye(), dhw, lambda t: t),
            ("flip0", flip_map(dhw, [0]), dhw, lambda t: torch.flip(t, [-3])),
            ("flip1", flip_map(dhw, [1]), dhw, lambda t: torch.flip(t, [-2])),
            ("flip2", flip_map(dhw, [2]), dhw, lambda t: torch.flip(t, [-1])),
            ("flip01", flip_map(dhw, [0, 1]), dhw, lambda t: torch.flip(t, [-3, -2])),
            ("crop", crop_map(start), crop, sl),
            ("crop+flip", crop_map(start) @ flip_map(crop, [0, 2]), crop, lambda t: torch.flip(sl(t), [-3, -1]))]


def check_exact(be, dev, n, ci, cl, dhw, label_dtype, seed):
    img, lab = make_batch(n, ci, cl, dhw, label_dtype, seed, constant_channel=True)
    for name, m4, out_shape, ref in exact_cases(dhw):
        m = as_m([m4] * n)
        got, glab = run(be, dev, img, lab, m, None, None, out_shape, "border", False)
        assert torch.equal(got, ref(img)), name
        if lab is not None:
            assert glab.dtype == lab.dtype and torch.equal(glab, ref(lab)), name
        # ... and through the statistics, against the oracle
        g = torch.linspace(0.9, 1.1, n * ci).view(n, ci)
        o = torch.linspace(-0.1, 0.1, n * ci).view(n, ci)
        check_against_oracle(be, dev, img, lab, m, g, o, out_shape, "zeros", True, what=name)


def interp_maps(dhw, n):
    """Per case n maps: rotations, zoom in / out and compositions with flips and a crop-like shift."""
    r0, r1 = rot_map(ROTATIONS[0], dhw), rot_map(ROTATIONS[1], dhw)
    pool = [r0, r1, zoom_map(1.1537, dhw), zoom_map(0.8713, dhw) @ r0, flip_map(dhw, [1]) @ r1 @ zoom_map(1.0931, dhw), crop_map((1, 0, 2)) @ r0]
    return [[pool[(k + s) % len(pool)] for s in range(n)] for k in range(len(pool))]


def check_interp(be, dev, n, ci, cl, dhw, label_dtype, seed, maps=None):
    img, lab = make_batch(n, ci, cl, dhw, label_dtype, seed)
    g = torch.linspace(0.9, 1.1, n * ci).view(n, ci)
    o = torch.linspace(-0.1, 0.1, n * ci).view(n, ci)
    for k, ms in enumerate(maps if maps is not None else interp_maps(dhw, n)):
        m = as_m(ms)
        for padding in ("border", "zeros"):
            check_against_oracle(be, dev, img, lab, m, None, None, dhw, padding, False, what=f"maps{k}")
            check_against_oracle(be, dev, img, lab, m, g, o, dhw, padding, False, what=f"maps{k} gain/offset in pass A")
            check_against_oracle(be, dev, img, lab, m, g, o, dhw, padding, True, what=f"maps{k} normalized")


def check_deterministic(be, dev, n, ci, cl, dhw, seed):
    img, lab = make_batch(n, ci, cl, dhw, torch.uint8, seed)
    m = as_m(interp_maps(dhw, n)[3])
    g = torch.linspace(0.9, 1.1, n * ci).view(n, ci)
    a, la = run(be, dev, img, lab, m, g, None, dhw, "border", True)
    b, lb = run(be, dev, img, lab, m, g, None, dhw, "border", True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and (la is None or torch.equal(la, lb))
