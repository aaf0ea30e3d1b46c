"""Cases and the exact oracle of the connected-component tests (tests/test_components.py on the emulator, test_components_gpu.py on
the HIP library).

Oracle: scipy.ndimage.label with generate_binary_structure(3, 1 | 3) when scipy imports, otherwise `torch_labels` below (labels =
linear index + 1 on the mask, repeated masked minimum over the 6 / 26 neighbours until nothing changes); a CPU test pins the
second to the first. Every oracle component is renamed to 1 + its smallest linear index, the canonical form the library writes, and
the comparison is torch.equal: labels, counts, sizes and masks have exact answers.
"""
import itertools

import numpy as np
import torch

try:
    import scipy.ndimage as _ndi
except Exception:                       # noqa: BLE001 -- scipy is optional: the torch reference below takes over
    _ndi = None

TILE = (4, 4, 64)                        # (z, y, x) tile of cc_local_kernel: what the constructed cases are built around
CONN = {1: 6, 3: 26}                     # generate_binary_structure(3, k) -> number of neighbours


def have_scipy():
    return _ndi is not None


def _offsets(k):
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0) and (k == 3 or sum(abs(v) for v in o) == 1)]


def torch_labels(mask, k):
    """mask [D, H, W] -> canonical int32 labels, by propagating the minimum index to a fixed point (plain torch)."""
    d, h, w = mask.shape
    big = d * h * w + 1
    fg = mask != 0
    lab = torch.where(fg, torch.arange(1, d * h * w + 1, dtype=torch.int64).reshape(d, h, w), torch.tensor(big))
    offs = _offsets(k)
    while True:
        p = torch.nn.functional.pad(lab, (1, 1, 1, 1, 1, 1), value=big)
        new = lab
        for dz, dy, dx in offs:
            new = torch.minimum(new, p[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        new = torch.where(fg, new, torch.tensor(big))
        if torch.equal(new, lab):
            break
        lab = new
    return torch.where(fg, lab, torch.tensor(0)).to(torch.int32)


def scipy_labels(mask, k):
    """mask [D, H, W] -> canonical int32 labels from scipy.ndimage.label."""
    m = mask.numpy() != 0
    lab, n = _ndi.label(m, structure=_ndi.generate_binary_structure(3, k))
    flat = lab.ravel()
    fg = np.flatnonzero(flat)
    first = np.zeros(n + 1, dtype=np.int64)
    first[flat[fg][::-1]] = fg[::-1] + 1                       # repeated indices: the last assignment wins = the smallest voxel index
    first[0] = 0
    return torch.from_numpy(first[flat].reshape(lab.shape).astype(np.int32))


def oracle_labels(mask4, k):
    """mask [C, D, H, W] uint8 (host) -> (canonical int32 labels [C, D, H, W], int64 component counts [C])."""
    fn = scipy_labels if have_scipy() else torch_labels
    labels = torch.stack([fn(mask4[c], k) for c in range(mask4.shape[0])])
    v = mask4[0].numel()
    count = (labels.reshape(mask4.shape[0], v) == torch.arange(1, v + 1, dtype=torch.int32)).sum(dim=1)
    return labels, count


def oracle_filter(mask4, labels, keep_largest, min_size):
    """-> (uint8 out [C, D, H, W], int32 stats [C, 3]: components, largest size, largest label); ties -> the smaller label
    (np.bincount(labels)[1:].argmax())."""
    out = torch.zeros_like(mask4)
    stats = torch.zeros(mask4.shape[0], 3, dtype=torch.int32)
    for c in range(mask4.shape[0]):
        l = labels[c].numpy().ravel()
        sizes = np.bincount(l, minlength=2)
        sizes[0] = 0
        n = int((sizes > 0).sum())
        win = int(sizes[1:].argmax()) + 1 if n else 0
        keep = (l > 0) & (sizes[l] >= max(int(min_size), 0))
        if keep_largest:
            keep &= l == win
        out[c] = torch.from_numpy(keep.astype(np.uint8).reshape(labels[c].shape))
        stats[c] = torch.tensor([n, int(sizes[win]) if n else 0, win], dtype=torch.int32)
    return out, stats


# ---- cases ------------------------------------------------------------------------------------------------------------------------
DENSITIES = (0.05, 0.10, 0.2, 0.31, 0.5, 0.9)                  # around the site-percolation thresholds (6: 0.3116, 26: 0.097)
EXTENTS = ((19, 13, 70), (1, 9, 130), (33, 1, 1), (5, 5, 5))


def random_mask(c, dhw, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(c, *dhw, generator=g) < p).to(torch.uint8)


def serpentine():
    """A one-voxel-wide path through every tile of a 3 x 3 x 3-tile volume (12 x 12 x 192): in every other (z, y) row the whole x-row,
    joined alternately at its two ends, the planes joined alternately too -- the longest chains, every tile face crossed many times."""
    tz, ty, tx = TILE
    d, h, w = 3 * tz, 3 * ty, 3 * tx
    m = torch.zeros(1, d, h, w, dtype=torch.uint8)
    end = 0
    for z in range(0, d, 2):
        ys = list(range(0, h, 2))
        if (z // 2) % 2:
            ys = ys[::-1]
        for i, y in enumerate(ys):
            m[0, z, y, :] = 1
            if i + 1 < len(ys):                                # connector to the next row of this plane, at alternating ends
                end = (w - 1) if end == 0 else 0
                m[0, z, min(y, ys[i + 1]) + 1, end] = 1
        if z + 2 < d:                                          # connector to the next plane, at the end the last row finished on ...
            end = (w - 1) if end == 0 else 0
            m[0, z + 1, ys[-1], end] = 1
    return m


def _blank(c=1, tiles=(2, 2, 2)):
    return torch.zeros(c, tiles[0] * TILE[0], tiles[1] * TILE[1], tiles[2] * TILE[2], dtype=torch.uint8)


def constructed_cases():
    """name -> uint8 mask [C, D, H, W]."""
    tz, ty, tx = TILE
    cases = {}
    cases["empty"] = torch.zeros(2, 5, 6, 70, dtype=torch.uint8)
    cases["full"] = torch.ones(1, 9, 7, 131, dtype=torch.uint8)
    m = torch.zeros(1, 6, 6, 66, dtype=torch.uint8); m[0, 5, 4, 65] = 1
    cases["single_voxel"] = m
    cases["serpentine"] = serpentine()
    m = _blank(); m[0, 1, 1, 3:8] = 1; m[0, 6, 6, 100:105] = 1; m[0, 3, 2, 70] = 1
    cases["equal_sizes"] = m                                   # two components of 5 voxels: the tie goes to the first
    m = _blank(); m[0, 5, 5, 90:95] = 1; m[0, 0, 1, 3:8] = 1; m[0, 3, 2, 70:72] = 1
    cases["equal_sizes_late_first"] = m
    for ax, name in enumerate(("z", "y", "x")):                # two voxels that touch only across a tile face, per axis
        m = _blank()
        a = [1, 1, 5]; a[ax] = TILE[ax] - 1
        b = list(a); b[ax] += 1
        m[0, a[0], a[1], a[2]] = 1; m[0, b[0], b[1], b[2]] = 1
        cases[f"face_{name}"] = m
    for ax in range(3):                                        # ... only across a tile EDGE (separate under 6, one under 26)
        for sign in (1, -1):
            m = _blank()
            a = [tz - 1, ty - 1, tx - 1]
            b = [tz, ty, tx]
            b[ax] = a[ax] = 2                                  # the axis the edge runs along: same coordinate
            if sign < 0:
                o = [i for i in range(3) if i != ax][0]
                a[o], b[o] = b[o], a[o]
            m[0, a[0], a[1], a[2]] = 1; m[0, b[0], b[1], b[2]] = 1
            cases[f"edge_{'zyx'[ax]}{'+' if sign > 0 else '-'}"] = m
    for sz, sy, sx in itertools.product((0, 1), repeat=3):     # ... only across a tile CORNER, every diagonal
        m = _blank()
        a = [tz - 1 + sz, ty - 1 + sy, tx - 1 + sx]
        b = [tz - sz, ty - sy, tx - sx]
        m[0, a[0], a[1], a[2]] = 1; m[0, b[0], b[1], b[2]] = 1
        cases[f"corner_{sz}{sy}{sx}"] = m
    return cases


def probabilities(m, c, dhw, seed, threshold=0.5, margin=1e-6):
    """[M, C, D, H, W] fp32 in [0, 1] whose float64 mean is nowhere within `margin` of the threshold (redrawn where it is; the tests
    assert the property themselves)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(m, c, *dhw, generator=g)
    near = (p.double().mean(dim=0) - threshold).abs() <= 4 * margin
    p[:, near] = 0.25
    return p


def noisy_ellipsoids(c, dhw, flip=0.02, seed=0):
    """The nested ellipsoid targets of synthetic.synthetic_case with salt-and-pepper flips: thousands of islands, one dominant component."""
    import importlib
    syn = importlib.import_module("3dunetcnn_amd.synthetic")
    g = torch.Generator().manual_seed(seed + 1)
    d, h, w = dhw
    m = syn.synthetic_case(1, 1, dhw, c, seed)[1][0]
    flips = torch.rand(c, d, h, w, generator=g) < flip
    return m ^ flips.to(torch.uint8)


# ---- the checks both test files run, on whichever backend ----------------------------------------------------------------------------
def check_labels(be, mask, k, prepost):
    dev = be.device
    labels, count = prepost.connected_components(mask.to(dev), connectivity=k, _backend=be)
    ref, ref_count = oracle_labels(mask, k)
    assert labels.dtype == torch.int32 and count.dtype == torch.int64
    assert torch.equal(labels.cpu(), ref), f"labels differ at {int((labels.cpu() != ref).sum())} voxels"
    assert torch.equal(count.cpu(), ref_count)
    return labels, ref


def check_filter(be, mask, k, keep_largest, min_size, ref_labels=None, labels=None):
    dev = be.device
    md = mask.to(dev)
    if labels is None:
        labels = be.cc_label(md, CONN[k])
    if ref_labels is None:
        ref_labels, _ = oracle_labels(mask, k)
    out, stats = be.cc_filter(md, labels, keep_largest, min_size)
    ref_out, ref_stats = oracle_filter(mask, ref_labels, keep_largest, min_size)
    assert torch.equal(stats.cpu(), ref_stats), (stats.cpu().tolist(), ref_stats.tolist())
    assert torch.equal(out.cpu(), ref_out)
    return out
