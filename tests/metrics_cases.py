"""Cases, oracles and the shared checks of the metric tests (tests/test_metrics.py on the emulator, tests/test_metrics_gpu.py on the HIP
library): overlap counts, mask edges, the exact Euclidean distance transform and the surface-distance statistics of csrc/metrics.hip.

Oracles, in int64 / float64, independent of the kernels' separable structure where the size allows:
  brute_dist2      all pairs (voxel, site): min over sites of sum_axis (spacing * difference)^2. Unit spacing: int64, exact.
  separable_dist2  the three passes with the per-axis min_j written as a broadcast; for volumes whose all-pairs table is too large.
  torch_edges      mask & ~(all six face neighbours, zero padded).
  surface_oracle   numpy on the oracle distances: np.max, np.mean over both directions, np.percentile (default linear rule).
A CPU test pins the first two to each other and, when scipy imports, both to scipy.ndimage.distance_transform_edt and the edges to
mask ^ binary_erosion(mask).

Tolerances. Counts, edges and unit-spacing dist2: exact. Other spacings: relative 1e-6 -- each of the three terms carries at most two
fp32 roundings, each sum one, < 5 * 2^-24 = 3e-7, and a minimum is no worse than its worst candidate. Surface statistics: relative 1e-6,
the same plus sqrtf within 1 ulp (the mean and the percentile are formed in double from fp32 roots). Ratios of counts: 1 ulp of fp32.
"""
import itertools

import numpy as np
import torch

import components_cases as CK

try:
    import scipy.ndimage as _ndi
except Exception:                       # noqa: BLE001 -- scipy is optional: the oracles below do not need it
    _ndi = None

X_CHUNK, LINE_CHUNK = 64, 128            # edt_x_kernel's sweep width; EDT_CHUNK of csrc/metrics.hip (a test reads it from the source)
LONG_EXTENTS = ((2 * LINE_CHUNK + 3, 5, 6), (6, 2 * LINE_CHUNK + 5, 5), (5, 6, 2 * LINE_CHUNK + 7))      # one axis streams in three chunks
EXTENTS = tuple(CK.EXTENTS) + LONG_EXTENTS
DENSITIES = (0.02, 0.3, 0.9)
CHANNELS = (1, 3)
SPACINGS = tuple(dict.fromkeys(((1, 1, 1), (1, 1, 1), (2, 0.5, 1.25), (1, 1, 3))))      # (z, y, x)
PERCENTILES = (0, 50, 95, 100)
REL = 1e-6
BRUTE_PAIRS = 40_000_000                 # all-pairs oracle while voxels * sites stays below this
BRUTE_VOXELS = 25_000


def have_scipy():
    return _ndi is not None


def ids(e):
    return "x".join(str(v) for v in e)


# ---- oracles ------------------------------------------------------------------------------------------------------------------------
def brute_dist2(sites, spacing=(1, 1, 1)):
    """sites [D, H, W] bool -> squared distance to the nearest True voxel: int64 for unit spacing, else float64; no site: -1 / inf."""
    d, h, w = sites.shape
    unit = tuple(spacing) == (1, 1, 1)
    grid = torch.stack(torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij"), dim=-1).reshape(-1, 3)
    s = grid[sites.reshape(-1)]
    if s.shape[0] == 0:
        return torch.full((d, h, w), -1, dtype=torch.int64) if unit else torch.full((d, h, w), float("inf"), dtype=torch.float64)
    out = []
    step = max(1, 4_000_000 // s.shape[0])
    for a in range(0, grid.shape[0], step):
        v = grid[a:a + step]
        acc = None
        for ax in range(3):
            diff = v[:, ax, None] - s[None, :, ax]
            term = diff * diff if unit else (diff.double() * float(spacing[ax])) ** 2
            acc = term if acc is None else acc + term
        out.append(acc.min(dim=1).values)
    return torch.cat(out).reshape(d, h, w)


def separable_dist2(sites, spacing=(1, 1, 1)):
    """The same by three passes in float64 (integers stay exact far beyond these extents); no site: inf. Always float64."""
    d, h, w = sites.shape
    inf = torch.tensor(float("inf"), dtype=torch.float64)

    def sq(n, sp):
        i = torch.arange(n, dtype=torch.float64)
        return ((i[:, None] - i[None, :]) * float(sp)) ** 2                       # [i, j]

    g = torch.where(sites[:, :, None, :], sq(w, spacing[2])[None, None], inf).min(dim=3).values               # [D, H, W(i)]
    g = (g[:, None, :, :] + sq(h, spacing[1])[None, :, :, None]).min(dim=2).values                             # [D, H(i), W]
    out = torch.empty(d, h, w, dtype=torch.float64)
    zz = sq(d, spacing[0])
    for a in range(0, d, 16):                                                     # [D(i) block, D(j), H, W]
        out[a:a + 16] = (g[None] + zz[a:a + 16, :, None, None]).min(dim=1).values
    return out


_DIST2 = {}


def oracle_dist2(mask4, spacing=(1, 1, 1), invert=False, key=None):
    """mask [C, D, H, W] -> float64 [C, D, H, W] squared distance to the nearest nonzero (invert: zero) voxel, inf without one. `key`:
    cache the answer (the cases are deterministic; a reference is computed once and shared)."""
    k = None if key is None else (key, tuple(spacing), bool(invert))
    if k in _DIST2:
        return _DIST2[k]
    out = []
    for c in range(mask4.shape[0]):
        s = (mask4[c] != 0) != bool(invert)
        n = int(s.sum())
        if s.numel() <= BRUTE_VOXELS and s.numel() * max(n, 1) <= BRUTE_PAIRS:
            r = brute_dist2(s, spacing).double()
            r = torch.where(r < 0, torch.tensor(float("inf"), dtype=torch.float64), r)
        else:
            r = separable_dist2(s, spacing)
        out.append(r)
    out = torch.stack(out)
    if k is not None:
        _DIST2[k] = out
    return out


def scipy_dist2(sites, spacing=(1, 1, 1)):
    """distance_transform_edt measures to the nearest ZERO voxel: the sites are inverted. Needs at least one site."""
    return torch.from_numpy(_ndi.distance_transform_edt(~sites.numpy(), sampling=tuple(float(v) for v in spacing))) ** 2


def torch_edges(mask4):
    m = mask4 != 0
    p = torch.nn.functional.pad(m, (1, 1, 1, 1, 1, 1), value=False)
    d, h, w = m.shape[1:]
    inner = m.clone()
    for dz, dy, dx in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
        inner &= p[:, 1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return (m & ~inner).to(torch.uint8)


def scipy_edges(mask3):
    m = mask3.numpy() != 0
    return torch.from_numpy((m ^ _ndi.binary_erosion(m)).astype(np.uint8))


def oracle_counts(pred4, truth4):
    p, t = (pred4 != 0).reshape(pred4.shape[0], -1), (truth4 != 0).reshape(truth4.shape[0], -1)
    return torch.stack([(p & t).sum(1), (p & ~t).sum(1), (~p & t).sum(1), (~p & ~t).sum(1)], dim=1).to(torch.int64)


def oracle_ratios(counts):
    """name -> float32 numpy [C]: the fp32 quotient of the exact counts, with the empty-set values."""
    c = counts.numpy().astype(np.float64)
    tp, fp, fn = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = {"dice": np.where(2 * tp + fp + fn == 0, 1.0, 2 * tp / (2 * tp + fp + fn)),
             "iou": np.where(tp + fp + fn == 0, 1.0, tp / (tp + fp + fn)),
             "sensitivity": tp / (tp + fn), "precision": tp / (tp + fp)}            # 0 / 0 = NaN
    return {k: v.astype(np.float32) for k, v in r.items()}


def surface_oracle(pred4, truth4, spacing, percentile, key=None):
    """-> dict of float64 numpy [C] (hausdorff, hausdorff_percentile, average_surface_distance), directed [C, 5], edge_counts [C, 2]."""
    ea, eb = torch_edges(pred4), torch_edges(truth4)
    to_b = oracle_dist2(eb, spacing, key=None if key is None else (key, "b")).sqrt().numpy()
    to_a = oracle_dist2(ea, spacing, key=None if key is None else (key, "a")).sqrt().numpy()
    c = pred4.shape[0]
    out = {"hausdorff": np.zeros(c), "hausdorff_percentile": np.zeros(c), "average_surface_distance": np.zeros(c),
           "directed": np.zeros((c, 5)), "edge_counts": np.zeros((c, 2), dtype=np.int64)}
    for i in range(c):
        a, b = ea[i].numpy() != 0, eb[i].numpy() != 0
        out["edge_counts"][i] = (a.sum(), b.sum())
        if not a.any() or not b.any():
            v = 0.0 if not a.any() and not b.any() else np.inf
            for k in ("hausdorff", "hausdorff_percentile", "average_surface_distance", "directed"):
                out[k][i] = v
            continue
        dab, dba = to_b[i][a], to_a[i][b]
        out["directed"][i] = (np.max(dab), np.max(dba), np.percentile(dab, percentile), np.percentile(dba, percentile), np.mean(dab))
        out["hausdorff"][i] = max(np.max(dab), np.max(dba))
        out["hausdorff_percentile"][i] = max(np.percentile(dab, percentile), np.percentile(dba, percentile))
        out["average_surface_distance"][i] = np.mean(np.concatenate([dab, dba]))
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def random_mask(c, dhw, p, seed):
    return CK.random_mask(c, dhw, p, seed)


def random_cases(dhw):
    """(key, pred, truth) per extent: C = 3 with one density per channel (0.02, 0.3, 0.9) and C = 1 at 0.3; truth at 0.3 / 0.25."""
    three = torch.cat([random_mask(1, dhw, p, seed=31 + i) for i, p in enumerate(DENSITIES)])
    yield (ids(dhw), 3), three, random_mask(3, dhw, 0.3, seed=77)
    yield (ids(dhw), 1), random_mask(1, dhw, DENSITIES[1], seed=11), random_mask(1, dhw, 0.25, seed=78)


BASE = (9, 10, 70)                       # more than one x chunk, nothing a multiple of a tile


def constructed_cases():
    """name -> uint8 mask [C, D, H, W]."""
    d, h, w = BASE
    z = lambda c=1: torch.zeros(c, d, h, w, dtype=torch.uint8)                   # noqa: E731
    cases = {"empty": z(2), "full": torch.ones(1, d, h, w, dtype=torch.uint8)}
    m = z(); m[0, 4, 3, 65] = 1
    cases["single_voxel"] = m
    for cz, cy, cx in itertools.product((0, 1), repeat=3):
        m = z(); m[0, cz * (d - 1), cy * (h - 1), cx * (w - 1)] = 1
        cases[f"corner_{cz}{cy}{cx}"] = m
    m = z(); m[0, 0] = 1
    cases["face_plane_z"] = m
    m = z(); m[0, :, :, w - 1] = 1
    cases["face_plane_x"] = m
    m = z(); m[0, :, 2] = 1; m[0, :, 7] = 1
    cases["two_planes"] = m
    m = z(); m[0, 0:5, 3:h, 40:w] = 1
    cases["box_at_border"] = m                                  # the border counts as an edge
    m = z(); m[0, 1:8, 1:9, 5:68] = 1; m[0, 3:6, 3:7, 8:65] = 0
    cases["hollow_shell"] = m
    m = random_mask(2, BASE, 0.05, 5); m[0] = 0
    cases["no_sites_beside_sites"] = m
    return cases


def edge_set_pairs():
    """name -> (pred, truth) [1, D, H, W]: pred is n isolated voxels (each is an edge voxel: n = 1, 2, 21, so that the percentile position
    q / 100 * (n - 1) is an integer for some q and fractional for others), truth a box."""
    d, h, w = BASE
    pairs = {}
    for n in (1, 2, 21):
        a = torch.zeros(1, d, h, w, dtype=torch.uint8)
        for i in range(n):
            a[0, (2 * i) % d, (4 * i + 1) % h, 3 * i + 2] = 1
        b = torch.zeros(1, d, h, w, dtype=torch.uint8); b[0, 2:6, 2:8, 20:50] = 1
        assert int(torch_edges(a).sum()) == n
        pairs[f"edges_{n}"] = (a, b)
    return pairs


def blob_pair(c, dhw, seed):
    """Two overlapping smooth random blobs per channel (thresholded box-filtered noise): surfaces, not salt and pepper."""
    g = torch.Generator().manual_seed(seed)

    def smooth(x):
        for _ in range(2):
            x = torch.nn.functional.avg_pool3d(x[None], 5, stride=1, padding=2)[0]
        return x

    a, b = smooth(torch.rand(c, *dhw, generator=g)), smooth(torch.rand(c, *dhw, generator=g))
    pred = a > a.flatten(1).median(dim=1).values[:, None, None, None]
    mix = 0.7 * a + 0.3 * b
    truth = mix > mix.flatten(1).median(dim=1).values[:, None, None, None]
    return pred.to(torch.uint8), truth.to(torch.uint8)


# ---- the checks both test files run, on whichever backend --------------------------------------------------------------------------------
def rel_close(got, ref, what=""):
    """got: fp32 tensor from the library, ref: float64 (tensor or numpy). Infinite and zero references are matched exactly."""
    g = got.detach().cpu().double().reshape(-1)
    r = torch.as_tensor(np.asarray(ref), dtype=torch.float64).reshape(-1)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    special = torch.isinf(r) | (r == 0)
    assert torch.equal(g[special], r[special]), (what, "zero / infinite entries differ")
    err = ((g[~special] - r[~special]).abs() / r[~special].abs())
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: worst relative error {worst:.3e} over {int(err.numel())} values")
    assert worst <= REL, (what, worst)


def check_counts(be, metrics, pred, truth):
    dev = be.device
    counts = metrics.confusion_counts(pred.to(dev), truth.to(dev), _backend=be)
    ref = oracle_counts(pred, truth)
    assert counts.dtype == torch.int32 and torch.equal(counts.cpu().long(), ref), (counts.cpu().tolist(), ref.tolist())
    ratios = oracle_ratios(ref)
    for name, fn in (("dice", metrics.dice_score), ("iou", metrics.iou), ("sensitivity", metrics.sensitivity), ("precision", metrics.precision)):
        got = fn(pred.to(dev), truth.to(dev), _backend=be)
        assert got.dtype == torch.float32 and got.shape == (pred.shape[0],)
        g, r = got.cpu().numpy(), ratios[name]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (name, g, r)
        ok = ~np.isnan(r)
        assert np.all(np.abs(g[ok].astype(np.float64) - r[ok]) <= np.spacing(r[ok])), (name, g, r)
    return counts


def check_edges(be, metrics, mask):
    e = metrics.mask_edges(mask.to(be.device), _backend=be)
    assert e.dtype == torch.uint8 and torch.equal(e.cpu(), torch_edges(mask))
    return e


def check_edt_unit(be, metrics, mask, key=None):
    """Unit spacing: the squared distance equals the integer oracle bit for bit, +inf for a channel without sites included; both
    polarities (distance_to: to the nearest nonzero voxel; distance_transform_edt: scipy's, to the nearest zero voxel)."""
    dev = be.device
    ref = oracle_dist2(mask, (1, 1, 1), False, key).float()
    got = metrics.distance_to(mask.to(dev), squared=True, _backend=be)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), ref), f"{int((got.cpu() != ref).sum())} voxels differ"
    ref_inv = oracle_dist2(mask, (1, 1, 1), True, key)
    got_inv = be.edt(mask.to(dev), (1, 1, 1), invert=True, sqrt=False)
    assert torch.equal(got_inv.cpu(), ref_inv.float())
    rel_close(metrics.distance_transform_edt(mask.to(dev), _backend=be), ref_inv.sqrt(), "distance_transform_edt")
    return got


def check_edt_spacing(be, metrics, mask, spacing, key=None):
    ref = oracle_dist2(mask, spacing, False, key)
    got = metrics.distance_to(mask.to(be.device), sampling=spacing, squared=True, _backend=be)
    rel_close(got, ref, f"dist2 spacing {spacing}")
    return got


def check_shift(be, metrics):
    """A solid box against itself moved by (0, 0, 3), nothing clipped: every edge voxel has its twin three voxels away and the face that
    leads has nothing nearer, so hausdorff == 3 * sx (every term of these spacings is exact in fp32)."""
    box = edge_set_pairs()["edges_1"][1]
    shifted = torch.zeros_like(box); shifted[..., 3:] = box[..., :-3]
    assert int(shifted.sum()) == int(box.sum())
    for sp in SPACINGS:
        s = metrics.surface_distances(box.to(be.device), shifted.to(be.device), spacing=sp, _backend=be)
        assert float(s.hausdorff[0]) == 3 * sp[2], (sp, float(s.hausdorff[0]))


def check_surface(be, metrics, pred, truth, spacing, percentiles, key=None):
    """Edges and distance fields once, the statistics op once per percentile against numpy on the oracle distances; the public
    surface_distances (one call, the last percentile) must give the bits of its parts. Returns that call's result."""
    dev = be.device
    percentiles = tuple(percentiles) if isinstance(percentiles, (tuple, list)) else (percentiles,)
    p, t = pred.to(dev), truth.to(dev)
    ea, eb = be.mask_edges(p), be.mask_edges(t)
    to_b, to_a = be.edt(eb, spacing, sqrt=False), be.edt(ea, spacing, sqrt=False)
    for q in percentiles:
        out, n = be.surface_stats(ea, eb, to_b, to_a, q)
        ref = surface_oracle(pred, truth, spacing, q, key)
        assert n.dtype == torch.int32 and np.array_equal(n.cpu().numpy(), ref["edge_counts"])
        for name, got in (("hausdorff", out[:, 0]), ("hausdorff_percentile", out[:, 1]), ("average_surface_distance", out[:, 2]),
                          ("directed", out[:, 3:8])):
            rel_close(got, ref[name], f"{name} q={q} spacing={spacing}")
    s = metrics.surface_distances(p, t, spacing=spacing, percentile=percentiles[-1], _backend=be)
    assert torch.equal(s.edge_counts, n)
    for name, got in (("hausdorff", out[:, 0]), ("hausdorff_percentile", out[:, 1]), ("average_surface_distance", out[:, 2]),
                      ("directed", out[:, 3:8])):
        a, b = getattr(s, name), got
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()), name
    return s
