"""TEST INFRASTRUCTURE: the bit-exact pin of the volume ops (csrc/prepost.hip, augment.hip, components.hip, metrics.hip, intensity.hip).

Every group below builds small inputs from seeded CPU generators, moves them to the backend's device, runs the entry points of one op
family through `Backend` and returns {case name: sha256 over dtype, shape and raw bytes of every output}. tests/test_volume_bits.py (the
emulator) and tests/test_volume_bits_gpu.py (the HIP library) compare the digests with tests/golden/volume_bits.json, which
tests/golden/make_volume_bits.py wrote from the commit BEFORE the ops were moved onto csrc/volume_common.h. A digest that moves is a
change of behaviour in a shared helper (most likely a product-sum that contracts differently), never a number to record again.

The shapes are the smallest that reach the edges of the shared pieces: extents that are no multiple of a brick or a tile, two bricks in
x and in z, a short last channel group, several 1024-voxel trips and several workgroups per channel, an emptied channel and a channel
with one edge voxel, ranks that clamp and ranks that straddle runs of equal values.
"""
import hashlib
import os

import torch

import augment_cases as A
import components_cases as CK
import metrics_cases as M
import normalize_cases as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume_bits.json")
GROUPS = ("resample_affine", "zscore", "augment_batch", "metrics", "percentiles", "zscore_select", "window_threshold", "components",
          "ensemble_threshold")
V_SMALL, V_LARGE = 4099, 70001


def digest(*outs):
    h = hashlib.sha256()
    for t in outs:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().cpu().contiguous()
        h.update(str(t.dtype).encode() + str(tuple(t.shape)).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _resize(src, dst):
    """4x4 float64: output voxel of extent dst -> source voxel of extent src, corners on corners."""
    m = A.eye()
    for a in range(3):
        m[a, a] = (src[a] - 1) / (dst[a] - 1)
    return m


def resample_affine(be):
    src, dst = (7, 6, 9), (9, 5, 11)
    x = torch.randn(2, *src, generator=torch.Generator().manual_seed(101))
    m = (A.rot_map(A.ROTATIONS[0], src) @ A.zoom_map(0.8713, src) @ _resize(src, dst))[:3].float().reshape(-1).tolist()
    return {f"resample_affine {mode} {pad}": digest(be.resample_affine(x.to(be.device), dst, m, mode, pad))
            for mode in ("trilinear", "nearest", "nearest_floor") for pad in ("border", "zeros")}


def zscore(be):
    x = torch.randn(3, 1, 1, V_SMALL, generator=torch.Generator().manual_seed(102)) * torch.tensor([1.0, 40.0, 1.0]).view(3, 1, 1, 1)
    x = x + torch.tensor([1000.0, -3.0, 0.0]).view(3, 1, 1, 1)
    x[2] = 7.0
    return {"zscore": digest(be.zscore(x.contiguous().to(be.device)))}


def augment_batch(be):
    n, ci, cl, src = 2, 5, 2, (15, 13, 10)
    g = torch.linspace(0.9, 1.1, n * ci).view(n, ci)
    o = torch.linspace(-0.1, 0.1, n * ci).view(n, ci)
    out = {}
    for dtype, tag in ((torch.uint8, "u8"), (torch.float32, "f32")):
        img, lab = A.make_batch(n, ci, cl, src, dtype, seed=103)
        for dst in (src, (17, 5, 70)):
            maps = A.as_m([A.rot_map(A.ROTATIONS[0], src) @ _resize(src, dst),
                           A.zoom_map(0.8713, src) @ A.rot_map(A.ROTATIONS[1], src) @ _resize(src, dst)])
            for pad in ("border", "zeros"):
                for normalize in (False, True):
                    out[f"augment_batch {tag} {dst} {pad} normalize={normalize}"] = digest(*A.run(be, be.device, img, lab, maps, g, o, dst, pad, normalize))
        flip = A.as_m([A.flip_map(src, [0, 2])] * n)
        out[f"augment_batch {tag} flip copy"] = digest(*A.run(be, be.device, img, lab, flip, None, None, src, "border", False))
        out[f"augment_batch {tag} flip normalize"] = digest(*A.run(be, be.device, img, lab, flip, g, o, src, "zeros", True))
    return out


def metrics(be):
    pred, truth = M.blob_pair(3, M.BASE, seed=104)
    pred = pred.clone()
    pred[1] = 0                                                 # an emptied channel of A
    pred[2] = 0; pred[2, 4, 3, 65] = 1                          # ... and one reduced to a single edge voxel
    p, t = pred.to(be.device), truth.to(be.device)
    ea, eb = be.mask_edges(p), be.mask_edges(t)
    out = {"seg_counts": digest(be.seg_counts(p, t)), "mask_edges": digest(ea, eb)}
    for sp in ((1.0, 1.0, 1.0), (2.0, 0.5, 1.25)):
        to_b, to_a = be.edt(eb, sp, sqrt=False), be.edt(ea, sp, sqrt=False)
        out[f"edt {sp}"] = digest(to_b, to_a, be.edt(t, sp, invert=True, sqrt=False))
        for q in M.PERCENTILES:
            out[f"surface_stats {sp} q={q}"] = digest(*be.surface_stats(ea, eb, to_b, to_a, q))
    return out


def percentiles(be):
    out = {}
    above = torch.tensor([0.0, -1.0, 1.5])
    for v in (V_SMALL, V_LARGE):
        for kind in ("mixed", "zeros60", "one_nan", "duplicates"):
            x = N.values(kind, 3, v).to(be.device)
            for ab in (None, above):
                res = be.percentiles(x, [0, 33.3, 50, 100], None if ab is None else ab.to(be.device), want_ranks=True)
                out[f"percentiles {kind} v={v} above={ab is not None}"] = digest(*res)
    return out


def zscore_select(be):
    x = N.values("zeros60", 3, V_SMALL).to(be.device)
    return {f"zscore_select select={sel} ddof={ddof}": digest(*be.zscore_select(x, sel, 310.0, True, ddof, False))
            for sel in (N.SELECT_ALL, N.SELECT_NONZERO, N.SELECT_ABS_ABOVE) for ddof in (0, 1)}


def window_threshold(be):
    x = N.values("gauss100", 3, V_SMALL).to(be.device)
    lo, hi = torch.tensor([-50.0, 0.0, 20.0]).to(be.device), torch.tensor([50.0, 130.0, 25.0]).to(be.device)
    out = {f"window mode={mode}": digest(be.window(x, lo, None if mode == N.WINDOW_SHIFT_FLOOR else hi, mode, 0.0, 1.0))
           for mode in (N.WINDOW_CLAMP, N.WINDOW_RESCALE, N.WINDOW_SHIFT_FLOOR)}
    out["threshold_any"] = digest(be.threshold_any(x, hi))
    return out


def components(be):
    mask = CK.random_mask(2, CK.EXTENTS[0], 0.31, seed=105).to(be.device)
    out = {}
    for conn in (6, 26):
        labels = be.cc_label(mask, conn)
        out[f"cc_label {conn}"] = digest(labels)
        out[f"cc_filter {conn} largest"] = digest(*be.cc_filter(mask, labels, True, 0))
        out[f"cc_filter {conn} min_size"] = digest(*be.cc_filter(mask, labels, False, 3))
    return out


def ensemble_threshold(be):
    p = torch.rand(3, V_SMALL, generator=torch.Generator().manual_seed(106))
    return {"ensemble_threshold": digest(*be.ensemble_threshold(p.to(be.device), 0.5))}


_DIGESTS = {}


def digests(be, group):
    """{case name: sha256 hex} of one group of GROUPS on backend `be`; computed once per backend and shared."""
    key = (id(be), group)
    if key not in _DIGESTS:
        _DIGESTS[key] = globals()[group](be)
    return _DIGESTS[key]


def check(be, section, group):
    """The digests of `group` on `be` against the committed section ("emu" | "gfx950"), exactly."""
    import json
    want = json.load(open(GOLDEN))[section]
    got = digests(be, group)
    assert got, group
    missing = sorted(set(got) - set(want))
    assert not missing, f"{GOLDEN} [{section}] has no digest for {missing}"
    moved = sorted(k for k in got if got[k] != want[k])
    assert not moved, f"{len(moved)} of {len(got)} outputs of {group} changed bits on {section}: {moved}"


def check_complete(be, section):
    """Every digest of the committed section is still produced by some group: a case dropped from a group does not vanish silently."""
    import json
    want = set(json.load(open(GOLDEN))[section])
    got = [k for group in GROUPS for k in digests(be, group)]
    assert len(got) == len(set(got)), "two groups produce a case of the same name"
    assert set(got) == want, f"no longer produced: {sorted(want - set(got))}; not in the fixture: {sorted(set(got) - want)}"
