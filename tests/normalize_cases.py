"""Cases, oracles and the shared checks of the intensity-normalisation tests (tests/test_normalize.py on the emulator,
tests/test_normalize_gpu.py on the HIP library): the percentile select, the windows, the z-score over a selected set and the any-channel
threshold of csrc/intensity.hip, and the functions of 3dunetcnn_amd/normalize.py composed from them.

Oracles, float64 numpy written from the formulas (nothing of the kernels' pass structure):
  oracle_percentiles   sort the participating values; position p = q / 100 * (n - 1) in double; lo, hi = the order statistics of rank
                       floor(p), min(floor(p) + 1, n - 1); lo if lo == hi else lo + (p - floor(p)) * (hi - lo). n == 0 or a NaN: NaN.
  oracle_zscore        mask on the fp32 values, mean and std (ddof) in float64, (x - mean) / std in float64.
  torch_window         the three window expressions in torch fp32 on the CPU.
A CPU test pins oracle_percentiles to np.percentile on float64 copies and the composed restatements to the committed reference fixture
(tests/golden/normalize_reference.pt, written by tests/golden/make_normalize_reference.py from the reference's own functions).

Bounds, all derived:
  n, ranks             exact: the uint32 views are compared; two zeros compare equal whatever their signs (-0 and +0 are equal values
                       and either may come back).
  percentile value     |got - oracle64| <= 2^-23 * max(|lo|, |hi|): the kernel evaluates the same double expression and rounds once to
                       fp32 (half an ulp, 2^-24 relative, of a value no larger than max(|lo|, |hi|)); the oracle's own double roundings
                       are 2^-29 of that. Below the normal range half an ulp is 2^-150 absolute, which the bound is floored at.
                       lo == hi: exact. The formula's own NaN (lo = -inf beside a finite hi) is compared as NaN.
  windows              bit-identical to the torch fp32 expression fed the thresholds the op produced (every step is one IEEE fp32
                       operation on both sides); NaN positions identical; zeros by value.
  threshold_any        exact.
  zscore_select        voxels not selected: the same bits. Selected: |y - oracle64| <= 2^-22 * (|x| + |mean|) / std.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normalize_reference.pt")
CHANNELS = (1, 3)
SMALL_SIZES = (1, 2, 3, 255, 256, 257, 4099)      # rank clamping and lo == hi; either side of a 256-thread sweep; several 1024-voxel trips
LARGE_SIZE = 70001                                 # several workgroups per channel (odd: the second channel's base is not 16-byte aligned)
MANY_WG_SHAPE = (3, 48, 56, 70)                    # GPU only: every launch has many workgroups, atomics arrive from all XCDs
PERCENTILES = (0, 0.1, 1, 5, 33.3, 50, 90, 0.9 * 100, 99, 99.9, 100)
Q_SETS = (PERCENTILES[0:4], PERCENTILES[4:8], PERCENTILES[8:11] + (50,), (50,), (0.9 * 100,))      # nq = 4, 4, 4, 1, 1
VALUE_SETS = ("gauss100", "offset1000", "tiny_minus5", "all_equal", "low_byte", "mixed", "zeros60", "one_nan", "duplicates")
NAN = float("nan")
WINDOW_CLAMP, WINDOW_RESCALE, WINDOW_SHIFT_FLOOR = 0, 1, 2
SELECT_ALL, SELECT_NONZERO, SELECT_ABS_ABOVE = 0, 1, 2


def values(kind, c, v, seed=0):
    """fp32 [c, v] of one of VALUE_SETS."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * c + v)
    r = torch.randn(c, v, generator=g)
    if kind == "gauss100":
        x = r * 100
    elif kind == "offset1000":                         # the mean far larger than the spread
        x = 1000 + r
    elif kind == "tiny_minus5":
        x = 1e-3 * r - 5
    elif kind == "all_equal":                          # one bin is hit in every pass
        x = torch.tensor([3.25, -7.5, 0.0])[:c, None].expand(c, v).clone()
    elif kind == "low_byte":                           # the keys differ in the lowest byte only: the last pass decides
        bits = 0x42280000 + torch.randint(0, 256, (c, v), generator=g, dtype=torch.int32)
        x = bits.view(torch.float32)
        x[c - 1] = -x[c - 1]
    elif kind == "mixed":                              # negatives, positives, both zeros, denormals, both infinities
        pool = torch.tensor([-np.inf, -np.inf, -3e38, -1.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 2.5, 7e37, np.inf, np.inf], dtype=torch.float32)
        x = pool[torch.randint(0, pool.numel(), (c, v), generator=g)]
        x = torch.where(torch.rand(c, v, generator=g) < 0.3, r, x)
    elif kind == "zeros60":                            # skull-stripped MR: 60 % exact zeros, a Gaussian foreground
        x = torch.where(torch.rand(c, v, generator=g) < 0.6, torch.zeros(()), r * 50 + 300)
    elif kind == "one_nan":
        x = r * 100
        x[0, v // 2] = NAN
    elif kind == "duplicates":                         # a handful of distinct values: runs of equal ones straddle every rank
        x = torch.randint(-2, 3, (c, v), generator=g).float() * 1.5
    else:
        raise KeyError(kind)
    return x.float().contiguous()


# ---- oracles ---------------------------------------------------------------------------------------------------------------------------
def oracle_percentiles(x, qs, above=None):
    """x fp32 [C, V] (tensor), qs in [0, 100], above None or fp32 [C] -> dict of numpy: value float64 [C, nq], lo / hi float32 [C, nq],
    n int64 [C], exact bool [C, nq] (lo == hi)."""
    a = x.reshape(x.shape[0], -1).numpy()
    c, nq = a.shape[0], len(qs)
    out = {"value": np.full((c, nq), np.nan), "lo": np.full((c, nq), np.nan, np.float32), "hi": np.full((c, nq), np.nan, np.float32),
           "n": np.zeros(c, np.int64)}
    for ch in range(c):
        v = a[ch]
        if above is not None:
            with np.errstate(invalid="ignore"):
                v = v[v > np.float32(above[ch])]
        n = out["n"][ch] = v.size
        if n == 0 or np.isnan(v).any():
            continue
        s = np.sort(v)
        for j, q in enumerate(qs):
            p = float(q) / 100 * (n - 1)
            f = int(np.floor(p))
            lo, hi = s[f], s[min(f + 1, n - 1)]
            out["lo"][ch, j], out["hi"][ch, j] = lo, hi
            with np.errstate(invalid="ignore"):
                out["value"][ch, j] = float(lo) if lo == hi else float(lo) + (p - f) * (float(hi) - float(lo))
    return out


def oracle_zscore(x, select, threshold, center, ddof, zero_std_to_one):
    """-> (y float64 [C, V], selected bool [C, V], mean [C], std [C], n [C])."""
    a = x.reshape(x.shape[0], -1).numpy()
    with np.errstate(invalid="ignore"):
        sel = {SELECT_ALL: np.ones_like(a, bool), SELECT_NONZERO: a != 0, SELECT_ABS_ABOVE: np.abs(a) > np.float32(threshold)}[select]
    a64 = a.astype(np.float64)
    y, mean, std = a64.copy(), np.zeros(a.shape[0]), np.zeros(a.shape[0])
    with np.errstate(all="ignore"):
        for ch in range(a.shape[0]):
            v = a64[ch][sel[ch]]
            m = v.mean() if v.size else np.nan
            sd = np.sqrt(((v - m) ** 2).sum() / (v.size - ddof)) if v.size - ddof > 0 else np.nan
            if zero_std_to_one and sd == 0:
                sd = 1.0
            mean[ch], std[ch] = (m if center else 0.0), sd
            y[ch][sel[ch]] = (v - mean[ch]) / sd
    return y, sel, mean, std, sel.sum(axis=1)


def torch_window(x, lo, hi, mode, floor=0.0, ceiling=1.0, channels=None):
    """The window expressions in torch fp32 on the CPU. x [C or 1, V], lo / hi fp32 [channels]."""
    c = x.shape[0] if channels is None else channels
    x = x.reshape(x.shape[0], -1).expand(c, -1)
    lo = lo.reshape(c, 1)
    if mode == WINDOW_CLAMP:
        return torch.clamp(x, lo, hi.reshape(c, 1))
    if mode == WINDOW_RESCALE:                          # the reference's window_data, literally
        t = (x - lo) / (hi.reshape(c, 1) - lo)
        t[t < floor] = floor
        t[t > ceiling] = ceiling
        return t
    background = x <= lo                               # the first half of the reference's zero_floor_normalize_image_data
    t = x - lo
    t[background] = floor
    return t


# ---- comparisons -----------------------------------------------------------------------------------------------------------------------
def same_bits(got, ref, what=""):
    """fp32 tensors: NaN in the same places; elsewhere the same bits, two zeros comparing equal whatever their signs."""
    g, r = got.detach().cpu().float().reshape(-1), ref.detach().cpu().float().reshape(-1)
    assert g.shape == r.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, "NaN positions differ", int((torch.isnan(g) != torch.isnan(r)).sum()))
    ok = ~torch.isnan(r)
    gb, rb = g[ok].view(torch.int32), r[ok].view(torch.int32)
    bad = (gb != rb) & ~((g[ok] == 0) & (r[ok] == 0))
    assert not bool(bad.any()), (what, f"{int(bad.sum())} of {int(ok.sum())} values differ", g[ok][bad][:4].tolist(), r[ok][bad][:4].tolist())


def check_percentile_values(out, n, ranks, ref, what=""):
    """out fp32 [C, nq], n int32 [C], ranks fp32 [C, nq, 2] or None from the library against oracle_percentiles' dict."""
    assert out.dtype == torch.float32 and n.dtype == torch.int32
    assert np.array_equal(n.cpu().numpy().astype(np.int64), ref["n"]), (what, n.cpu().numpy(), ref["n"])
    if ranks is not None:
        same_bits(ranks[..., 0], torch.from_numpy(ref["lo"]), what + " lower rank")
        same_bits(ranks[..., 1], torch.from_numpy(ref["hi"]), what + " upper rank")
    g, r = out.cpu().numpy().astype(np.float64), ref["value"]
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(np.isnan(g), np.isnan(r)), (what, "NaN positions differ", g, r)
    with np.errstate(invalid="ignore"):
        lo, hi = ref["lo"].astype(np.float64), ref["hi"].astype(np.float64)
        exact = lo == hi
        bound = np.where(exact, 0.0, np.maximum(2.0 ** -23 * np.maximum(np.abs(lo), np.abs(hi)), 2.0 ** -150))
        ok = ~np.isnan(r)
        inf = ok & np.isinf(r)
        assert np.array_equal(g[inf], r[inf]), (what, g, r)
        fin = ok & ~inf
        err = np.abs(g[fin] - r[fin])
    worst = float((err / np.maximum(bound[fin], 2.0 ** -150)).max()) if err.size else 0.0
    print(f"{what}: worst percentile error {worst:.3f} of its bound over {int(fin.sum())} values")
    assert np.all(err <= bound[fin]), (what, g, r, bound)


def check_percentiles(be, x, qs, above=None, what=""):
    """x fp32 [C, V] on the host. Returns the library's (out, n, ranks)."""
    dev = be.device
    ab = None if above is None else torch.as_tensor(above, dtype=torch.float32)
    out, n, ranks = be.percentiles(x.to(dev), list(qs), None if ab is None else ab.to(dev), want_ranks=True)
    assert out.shape == (x.shape[0], len(qs)) and ranks.shape == (x.shape[0], len(qs), 2) and n.shape == (x.shape[0],)
    check_percentile_values(out, n, ranks, oracle_percentiles(x, qs, None if ab is None else ab.numpy()), what or f"q={tuple(qs)}")
    plain = be.percentiles(x.to(dev), list(qs), None if ab is None else ab.to(dev))            # without ranks: the same values
    assert plain[2] is None and torch.equal(plain[0].view(torch.int32), out.view(torch.int32)) and torch.equal(plain[1], n)
    return out, n, ranks


def check_window(be, x, lo, hi, mode, floor=0.0, ceiling=1.0, channels=None, what=""):
    dev = be.device
    y = be.window(x.to(dev), lo.to(dev), None if hi is None else hi.to(dev), mode, floor, ceiling, channels)
    c = x.shape[0] if channels is None else channels
    assert y.dtype == torch.float32 and y.shape == (c,) + tuple(x.shape[1:])
    same_bits(y, torch_window(x, lo, hi, mode, floor, ceiling, channels), what or f"window mode {mode}")
    return y


def check_threshold_any(be, x, thr):
    got = be.threshold_any(x.to(be.device), thr.to(be.device))
    with np.errstate(invalid="ignore"):
        ref = (x.reshape(x.shape[0], -1) > thr.reshape(-1, 1)).any(dim=0).reshape(x.shape[1:])
    assert got.dtype == torch.uint8 and got.shape == x.shape[1:] and torch.equal(got.cpu().bool(), ref)
    assert int(got.max()) <= 1
    return got


def check_zscore(be, x, select, threshold=0.0, center=True, ddof=0, zero_std_to_one=False, what=""):
    y, n = be.zscore_select(x.to(be.device), select, threshold, center, ddof, zero_std_to_one)
    ref, sel, mean, std, cnt = oracle_zscore(x, select, threshold, center, ddof, zero_std_to_one)
    assert y.dtype == torch.float32 and y.shape == x.shape and n.dtype == torch.int32
    assert np.array_equal(n.cpu().numpy().astype(np.int64), cnt), (what, n.cpu().numpy(), cnt)
    a = x.reshape(x.shape[0], -1).numpy()
    g = y.cpu().reshape(x.shape[0], -1).numpy()
    assert np.array_equal(g.view(np.uint32)[~sel], a.view(np.uint32)[~sel]), (what, "voxels not selected changed")
    worst = 0.0
    for ch in range(a.shape[0]):
        gs, rs, xs = g[ch][sel[ch]].astype(np.float64), ref[ch][sel[ch]], a[ch][sel[ch]].astype(np.float64)
        assert np.array_equal(np.isnan(gs), np.isnan(rs)), (what, ch, "NaN positions differ", mean[ch], std[ch])
        ok = ~np.isnan(rs)
        inf = ok & np.isinf(rs)
        assert np.array_equal(gs[inf], rs[inf]), (what, ch)
        fin = ok & ~inf
        if not fin.any():
            continue
        bound = 2.0 ** -22 * (np.abs(xs[fin]) + abs(mean[ch])) / std[ch]
        err = np.abs(gs[fin] - rs[fin])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))))
        assert np.all(err <= bound), (what, ch, float(err.max()), mean[ch], std[ch])
    print(f"{what}: worst z-score error {worst:.3f} of its bound")
    return y, n


# ---- the composed functions: the restatement runs the parts on the same backend and holds each to its bound ----------------------------
def flat(t):
    return t.reshape(t.shape[0], -1)


def check_percentile_window(be, N, x, lo_q=5, hi_q=95):
    got = N.percentile_window(x.to(be.device), lo_q, hi_q, _backend=be)
    thr, _, _ = check_percentiles(be, flat(x), (lo_q, hi_q), what="percentile_window thresholds")
    thr = thr.cpu()
    assert got.shape == x.shape
    same_bits(got, torch_window(flat(x), thr[:, 0], thr[:, 1], WINDOW_CLAMP), "percentile_window")
    return got


def check_percentile_threshold(be, N, x, fraction):
    got = N.percentile_threshold(x.to(be.device), fraction, _backend=be)
    thr, _, _ = check_percentiles(be, flat(x), (fraction * 100,), what="percentile_threshold threshold")
    ref = (flat(x) > thr.cpu().reshape(-1, 1)).any(dim=0).reshape((1,) + tuple(x.shape[1:]))
    assert got.dtype == torch.bool and got.shape == ref.shape and torch.equal(got.cpu(), ref)
    return got


def check_zero_one_window(be, N, x, ceiling_percentile=99, floor_percentile=1, floor=0, ceiling=1):
    x4 = x if x.dim() == 4 else x[None]
    axis = (1, 2, 3) if x.dim() == 4 else (0, 1, 2)
    got = N.zero_one_window(x.to(be.device), axis, ceiling_percentile, floor_percentile, floor, ceiling, _backend=be)
    lo, _, _ = check_percentiles(be, flat(x4), (floor_percentile,), what="zero_one_window floor")
    lo = lo.cpu().reshape(-1)
    hi, _, _ = check_percentiles(be, flat(x4), (ceiling_percentile,), above=lo, what="zero_one_window ceiling")
    assert got.shape == x.shape
    same_bits(got, torch_window(flat(x4), lo, hi.cpu().reshape(-1), WINDOW_RESCALE, floor, ceiling), "zero_one_window")
    return got


def check_zero_floor(be, N, x, floor_percentile=1, floor=0):
    got = N.zero_floor_normalize_image_data(x.to(be.device), (1, 2, 3), floor_percentile, floor, _backend=be)
    thr, _, _ = check_percentiles(be, flat(x), (floor_percentile,), what="zero_floor threshold")
    shifted = check_window(be, flat(x), thr.cpu().reshape(-1), None, WINDOW_SHIFT_FLOOR, floor, what="zero_floor shift")
    y, _ = check_zscore(be, shifted.cpu(), SELECT_ALL, 0.0, False, 1, False, what="zero_floor scale")
    assert got.shape == x.shape and torch.equal(flat(got).view(torch.int32), y.view(torch.int32))
    return got


def check_foreground(be, N, x, background_value=0, tolerance=1e-5):
    got = N.foreground_zero_mean_normalize_image_data(x.to(be.device), 0, background_value, tolerance, _backend=be)
    y, _ = check_zscore(be, flat(x), SELECT_ABS_ABOVE, background_value + tolerance, True, 1, False, what="foreground_zero_mean")
    assert got.shape == x.shape and torch.equal(flat(got).view(torch.int32), y.view(torch.int32))
    return got


def check_static_windows(be, N, x3, windows, floor=0, ceiling=1):
    got = N.static_windows(x3.to(be.device), windows, floor, ceiling, _backend=be)
    lo = torch.tensor([l - w / 2 for l, w in windows], dtype=torch.float32)      # noqa: E741
    hi = torch.tensor([l + w / 2 for l, w in windows], dtype=torch.float32)      # noqa: E741
    sq = torch.squeeze(x3)
    assert got.shape == tuple(sq.shape) + (len(windows),)
    ref = torch_window(sq.reshape(1, -1), lo, hi, WINDOW_RESCALE, floor, ceiling, channels=len(windows))
    same_bits(got.movedim(-1, 0), ref, "static_windows")
    one = N.radiology_style_windowing(sq.to(be.device), windows[0][0], windows[0][1], floor, ceiling, _backend=be)
    assert one.shape == sq.shape
    same_bits(one, ref[0], "radiology_style_windowing")
    return got


# ---- the committed reference fixture -------------------------------------------------------------------------------------------------
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = torch.load(GOLDEN, map_location="cpu", weights_only=True)
    return _FIXTURE


def check_against_reference(be, N):
    """The functions on the fixture's fp32 inputs against what the reference's own code returned (float64 where it ran on the float64
    copies). Reads nothing but the fixture."""
    fx = fixture()
    dev = be.device
    for name in ("a", "b"):
        x = fx[name]
        for lo_q, hi_q in fx["window_percentiles"]:
            ref = fx[f"percentile_window_{name}_{lo_q}_{hi_q}"]                     # float64: clamp(x, np.percentile(lo_q), np.percentile(hi_q))
            got = N.percentile_window(x.to(dev), lo_q, hi_q, _backend=be).cpu().double()
            o = oracle_percentiles(flat(x), (lo_q, hi_q))
            # a clamped voxel holds a threshold, within the percentile bound of the reference's; any other voxel is x on both sides, or
            # lies between the two thresholds
            bound = 2.0 ** -23 * np.maximum(np.abs(o["lo"].astype(np.float64)), np.abs(o["hi"].astype(np.float64))).max(axis=1)
            err = flat((got - ref).abs()).max(dim=1).values.numpy()
            print(f"percentile_window {name} {lo_q}/{hi_q} against the reference: {err} within {bound}")
            assert np.all(err <= bound), (name, err, bound)
            thr = be.percentiles(flat(x).to(dev), [lo_q, hi_q])[0].cpu().double().numpy()
            refthr = np.stack([flat(ref).min(dim=1).values.numpy(), flat(ref).max(dim=1).values.numpy()], axis=1)
            tb = 2.0 ** -23 * np.maximum(np.abs(o["lo"].astype(np.float64)), np.abs(o["hi"].astype(np.float64)))
            assert np.all(np.abs(thr - refthr) <= tb), (name, thr, refthr)
        for fraction in fx["threshold_fractions"]:
            ref = fx[f"percentile_threshold_{name}_{fraction}"]
            got = N.percentile_threshold(x.to(dev), fraction, _backend=be)
            assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (name, fraction)
    b = fx["b"]
    ref = fx["foreground_zero_mean_b"]                                              # float64, the single-channel branch
    got = N.foreground_zero_mean_normalize_image_data(b.to(dev), _backend=be).cpu()
    sel = b.abs() > 1e-5
    assert torch.equal(got[~sel].view(torch.int32), b[~sel].view(torch.int32)) and torch.equal(ref[~sel], b[~sel].double())
    fg = b[sel].double()
    bound = 2.0 ** -22 * (fg.abs() + fg.mean().abs()) / fg.std()
    err = (got[sel].double() - ref[sel]).abs()
    print(f"foreground_zero_mean against the reference: worst {float((err / bound).max()):.3f} of its bound")
    assert bool((err <= bound).all())
    ct, windows = fx["ct"], [tuple(w) for w in fx["windows"]]
    same_bits(N.static_windows(ct.to(dev), windows, _backend=be), fx["static_windows_ct"], "static_windows against the reference")
    lvl, wid = fx["radiology_window"]
    same_bits(N.radiology_style_windowing(ct[0].to(dev), lvl, wid, _backend=be), fx["radiology_ct"], "radiology_style_windowing against the reference")
