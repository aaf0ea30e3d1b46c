"""Percentile statistics, intensity windows, the z-score over a selected set and the any-channel threshold (csrc/intensity.hip,
3dunetcnn_amd/normalize.py) on the CPU emulator of the same kernel sources, against the oracles and bounds of tests/normalize_cases.py,
on hostile memory, through the C ABI."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import normalize_cases as K
import scratch_guard as G

normalize = importlib.import_module("3dunetcnn_amd.normalize")
prepost = importlib.import_module("3dunetcnn_amd.prepost")
_lib = importlib.import_module("3dunetcnn_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = {"mi355_percentiles", "mi355_window", "mi355_zscore_select", "mi355_threshold_any"}
LAUNCHES = {"percentiles": 10, "window": 1, "zscore_select": 3, "threshold_any": 1}      # as include/mi355_unet3d.h states them


# ---- the oracles themselves (no backend) -----------------------------------------------------------------------------------------------
def test_oracle_is_numpy_percentile_on_float64():
    """np.percentile on float64 input is the double rule; its interpolation is a + (b - a) * t below t = 0.5 and b - (b - a) * (1 - t)
    above, the oracle's always the first: each form is three double roundings of magnitudes <= 2 * max(|lo|, |hi|) away from the exact
    value, so the two differ by at most 12 * 2^-53 * max(|lo|, |hi|)."""
    for kind in ("gauss100", "offset1000", "tiny_minus5", "zeros60", "duplicates", "low_byte"):
        for v in (1, 2, 3, 257, 4099, K.LARGE_SIZE):
            x = K.values(kind, 2, v, seed=3)
            o = K.oracle_percentiles(x, K.PERCENTILES)
            ref = np.percentile(x.numpy().astype(np.float64), K.PERCENTILES, axis=1).T
            bound = 12 * 2.0 ** -53 * np.maximum(np.abs(o["lo"]), np.abs(o["hi"])).astype(np.float64)
            assert np.all(np.abs(o["value"] - ref) <= bound), (kind, v)
    x = K.values("one_nan", 2, 257)
    o = K.oracle_percentiles(x, (50,))
    assert np.isnan(o["value"][0, 0]) and np.isnan(np.percentile(x.numpy()[0].astype(np.float64), 50)) and not np.isnan(o["value"][1, 0])


def test_restatements_are_pinned_to_the_reference_fixture():
    """The float64 restatements reproduce what the reference's own functions returned (tests/golden/normalize_reference.pt)."""
    fx = K.fixture()
    for name in ("a", "b"):
        x = fx[name]
        for lo_q, hi_q in fx["window_percentiles"]:
            o = K.oracle_percentiles(K.flat(x), (lo_q, hi_q))["value"]
            mine = torch.clamp(K.flat(x).double(), torch.from_numpy(o[:, :1]), torch.from_numpy(o[:, 1:])).reshape(x.shape)
            ref = fx[f"percentile_window_{name}_{lo_q}_{hi_q}"]
            assert ref.dtype == torch.float64 and float((mine - ref).abs().max()) <= 12 * 2.0 ** -53 * float(x.abs().max())
        for fraction in fx["threshold_fractions"]:
            o = K.oracle_percentiles(K.flat(x), (fraction * 100,))["value"]
            mine = (K.flat(x).double() > torch.from_numpy(o)).any(dim=0).reshape((1,) + tuple(x.shape[1:]))
            assert torch.equal(mine, fx[f"percentile_threshold_{name}_{fraction}"])
            # no voxel lies between the double threshold and its fp32 rounding: the fp32 comparison gives the same mask
            o32 = torch.from_numpy(o.astype(np.float32))
            assert torch.equal((K.flat(x) > o32).any(dim=0).reshape(mine.shape), mine)
    b = fx["b"]
    y, sel, _, _, _ = K.oracle_zscore(K.flat(b), K.SELECT_ABS_ABOVE, 1e-5, True, 1, False)
    assert np.allclose(y.reshape(b.shape), fx["foreground_zero_mean_b"].numpy(), rtol=1e-12, atol=1e-12) and 0 < sel.sum() < sel.size
    ct, windows = fx["ct"], [tuple(w) for w in fx["windows"]]
    lo = torch.tensor([l - w / 2 for l, w in windows], dtype=torch.float32)      # noqa: E741
    hi = torch.tensor([l + w / 2 for l, w in windows], dtype=torch.float32)      # noqa: E741
    mine = K.torch_window(ct.reshape(1, -1), lo, hi, K.WINDOW_RESCALE, 0, 1, channels=len(windows)).reshape(len(windows), *ct.shape[1:])
    K.same_bits(mine.movedim(0, -1), fx["static_windows_ct"], "static_windows restatement")
    assert fx["static_windows_ct"].shape == tuple(ct.shape[1:]) + (len(windows),)


# ---- percentiles -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.VALUE_SETS)
def test_percentiles_of_small_volumes(emu_backend, kind):
    for c in K.CHANNELS:
        for v in K.SMALL_SIZES:
            x = K.values(kind, c, v)
            for qs in K.Q_SETS if v in (3, 257, 4099) else K.Q_SETS[1:4:2]:
                K.check_percentiles(emu_backend, x, qs, what=f"{kind} c={c} v={v} q={qs}")


@pytest.mark.parametrize("kind", ("offset1000", "zeros60", "mixed"))
def test_percentiles_with_several_workgroups(emu_backend, kind):
    x = K.values(kind, 3, K.LARGE_SIZE)
    K.check_percentiles(emu_backend, x, (1, 50, 0.9 * 100, 99.9), what=f"{kind} v={K.LARGE_SIZE}")
    K.check_percentiles(emu_backend, x, (33.3,), what=f"{kind} v={K.LARGE_SIZE}")


@pytest.mark.parametrize("v", (3, 257, 4099))
def test_percentiles_above_a_device_threshold(emu_backend, v):
    """Thresholds that leave 0, 1, 2 and many values, and a NaN threshold (selects nothing); a NaN VALUE never exceeds a threshold."""
    for kind in ("gauss100", "zeros60", "one_nan"):
        x = K.values(kind, 3, v)
        s = np.sort(x.numpy()[~np.isnan(x.numpy())].reshape(-1))
        for above in ([s[-1]] * 3, [s[-2], s[-1], s[-3]], [s[-3], s[-2], K.NAN], [s[s.size // 3], 0.0, -np.inf], [K.NAN] * 3):
            for qs in ((0, 50, 99, 100), (0.9 * 100,)):
                K.check_percentiles(emu_backend, x, qs, above=above, what=f"{kind} v={v} above={above}")


# ---- windows, threshold ----------------------------------------------------------------------------------------------------------------
def window_inputs(c, v):
    x = K.values("mixed", c, v, seed=2)
    if v > 4:
        x[0, 1], x[c - 1, v - 2] = K.NAN, K.NAN
    return x


@pytest.mark.parametrize("v", (1, 3, 255, 257, 4099))
def test_windows_are_the_torch_expressions(emu_backend, v):
    be = emu_backend
    for c in K.CHANNELS:
        x = window_inputs(c, v)
        bounds = [(torch.tensor([-1.5, 0.0, -np.inf][:c]), torch.tensor([2.5, 0.0, 1e-40][:c])),
                  (torch.tensor([2.5, K.NAN, 1.0][:c]), torch.tensor([-1.5, 1.0, K.NAN][:c]))]      # lo > hi, NaN bounds, hi == lo
        for lo, hi in bounds:
            K.check_window(be, x, lo, hi, K.WINDOW_CLAMP)
            K.check_window(be, x, lo, hi, K.WINDOW_RESCALE, 0, 1)
            K.check_window(be, x, lo, hi, K.WINDOW_RESCALE, -0.5, 2.0)
            K.check_window(be, x, lo, None, K.WINDOW_SHIFT_FLOOR, 0)
            K.check_window(be, x, lo, hi, K.WINDOW_SHIFT_FLOOR, -3.0)
            K.check_threshold_any(be, x, lo)
        g = K.values("gauss100", c, v, seed=5)
        K.check_window(be, g, g.min(dim=1).values * 0.5, g.max(dim=1).values * 0.5, K.WINDOW_RESCALE, 0, 1)
        K.check_threshold_any(be, g, g.median(dim=1).values)
    one = window_inputs(1, v)                                  # one input channel behind three windows
    K.check_window(be, one, torch.tensor([-1.5, 0.0, 2.5]), torch.tensor([2.5, 0.0, 7e37]), K.WINDOW_RESCALE, 0, 1, channels=3)


# ---- z-score over a selected set -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("gauss100", "offset1000", "tiny_minus5", "zeros60", "duplicates"))
def test_zscore_select_within_its_bound(emu_backend, kind):
    be = emu_backend
    for c in K.CHANNELS:
        for v in (2, 3, 257, 4099):
            x = K.values(kind, c, v)
            for select, thr in ((K.SELECT_ALL, 0.0), (K.SELECT_NONZERO, 0.0), (K.SELECT_ABS_ABOVE, 1.5)):
                for center, ddof, z in ((True, 0, True), (True, 1, False), (False, 1, False)):
                    K.check_zscore(be, x, select, thr, center, ddof, z, what=f"{kind} c={c} v={v} select={select} {center, ddof, z}")


def test_zscore_select_where_a_naive_fp32_sum_of_squares_fails(emu_backend):
    x = K.values("offset1000", 3, K.LARGE_SIZE)
    K.check_zscore(emu_backend, x, K.SELECT_ALL, 0.0, True, 1, False, what="offset1000 large")
    K.check_zscore(emu_backend, K.values("zeros60", 3, K.LARGE_SIZE), K.SELECT_NONZERO, 0.0, True, 0, True, what="zeros60 large")


def test_zscore_select_edge_cases(emu_backend):
    be = emu_backend
    x = K.values("gauss100", 3, 257)
    y, n = K.check_zscore(be, x, K.SELECT_ABS_ABOVE, 1e9, True, 1, False, what="nothing selected")      # n == 0: the channel is copied
    assert n.tolist() == [0, 0, 0] and torch.equal(y.cpu().view(torch.int32), x.view(torch.int32))
    one = torch.zeros(2, 257); one[0, 100] = 4.0; one[1, 3] = -2.0; one[1, 200] = -2.0
    y, n = K.check_zscore(be, one, K.SELECT_NONZERO, 0.0, True, 1, False, what="n == 1 with ddof == 1")
    assert n.tolist() == [1, 2] and bool(torch.isnan(y[0, 100])) and bool(torch.isnan(y[1, 3]))           # 0 / 0 both: as torch
    y, _ = K.check_zscore(be, one, K.SELECT_NONZERO, 0.0, True, 0, True, what="std 0 counts as 1")
    assert float(y[0, 100]) == 0.0 and float(y[1, 200]) == 0.0 and int((y != 0).sum()) == 0
    const = K.values("all_equal", 3, 255)
    y, _ = K.check_zscore(be, const, K.SELECT_ALL, 0.0, True, 0, False, what="std 0, IEEE")
    assert bool(torch.isnan(y).all())
    y, _ = K.check_zscore(be, const, K.SELECT_ALL, 0.0, False, 0, False, what="std 0, IEEE, not centred")
    assert bool(torch.isinf(y[:2]).all()) and bool(torch.isnan(y[2]).all())
    y, _ = K.check_zscore(be, const, K.SELECT_ALL, 0.0, True, 0, True, what="std 0 counts as 1, constant")
    assert float(y.abs().max()) == 0.0


# ---- the public functions --------------------------------------------------------------------------------------------------------------
def volume(kind, c, dhw, seed=0):
    return K.values(kind, c, dhw[0] * dhw[1] * dhw[2], seed).reshape(c, *dhw)


@pytest.mark.parametrize("kind", ("gauss100", "zeros60", "offset1000"))
def test_composed_functions_against_their_restatements(emu_backend, kind):
    be = emu_backend
    for c, dhw in ((3, (5, 6, 7)), (1, (9, 10, 11))):
        x = volume(kind, c, dhw)
        K.check_percentile_window(be, normalize, x)
        K.check_percentile_threshold(be, normalize, x, 0.9)
        K.check_zero_one_window(be, normalize, x)
        K.check_zero_floor(be, normalize, x)
        K.check_foreground(be, normalize, x)
    K.check_zero_one_window(be, normalize, volume(kind, 1, (5, 6, 7))[0], 95, 5, -1, 2)      # [D, H, W] with every axis
    K.check_static_windows(be, normalize, volume("gauss100", 1, (5, 6, 7), 3) * 4, [(40, 80), (50, 350), (-600, 1500)])


def test_what_the_functions_mean(emu_backend):
    be = emu_backend
    host = volume("zeros60", 2, (5, 6, 7))
    x = host.to(be.device)
    q = normalize.percentiles(x, (0, 50, 100, 25, 75), _backend=be).cpu()             # more than four: several calls
    assert q.shape == (2, 5) and torch.equal(q[:, 0], K.flat(host).min(dim=1).values) and torch.equal(q[:, 2], K.flat(host).max(dim=1).values)
    assert normalize.percentiles(x, 50, _backend=be).shape == (2, 1)
    const = torch.full((1, 5, 6, 7), 2.5).to(be.device)      # no foreground above the floor: NaN ceiling, NaN channel (documented)
    assert bool(torch.isnan(normalize.zero_one_window(const, _backend=be)).all())
    for fn, args in ((normalize.zero_one_window, (x[0], (1, 2))), (normalize.zero_floor_normalize_image_data, (x, (2, 3))),
                     (normalize.zero_one_window, (x, (1, 2, 3), 99, 1, 0, 1, 3))):
        with pytest.raises(NotImplementedError):
            fn(*args, _backend=be)
    with pytest.raises(RuntimeError, match="MI355X"):
        normalize.percentile_window(host)
    # prepost.normalize_intensity(nonzero=True): MONAI's rule -- the nonzero voxels' own mean and std (ddof 0), the others untouched
    y = prepost.normalize_intensity(x, nonzero=True, _backend=be)
    ref, sel, _, _, _ = K.oracle_zscore(K.flat(host), K.SELECT_NONZERO, 0.0, True, 0, True)
    assert bool((K.flat(y.cpu())[torch.from_numpy(~sel)] == 0).all()) and np.allclose(K.flat(y.cpu()).numpy(), ref, rtol=0, atol=1e-5)
    y5 = prepost.normalize_intensity(x[None], nonzero=True, _backend=be)
    assert torch.equal(y5[0].view(torch.int32), y.view(torch.int32))
    with pytest.raises(NotImplementedError):
        prepost.normalize_intensity(x, channel_wise=False, _backend=be)


def test_reference_fixture(emu_backend):
    K.check_against_reference(emu_backend, normalize)


def test_module_never_waits_for_the_host():
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "normalize.py")).read()
    for word in (".item()", ".tolist()", ".cpu()", "synchronize", ".numpy()"):
        assert word not in src, word


# ---- hostile memory ------------------------------------------------------------------------------------------------------------------------
def _hostile_volume():
    return volume("zeros60", 3, (5, 7, 119))                  # 4165 voxels per channel: odd, several trips, a partial last one


HOSTILE = {
    "percentiles": lambda be, x: be.percentiles(K.flat(x), [1, 50, 0.9 * 100, 99], want_ranks=True),
    "percentiles_above": lambda be, x: be.percentiles(K.flat(x), [99], above=be.percentiles(K.flat(x), [1])[0].reshape(-1)),
    "window": lambda be, x: [be.window(K.flat(x), K.flat(x)[:, 0].contiguous(), K.flat(x)[:, 1].contiguous() + 100, m, 0, 1) for m in (0, 1, 2)],
    "zscore_select": lambda be, x: [be.zscore_select(x, s, 1.5, True, 1, False) for s in (0, 1, 2)],
    "threshold_any": lambda be, x: be.threshold_any(x, K.flat(x)[:, 5].contiguous()),
    "percentile_window": lambda be, x: normalize.percentile_window(x, _backend=be),
    "percentile_threshold": lambda be, x: normalize.percentile_threshold(x, 0.9, _backend=be),
    "zero_one_window": lambda be, x: normalize.zero_one_window(x, _backend=be),
    "zero_floor": lambda be, x: normalize.zero_floor_normalize_image_data(x, _backend=be),
    "foreground_zero_mean": lambda be, x: normalize.foreground_zero_mean_normalize_image_data(x, _backend=be),
    "static_windows": lambda be, x: normalize.static_windows(x[:1], [(40, 80), (300, 100)], _backend=be),
    "normalize_intensity_nonzero": lambda be, x: prepost.normalize_intensity(x, nonzero=True, _backend=be),
}


def hold_op(be, name):
    """scratch_guard.hold: clean twice (same bits), then with every `empty` tensor pre-filled with QNAN and with ONES inside guard
    bands: same bits again, every guard byte untouched."""
    x = _hostile_volume().to(be.device)
    held = G.hold(be, lambda: HOSTILE[name](be, x), fills=(G.QNAN, G.ONES), modules=(normalize,))
    assert held.results >= 1 and held.allocations >= 1, held
    return held


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_op_on_hostile_memory(emu_backend, name):
    held = hold_op(emu_backend, name)
    if name == "percentiles":
        assert held.allocations == 4                          # values, counts, ranks, scratch


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(emu_backend):
    lib = emu_backend.lib
    c, v = 2, 300
    x, y = K.values("gauss100", c, v), torch.zeros(c, v)
    lo, hi = torch.zeros(c), torch.ones(c)
    out, ranks, n = torch.zeros(c, 4), torch.zeros(c, 4, 2), torch.zeros(c, dtype=torch.int32)
    mask = torch.zeros(v, dtype=torch.uint8)
    ps = torch.zeros(c * _lib.PERCENTILE_SCRATCH_BYTES // 8 + 1, dtype=torch.float64)
    zs = torch.zeros(c * _lib.ZSCORE_SELECT_SCRATCH_BYTES // 8 + 1, dtype=torch.float64)
    xp, yp, lp, hp, op, rp, np_, mp, pp, zp = (t.data_ptr() for t in (x, y, lo, hi, out, ranks, n, mask, ps, zs))
    big = 2 ** 31 - 1
    nan = float("nan")

    def q(*vals):
        return (ctypes.c_double * len(vals))(*vals)

    q2 = q(5.0, 95.0)
    assert lib.mi355_percentiles(xp, c, v, q2, 2, lp, op, rp, np_, pp, 0) == 0
    assert lib.mi355_percentiles(xp, c, v, q2, 2, None, op, None, np_, pp, 0) == 0      # above and ranks are optional
    for args in ((None, c, v, q2, 2, lp, op, rp, np_, pp), (xp, c, v, None, 2, lp, op, rp, np_, pp), (xp, c, v, q2, 2, lp, None, rp, np_, pp),
                 (xp, c, v, q2, 2, lp, op, rp, None, pp), (xp, c, v, q2, 2, lp, op, rp, np_, None), (xp, c, v, q2, 2, lp, op, rp, np_, pp + 4),
                 (xp, 0, v, q2, 2, lp, op, rp, np_, pp), (xp, 65536, v, q2, 2, lp, op, rp, np_, pp), (xp, c, 0, q2, 2, lp, op, rp, np_, pp),
                 (xp, c, big, q2, 2, lp, op, rp, np_, pp), (xp, c, v, q2, 0, lp, op, rp, np_, pp),
                 (xp, c, v, q(1.0, 2.0, 3.0, 4.0, 5.0), 5, lp, op, rp, np_, pp), (xp, c, v, q(5.0, -0.5), 2, lp, op, rp, np_, pp),
                 (xp, c, v, q(100.5, 5.0), 2, lp, op, rp, np_, pp), (xp, c, v, q(5.0, nan), 2, lp, op, rp, np_, pp)):
        assert lib.mi355_percentiles(*args, 0) == EINVAL, args

    for mode in (0, 1, 2):
        assert lib.mi355_window(xp, c, yp, c, v, lp, hp, mode, 0.0, 1.0, 0) == 0
    assert lib.mi355_window(xp, 1, yp, c, v, lp, hp, 1, 0.0, 1.0, 0) == 0 and lib.mi355_window(xp, c, yp, c, v, lp, None, 2, 0.0, 1.0, 0) == 0
    for args in ((None, c, yp, c, v, lp, hp, 0), (xp, c, None, c, v, lp, hp, 0), (xp, c, yp, c, v, None, hp, 0), (xp, c, yp, c, v, lp, None, 0),
                 (xp, c, yp, c, v, lp, None, 1), (xp, c, yp, 0, v, lp, hp, 0), (xp, c, yp, 65536, v, lp, hp, 0), (xp, c, yp, c, 0, lp, hp, 0),
                 (xp, c, yp, c, big, lp, hp, 0), (xp, 3, yp, c, v, lp, hp, 0), (xp, 0, yp, c, v, lp, hp, 0), (xp, c, yp, c, v, lp, hp, 3),
                 (xp, c, yp, c, v, lp, hp, -1)):
        assert lib.mi355_window(*args, 0.0, 1.0, 0) == EINVAL, args

    assert lib.mi355_zscore_select(xp, yp, c, v, 2, 1.5, 1, 1, 0, np_, zp, 0) == 0
    for args in ((None, yp, c, v, 0, 0.0, 1, 0, 0, np_, zp), (xp, None, c, v, 0, 0.0, 1, 0, 0, np_, zp), (xp, yp, c, v, 0, 0.0, 1, 0, 0, None, zp),
                 (xp, yp, c, v, 0, 0.0, 1, 0, 0, np_, None), (xp, yp, c, v, 0, 0.0, 1, 0, 0, np_, zp + 4), (xp, yp, 0, v, 0, 0.0, 1, 0, 0, np_, zp),
                 (xp, yp, c, 0, 0, 0.0, 1, 0, 0, np_, zp), (xp, yp, c, big, 0, 0.0, 1, 0, 0, np_, zp), (xp, yp, c, v, 3, 0.0, 1, 0, 0, np_, zp),
                 (xp, yp, c, v, -1, 0.0, 1, 0, 0, np_, zp), (xp, yp, c, v, 0, 0.0, 1, 2, 0, np_, zp), (xp, yp, c, v, 0, 0.0, 1, -1, 0, np_, zp),
                 (xp, yp, c, v, 2, nan, 1, 0, 0, np_, zp)):
        assert lib.mi355_zscore_select(*args, 0) == EINVAL, args

    assert lib.mi355_threshold_any(xp, c, v, lp, mp, 0) == 0
    for args in ((None, c, v, lp, mp), (xp, c, v, None, mp), (xp, c, v, lp, None), (xp, 0, v, lp, mp), (xp, 65536, v, lp, mp), (xp, c, 0, lp, mp),
                 (xp, c, big, lp, mp)):
        assert lib.mi355_threshold_any(*args, 0) == EINVAL, args
    with pytest.raises(RuntimeError, match="percentiles"):
        emu_backend.percentiles(x, [101.0])


def _take(be):
    fn = be.lib.emu_take_launches
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(8192)
    fn(buf, 8192)
    return buf.value.decode().split()


def test_header_signatures_and_launch_counts(emu_backend):
    be = emu_backend
    hdr = open(os.path.join(ROOT, "include", "mi355_unet3d.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.SIGNATURES) and declared == set(_lib.SIGNATURES)
    for name in NEW:
        assert hasattr(be.lib, name)
    assert not [n for n in NEW if n.endswith(("_workspace", "_blocks"))]
    for macro, value in (("PERCENTILE_MAX_Q", _lib.PERCENTILE_MAX_Q), ("PERCENTILE_SCRATCH_BYTES", _lib.PERCENTILE_SCRATCH_BYTES),
                         ("ZSCORE_SELECT_SCRATCH_BYTES", _lib.ZSCORE_SELECT_SCRATCH_BYTES), ("WINDOW_CLAMP", _lib.WINDOW_CLAMP),
                         ("WINDOW_RESCALE", _lib.WINDOW_RESCALE), ("WINDOW_SHIFT_FLOOR", _lib.WINDOW_SHIFT_FLOOR), ("SELECT_ALL", _lib.SELECT_ALL),
                         ("SELECT_NONZERO", _lib.SELECT_NONZERO), ("SELECT_ABS_ABOVE", _lib.SELECT_ABS_ABOVE)):
        assert int(re.search(rf"#define MI355_{macro} (\d+)", hdr).group(1)) == value, macro
    assert (K.WINDOW_CLAMP, K.WINDOW_RESCALE, K.WINDOW_SHIFT_FLOOR) == (_lib.WINDOW_CLAMP, _lib.WINDOW_RESCALE, _lib.WINDOW_SHIFT_FLOOR)
    assert (K.SELECT_ALL, K.SELECT_NONZERO, K.SELECT_ABS_ABOVE) == (_lib.SELECT_ALL, _lib.SELECT_NONZERO, _lib.SELECT_ABS_ABOVE)
    assert _lib.PERCENTILE_SCRATCH_BYTES % 8 == 0 and _lib.ZSCORE_SELECT_SCRATCH_BYTES % 8 == 0
    for word, count in (("Ten launches", LAUNCHES["percentiles"]), ("Three launches", LAUNCHES["zscore_select"])):
        assert word in hdr[hdr.index("csrc/intensity.hip"):], (word, count)

    # the same launches for no participating value (a NaN threshold), constant and random data
    nothing = torch.full((3,), K.NAN)
    seen = {}
    for label, x, above in (("empty", K.values("gauss100", 3, 4099), nothing), ("constant", K.values("all_equal", 3, 4099), None),
                            ("random", K.values("mixed", 3, 4099), None)):
        calls = {"percentiles": lambda: be.percentiles(x, [1, 50, 99, 100], above),
                 "window": lambda: be.window(x, x[:, 0].contiguous(), x[:, 1].contiguous(), K.WINDOW_RESCALE),
                 "zscore_select": lambda: be.zscore_select(x, K.SELECT_ABS_ABOVE, 1e30 if label == "empty" else 0.5, True, 1, False),
                 "threshold_any": lambda: be.threshold_any(x, x[:, 0].contiguous()),
                 "zero_one_window": lambda: normalize.zero_one_window(x.reshape(3, 1, 1, -1), _backend=be),
                 "zero_floor": lambda: normalize.zero_floor_normalize_image_data(x.reshape(3, 1, 1, -1), _backend=be)}
        for name, call in calls.items():
            _take(be)
            call()
            seen.setdefault(name, []).append(_take(be))
    for name, runs in seen.items():
        assert runs[0] == runs[1] == runs[2], (name, runs)
    for name, count in LAUNCHES.items():
        assert len(seen[name][0]) == count, (name, seen[name][0])
    assert len(seen["zero_one_window"][0]) == 2 * LAUNCHES["percentiles"] + LAUNCHES["window"]
    assert len(seen["zero_floor"][0]) == LAUNCHES["percentiles"] + LAUNCHES["window"] + LAUNCHES["zscore_select"]


def test_source_has_no_host_round_trip_and_only_integer_atomics():
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", "intensity.hip")).read()
    for word in ("hipMalloc", "hipMemcpy", "Synchronize", "hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipFree"):
        assert word not in src, word
    # every atomic's operand is an int object of this file: a histogram bin (LDS or scratch) or the NaN counter
    targets = re.findall(r"atomic\w+\(\s*&?\s*([^,]+),", src)
    assert len(targets) >= 4
    for t in targets:
        assert re.match(r"(lh\[|S->hist\[|S->nan$)", t.strip()), t
    assert re.findall(r"atomic(\w+)\(", src).count("Add") == len(targets)
    for decl in (r"int hist\[", r"int n, nan;", r"__shared__ int lh\["):
        assert re.search(decl, src), decl
