"""Overlap counts, mask edges, the exact Euclidean distance transform and the surface-distance statistics (csrc/metrics.hip,
3dunetcnn_amd/metrics.py) on the CPU emulator of the same kernel sources, against the oracles of tests/metrics_cases.py: exact where
the answer is an integer, relative 1e-6 elsewhere (derived in metrics_cases), on hostile memory, through the C ABI."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_cases as M
import scratch_guard as G

metrics = importlib.import_module("3dunetcnn_amd.metrics")
prepost = importlib.import_module("3dunetcnn_amd.prepost")
_lib = importlib.import_module("3dunetcnn_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = M.constructed_cases()
PAIRS = M.edge_set_pairs()
NEW = {"mi355_seg_counts", "mi355_mask_edges", "mi355_edt", "mi355_surface_stats"}


_random_cases = M.random_cases


# ---- the oracles themselves ------------------------------------------------------------------------------------------------------------
def test_oracles_are_pinned_to_each_other_and_to_scipy():
    masks = [(CASES[n][-1], M.SPACINGS) for n in sorted(CASES)]
    masks += [(M.random_mask(1, e, p, 7)[0], (M.SPACINGS[0], M.SPACINGS[1 + i % 2])) for e in M.EXTENTS for i, p in enumerate(M.DENSITIES)]
    for m, spacings in masks:
        sites = m != 0
        for sp in spacings:
            sep = M.separable_dist2(sites, sp)
            if sites.numel() * max(int(sites.sum()), 1) <= M.BRUTE_PAIRS:
                brute = M.brute_dist2(sites, sp).double()
                brute = torch.where(brute < 0, torch.tensor(float("inf"), dtype=torch.float64), brute)
                if tuple(sp) == (1, 1, 1):
                    assert torch.equal(brute, sep)
                else:
                    assert torch.allclose(brute, sep, rtol=1e-12, atol=0)
            if M.have_scipy() and bool(sites.any()):
                ref = M.scipy_dist2(sites, sp)
                if tuple(sp) == (1, 1, 1):
                    assert torch.equal(torch.from_numpy(np.rint(ref.numpy())), sep)
                else:
                    assert torch.allclose(ref, sep, rtol=1e-12, atol=0)
        if M.have_scipy():
            assert torch.equal(M.torch_edges(m[None])[0], M.scipy_edges(m))


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dhw", M.EXTENTS, ids=M.ids)
def test_counts_and_ratios_match_the_oracle(emu_backend, dhw):
    for _, pred, truth in _random_cases(dhw):
        M.check_counts(emu_backend, metrics, pred, truth)


def test_counts_of_the_constructed_masks(emu_backend):
    be = emu_backend
    for name in sorted(CASES):
        M.check_counts(be, metrics, CASES[name], CASES[name])
        M.check_counts(be, metrics, CASES[name], torch.roll(CASES[name], 1, dims=3))
    e = CASES["empty"]
    assert metrics.dice_score(e, e, _backend=be).tolist() == [1.0, 1.0] and metrics.iou(e, e, _backend=be).tolist() == [1.0, 1.0]
    assert bool(torch.isnan(metrics.sensitivity(e, e, _backend=be)).all()) and bool(torch.isnan(metrics.precision(e, e, _backend=be)).all())
    # the 16-byte path and the bytewise one: an unaligned channel base (odd voxel count) and a 3-D input of another dtype
    odd = M.random_mask(3, (3, 5, 7), 0.5, 1)
    M.check_counts(be, metrics, odd, M.random_mask(3, (3, 5, 7), 0.5, 2))
    c3 = metrics.confusion_counts(odd[1].bool(), (odd[2] * 7).float(), _backend=be)
    assert c3.shape == (1, 4) and torch.equal(c3.long(), M.oracle_counts(odd[1:2], odd[2:3]))


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dhw", M.EXTENTS, ids=M.ids)
def test_edges_of_random_masks(emu_backend, dhw):
    for _, mask, _t in _random_cases(dhw):
        M.check_edges(emu_backend, metrics, mask)


def test_edges_of_the_constructed_masks(emu_backend):
    for name in sorted(CASES):
        M.check_edges(emu_backend, metrics, CASES[name])
    box = M.check_edges(emu_backend, metrics, CASES["box_at_border"])
    assert int(box[0, 0, 5, 50]) == 1 and int(box[0, 2, 5, 69]) == 1 and int(box[0, 2, 5, 50]) == 0       # the border counts as an edge
    full = metrics.mask_edges(CASES["full"][0], _backend=emu_backend)                                      # 3-D in, 3-D out
    assert full.shape == M.BASE and int(full.sum()) == 9 * 10 * 70 - 7 * 8 * 68


# ---- distance transform ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dhw", M.EXTENTS, ids=M.ids)
def test_edt_unit_spacing_is_bit_exact(emu_backend, dhw):
    for key, mask, _t in _random_cases(dhw):
        M.check_edt_unit(emu_backend, metrics, mask, key)


@pytest.mark.parametrize("name", sorted(CASES))
def test_edt_of_the_constructed_masks(emu_backend, name):
    M.check_edt_unit(emu_backend, metrics, CASES[name], name)
    for sp in M.SPACINGS[1:]:
        M.check_edt_spacing(emu_backend, metrics, CASES[name], sp, name)


@pytest.mark.parametrize("spacing", M.SPACINGS[1:], ids=M.ids)
@pytest.mark.parametrize("dhw", M.EXTENTS, ids=M.ids)
def test_edt_with_spacing(emu_backend, dhw, spacing):
    for key, mask, _t in _random_cases(dhw):
        M.check_edt_spacing(emu_backend, metrics, mask, spacing, key)


def test_what_the_edt_means(emu_backend):
    be = emu_backend
    single = CASES["single_voxel"]
    d2 = metrics.distance_to(single[0], squared=True, _backend=be)
    assert d2.shape == M.BASE and float(d2[4, 3, 65]) == 0.0 and float(d2[0, 0, 0]) == 16 + 9 + 65 * 65
    d = metrics.distance_to(single, sampling=(2, 0.5, 1.25), _backend=be)
    assert abs(float(d[0, 0, 0, 0]) - math.sqrt(64 + 2.25 + (65 * 1.25) ** 2)) <= 1e-4
    assert bool(torch.isinf(metrics.distance_to(CASES["empty"], _backend=be)).all())
    both = metrics.distance_to(CASES["no_sites_beside_sites"], squared=True, _backend=be)
    assert bool(torch.isinf(both[0]).all()) and bool(torch.isfinite(both[1]).all())
    # scipy's meaning: 0 on the background, the distance to the background inside
    box = metrics.distance_transform_edt(CASES["box_at_border"], _backend=be)
    assert float(box[0, 7, 0, 0]) == 0.0 and float(box[0, 0, 9, 69]) == 5.0 and float(box[0, 4, 9, 69]) == 1.0
    with pytest.raises(RuntimeError, match="MI355X"):
        metrics.distance_transform_edt(CASES["full"])
    with pytest.raises(RuntimeError, match="MI355X"):
        metrics.evaluate(CASES["full"], CASES["full"])


# ---- surface distances ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", M.SPACINGS, ids=M.ids)
@pytest.mark.parametrize("dhw", M.EXTENTS, ids=M.ids)
def test_surface_distances_of_random_masks(emu_backend, dhw, spacing):
    for key, pred, truth in _random_cases(dhw):
        M.check_surface(emu_backend, metrics, pred, truth, spacing, M.PERCENTILES, key)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_surface_distances_of_small_edge_sets(emu_backend, name):
    pred, truth = PAIRS[name]
    for sp in M.SPACINGS:
        s = M.check_surface(emu_backend, metrics, pred, truth, sp, M.PERCENTILES, name)
        M.check_surface(emu_backend, metrics, truth, pred, sp, M.PERCENTILES, name + "_swapped")
        assert int(s.edge_counts[0, 0]) == int(name.split("_")[1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_surface_distances_of_the_constructed_masks(emu_backend, name):
    be, mask = emu_backend, CASES[name]
    other = torch.roll(mask, 2, dims=2)
    for sp in M.SPACINGS:
        M.check_surface(be, metrics, mask, other, sp, 95, name)
        s = metrics.surface_distances(mask, mask, spacing=sp, _backend=be)           # equal masks: 0 for all three, Dice 1
        assert float(s.hausdorff.abs().max()) == 0 and float(s.hausdorff_percentile.abs().max()) == 0
        assert float(s.average_surface_distance.abs().max()) == 0 and float(s.directed.abs().max()) == 0
    assert metrics.dice_score(mask, mask, _backend=be).tolist() == [1.0] * mask.shape[0]


def test_empty_set_rules_and_a_shifted_mask(emu_backend):
    be = emu_backend
    empty, box = CASES["empty"][:1], CASES["hollow_shell"]
    s = metrics.surface_distances(empty, empty, _backend=be)
    assert s.hausdorff.tolist() == [0.0] and s.hausdorff_percentile.tolist() == [0.0] and s.average_surface_distance.tolist() == [0.0]
    assert s.directed.tolist() == [[0.0] * 5] and s.edge_counts.tolist() == [[0, 0]]
    for a, b in ((empty, box), (box, empty)):
        s = metrics.surface_distances(a, b, _backend=be)
        assert bool(torch.isinf(s.hausdorff).all() and torch.isinf(s.hausdorff_percentile).all() and torch.isinf(s.directed).all())
        assert bool(torch.isinf(s.average_surface_distance).all()) and int(s.edge_counts.min()) == 0 and int(s.edge_counts.max()) > 0
    # one channel empty on both sides beside one that is not
    two = torch.cat([empty, box])
    s = metrics.surface_distances(two, torch.roll(two, 1, dims=1), _backend=be)
    assert float(s.hausdorff[0]) == 0.0 and float(s.hausdorff[1]) == 1.0
    M.check_shift(be, metrics)


def test_evaluate_is_the_composition_of_its_parts(emu_backend):
    be = emu_backend
    p = M.CK.probabilities(3, 2, (9, 10, 70), seed=4)
    truth = M.random_mask(2, (9, 10, 70), 0.4, 9)
    _, mask = prepost.finish_prediction(p, _backend=be)
    ev = metrics.evaluate(mask, truth, (1, 1, 3), percentile=95.0, _backend=be)
    s = metrics.surface_distances(mask, truth, (1, 1, 3), 95.0, _backend=be)
    assert torch.equal(ev.counts, metrics.confusion_counts(mask, truth, _backend=be))
    for name in ("dice_score", "iou", "sensitivity", "precision"):
        assert torch.equal(getattr(ev, name.replace("_score", "")), getattr(metrics, name)(mask, truth, _backend=be))
    for name in s._fields:
        assert torch.equal(getattr(ev, name), getattr(s, name)), name
    with pytest.raises(ValueError):
        metrics.evaluate(mask, truth[:1], _backend=be)


# ---- hostile memory ------------------------------------------------------------------------------------------------------------------------
def _hostile_inputs():
    pred, truth = M.random_mask(2, (5, 6, 2 * M.LINE_CHUNK + 7), 0.3, 3), M.random_mask(2, (5, 6, 2 * M.LINE_CHUNK + 7), 0.25, 4)
    return pred, truth


HOSTILE = {
    "seg_counts": lambda be, p, t: be.seg_counts(p, t),
    "mask_edges": lambda be, p, t: be.mask_edges(p),
    "edt": lambda be, p, t: (be.edt(p, (2, 0.5, 1.25), sqrt=False), be.edt(t, (1, 1, 1), invert=True, sqrt=True)),
    "surface_stats": lambda be, p, t: metrics.surface_distances(p, t, (1, 1, 3), 50.0, _backend=be),
    "evaluate": lambda be, p, t: metrics.evaluate(p, t, (1, 1, 1), _backend=be),
}


def hold_op(be, name):
    """scratch_guard.hold: clean twice (same bits), then with every `empty` tensor pre-filled with QNAN and with ONES inside guard
    bands: same bits again, every guard byte untouched."""
    pred, truth = (t.to(be.device) for t in _hostile_inputs())
    held = G.hold(be, lambda: HOSTILE[name](be, pred, truth), fills=(G.QNAN, G.ONES), modules=(metrics,))
    assert held.results >= 1 and held.allocations >= 1, held
    return held


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_op_on_hostile_memory(emu_backend, name):
    held = hold_op(emu_backend, name)
    if name == "surface_stats":
        assert held.allocations >= 2 + 4 + 3                 # edges, distance fields and their scratch, statistics + counts + scratch


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(emu_backend):
    lib = emu_backend.lib
    c, d, h, w = 2, 3, 5, 70
    v = d * h * w
    a, b = M.random_mask(c, (d, h, w), 0.3, 1), M.random_mask(c, (d, h, w), 0.3, 2)
    e = torch.zeros_like(a)
    counts = torch.zeros(c, 4, dtype=torch.int32)
    f1, f2 = torch.zeros(c, d, h, w), torch.zeros(c, d, h, w)
    out, n = torch.zeros(c, 8), torch.zeros(c, 2, dtype=torch.int32)
    scratch = torch.zeros(c * _lib.SURFACE_SCRATCH_BYTES // 8, dtype=torch.float64)
    ap, bp, ep, cp, p1, p2, op, np_, sp = (t.data_ptr() for t in (a, b, e, counts, f1, f2, out, n, scratch))
    big = (1, 2048, 1024, 1024)                                # 2^31 voxels: above the cap of mi355_cc_label
    inf, nan = float("inf"), float("nan")

    assert lib.mi355_seg_counts(ap, bp, c, d, h, w, cp, 0) == 0
    for args in ((None, bp, c, d, h, w, cp), (ap, None, c, d, h, w, cp), (ap, bp, c, d, h, w, None), (ap, bp, 0, d, h, w, cp),
                 (ap, bp, c, 0, h, w, cp), (ap, bp, c, d, 0, w, cp), (ap, bp, c, d, h, 0, cp), (ap, bp, *big, cp)):
        assert lib.mi355_seg_counts(*args, 0) == EINVAL, args

    assert lib.mi355_mask_edges(ap, c, d, h, w, ep, 0) == 0
    for args in ((None, c, d, h, w, ep), (ap, c, d, h, w, None), (ap, 0, d, h, w, ep), (ap, c, d, h, -1, ep), (ap, *big, ep)):
        assert lib.mi355_mask_edges(*args, 0) == EINVAL, args

    assert lib.mi355_edt(ap, 0, c, d, h, w, 1.0, 1.0, 1.0, p1, p2, 0) == 0
    for args in ((None, 0, c, d, h, w, 1.0, 1.0, 1.0, p1, p2), (ap, 0, c, d, h, w, 1.0, 1.0, 1.0, None, p2),
                 (ap, 0, c, d, h, w, 1.0, 1.0, 1.0, p1, None), (ap, 0, 0, d, h, w, 1.0, 1.0, 1.0, p1, p2),
                 (ap, 0, c, d, 0, w, 1.0, 1.0, 1.0, p1, p2), (ap, 0, *big, 1.0, 1.0, 1.0, p1, p2),
                 (ap, 0, c, d, h, w, 0.0, 1.0, 1.0, p1, p2), (ap, 0, c, d, h, w, 1.0, -1.0, 1.0, p1, p2),
                 (ap, 0, c, d, h, w, 1.0, 1.0, inf, p1, p2), (ap, 0, c, d, h, w, nan, 1.0, 1.0, p1, p2)):
        assert lib.mi355_edt(*args, 0) == EINVAL, args

    assert lib.mi355_surface_stats(ap, bp, p1, p2, c, v, 95.0, op, np_, sp, 0) == 0
    for args in ((None, bp, p1, p2, c, v, 95.0, op, np_, sp), (ap, None, p1, p2, c, v, 95.0, op, np_, sp),
                 (ap, bp, None, p2, c, v, 95.0, op, np_, sp), (ap, bp, p1, None, c, v, 95.0, op, np_, sp),
                 (ap, bp, p1, p2, c, v, 95.0, None, np_, sp), (ap, bp, p1, p2, c, v, 95.0, op, None, sp),
                 (ap, bp, p1, p2, c, v, 95.0, op, np_, None), (ap, bp, p1, p2, 0, v, 95.0, op, np_, sp),
                 (ap, bp, p1, p2, c, 0, 95.0, op, np_, sp), (ap, bp, p1, p2, c, 2 ** 31 - 1, 95.0, op, np_, sp),
                 (ap, bp, p1, p2, c, v, -0.5, op, np_, sp), (ap, bp, p1, p2, c, v, 100.5, op, np_, sp),
                 (ap, bp, p1, p2, c, v, nan, op, np_, sp)):
        assert lib.mi355_surface_stats(*args, 0) == EINVAL, args
    with pytest.raises(RuntimeError, match="edt"):
        emu_backend.edt(a, (1.0, 0.0, 1.0))


def test_header_signatures_and_launch_counts(emu_backend):
    hdr = open(os.path.join(ROOT, "include", "mi355_unet3d.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.SIGNATURES) and declared == set(_lib.SIGNATURES)
    for name in NEW:
        assert hasattr(emu_backend.lib, name)
    # the scratch of mi355_surface_stats has a published, constant size; nothing new is a size query
    assert int(re.search(r"#define MI355_SURFACE_SCRATCH_BYTES (\d+)", hdr).group(1)) == _lib.SURFACE_SCRATCH_BYTES
    assert not [n for n in NEW if n.endswith(("_workspace", "_blocks"))]
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", "metrics.hip")).read()
    assert int(re.search(r"#define EDT_CHUNK (\d+)", src).group(1)) == M.LINE_CHUNK      # what LONG_EXTENTS are built around
    assert "2^24" in hdr                                                                 # the exactness bound is stated

    fn = emu_backend.lib.emu_take_launches
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]

    def take():
        buf = ctypes.create_string_buffer(4096)
        fn(buf, 4096)
        return buf.value.decode().split()

    seen = []
    for mask in (CASES["empty"][:1], CASES["full"], M.random_mask(1, M.BASE, 0.3, 1)):
        take()
        metrics.evaluate(mask, torch.roll(mask, 1, dims=3), _backend=emu_backend)
        seen.append(take())
    assert seen[0] == seen[1] == seen[2], seen
    assert len(seen[0]) == 2 + 2 * 1 + 2 * 3 + 10, seen[0]     # seg_counts, two mask_edges, two edt, surface_stats


def test_source_has_no_host_round_trip_and_only_integer_atomics():
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", "metrics.hip")).read()
    for word in ("hipMalloc", "hipMemcpy", "Synchronize", "hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipFree"):
        assert word not in src, word
    # every atomic's operand is an int / unsigned / unsigned long long object of this file
    targets = re.findall(r"atomic(?:Add|Max)\(\s*&?\s*([^,]+),", src)
    assert len(targets) >= 8
    for t in targets:
        assert re.match(r"(out \+ \d|S->n\[|S->maxbits\[|S->hist\[|lh\[)", t.strip()), t
