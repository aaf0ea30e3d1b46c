"""Ensemble mean + threshold, connected components and largest-component cleanup (csrc/components.hip) on the CPU emulator of the same
kernel sources: exact equality with the oracle of tests/components_cases.py (scipy.ndimage.label, or its pinned torch twin)."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import components_cases as K

prepost = importlib.import_module("3dunetcnn_amd.prepost")
_lib = importlib.import_module("3dunetcnn_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -4
CASES = K.constructed_cases()


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("dhw", K.EXTENTS, ids=lambda e: "x".join(map(str, e)))
def test_random_masks_match_the_oracle(emu_backend, dhw, k):
    for c in (1, 3):
        for i, p in enumerate(K.DENSITIES):
            mask = K.random_mask(c, dhw, p, seed=100 * c + i)
            labels, ref = K.check_labels(emu_backend, mask, k, prepost)
            K.check_filter(emu_backend, mask, k, True, 0, ref, labels)
            K.check_filter(emu_backend, mask, k, False, 3, ref, labels)


@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_masks_match_the_oracle(emu_backend, name, k):
    mask = CASES[name]
    labels, ref = K.check_labels(emu_backend, mask, k, prepost)
    K.check_filter(emu_backend, mask, k, True, 0, ref, labels)


def test_torch_reference_is_pinned_to_scipy():
    if not K.have_scipy():
        pytest.skip("scipy absent: the torch reference is the oracle")
    masks = [CASES[n] for n in sorted(CASES)] + [K.random_mask(1, e, p, 7) for e in K.EXTENTS for p in K.DENSITIES]
    for mask in masks:
        for k in (1, 3):
            assert torch.equal(K.torch_labels(mask[0], k), K.scipy_labels(mask[0], k))


def test_what_the_constructed_cases_mean(emu_backend):
    """The expectations written out, independent of the oracle."""
    be = emu_backend

    def count(name, k):
        return int(prepost.connected_components(CASES[name], connectivity=k, _backend=be)[1][0])

    labels, n = prepost.connected_components(CASES["empty"], _backend=be)
    assert n.tolist() == [0, 0] and int(labels.abs().sum()) == 0
    assert int(prepost.keep_largest_component(CASES["empty"], _backend=be).sum()) == 0
    labels, n = prepost.connected_components(CASES["full"], _backend=be)
    assert n.tolist() == [1] and bool((labels == 1).all())
    labels, n = prepost.connected_components(CASES["single_voxel"][0], _backend=be)          # 3-D input: 3-D labels, 0-dim count
    assert labels.shape == CASES["single_voxel"].shape[1:] and n.dim() == 0 and int(n) == 1
    assert int(labels[5, 4, 65]) == 1 + (5 * 6 + 4) * 66 + 65
    assert count("serpentine", 1) == 1 and count("serpentine", 3) == 1
    for name in CASES:
        if name.startswith("face_"):
            assert (count(name, 1), count(name, 3)) == (1, 1), name
        if name.startswith(("edge_", "corner_")):
            assert (count(name, 1), count(name, 3)) == (2, 1), name
    # the tie goes to the component met first in raster order, wherever it sits in the construction order
    for name, first in (("equal_sizes", (1, 1, 3)), ("equal_sizes_late_first", (0, 1, 3))):
        m = CASES[name]
        out = prepost.keep_largest_component(m, _backend=be)
        assert int(out.sum()) == 5 and int(out[0, first[0], first[1], first[2]]) == 1, name
    with pytest.raises(NotImplementedError):
        prepost.connected_components(CASES["full"], connectivity=2, _backend=be)
    with pytest.raises(RuntimeError, match="MI355X"):
        prepost.connected_components(CASES["full"])


def test_min_size_on_both_sides_of_a_size(emu_backend):
    be = emu_backend
    m = CASES["equal_sizes"]                                  # components of 5, 5 and 1 voxels
    for min_size, kept in ((0, 11), (1, 11), (2, 10), (5, 10), (6, 0)):
        out = K.check_filter(be, m, 1, False, min_size)
        assert int(out.sum()) == kept, (min_size, kept)
    for min_size, kept in ((5, 5), (6, 0)):
        assert int(K.check_filter(be, m, 1, True, min_size).sum()) == kept
    mean, out = prepost.finish_prediction(m[None].float(), keep_largest=False, min_size=2, _backend=be)
    assert int(out.sum()) == 10 and torch.equal(mean, m.float())


@pytest.mark.parametrize("m", (1, 5))
def test_ensemble_mean_and_threshold(emu_backend, m):
    be = emu_backend
    for dhw in ((5, 6, 8), (3, 5, 7)):                        # 16-byte path and the scalar one
        p = K.probabilities(m, 2, dhw, seed=m)
        ref = p.double().mean(dim=0)
        assert float((ref - 0.5).abs().min()) > 1e-6          # the precondition of comparing masks exactly
        mean, mask = be.ensemble_threshold(p, 0.5)
        assert mean.dtype == torch.float32 and mask.dtype == torch.uint8
        assert float((mean.double() - ref).abs().max()) <= 1e-6
        assert torch.equal(mask, (ref >= 0.5).to(torch.uint8))
        assert torch.equal(prepost.ensemble_mean(p, _backend=be), mean)
        assert torch.equal(prepost.ensemble_mean(list(p), _backend=be), mean)
    if m == 1:                                                # voxels exactly at the threshold are kept (>=)
        p = torch.tensor([0.5, 0.49999997, 0.50000006, 0.0, 1.0, 0.5, 0.25, 0.75]).reshape(1, 1, 2, 2, 2)
        _, mask = be.ensemble_threshold(p, 0.5)
        assert mask.reshape(-1).tolist() == [1, 0, 1, 0, 1, 1, 0, 1]
        _, mask = be.ensemble_threshold(p.reshape(1, 8)[:, :7].contiguous(), 0.5)
        assert mask.reshape(-1).tolist() == [1, 0, 1, 0, 1, 1, 0]


def test_finish_prediction_is_the_composition_of_its_parts(emu_backend):
    be = emu_backend
    p = K.probabilities(5, 3, (9, 10, 70), seed=11)
    for k in (1, 3):
        mean, out = prepost.finish_prediction(p, threshold=0.5, connectivity=k, _backend=be)
        mean2, mask = be.ensemble_threshold(p, 0.5)
        assert torch.equal(mean, mean2) and torch.equal(mean, prepost.ensemble_mean(p, _backend=be))
        assert torch.equal(out, prepost.keep_largest_component(mask, connectivity=k, _backend=be))
        ref_labels, _ = K.oracle_labels((p.double().mean(dim=0) >= 0.5).to(torch.uint8), k)
        assert torch.equal(out, K.oracle_filter(mask, ref_labels, True, 0)[0])
        again = prepost.finish_prediction(p, threshold=0.5, connectivity=k, _backend=be)
        assert torch.equal(again[0], mean) and torch.equal(again[1], out)          # identical bits on a second call
    mean, out = prepost.finish_prediction(p, keep_largest=False, _backend=be)      # nothing to remove: the thresholded mean
    assert torch.equal(out, (p.double().mean(dim=0) >= 0.5).to(torch.uint8))


def test_abi_rejects_bad_arguments(emu_backend):
    lib = emu_backend.lib
    c, d, h, w = 2, 3, 5, 70
    mask = torch.ones(c, d, h, w, dtype=torch.uint8)
    labels = torch.zeros(c, d, h, w, dtype=torch.int32)
    out = torch.zeros_like(mask)
    need = lib.mi355_cc_workspace(c, d, h, w)
    assert need >= c * d * h * w * 4
    ws = torch.zeros((need + 3) // 4, dtype=torch.float32)
    mp, lp, op, wp = mask.data_ptr(), labels.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert lib.mi355_cc_label(mp, c, d, h, w, 6, lp, 0) == 0
    assert lib.mi355_cc_label(None, c, d, h, w, 6, lp, 0) == EINVAL
    assert lib.mi355_cc_label(mp, c, d, h, w, 6, None, 0) == EINVAL
    assert lib.mi355_cc_label(mp, c, d, h, w, 18, lp, 0) == EINVAL
    assert lib.mi355_cc_label(mp, 0, d, h, w, 6, lp, 0) == EINVAL
    assert lib.mi355_cc_label(mp, 1, 2048, 1024, 1024, 6, lp, 0) == EINVAL          # 2^31 voxels: labels would not fit int32
    assert lib.mi355_cc_workspace(1, 2048, 1024, 1024) == 0
    assert lib.mi355_cc_filter(mp, lp, c, d, h, w, 1, 0, op, None, wp, need, 0) == 0
    assert lib.mi355_cc_filter(mp, lp, c, d, h, w, 1, 0, op, None, wp, need - 4, 0) == EWORKSPACE
    assert lib.mi355_cc_filter(None, lp, c, d, h, w, 1, 0, op, None, wp, need, 0) == EINVAL
    assert lib.mi355_cc_filter(mp, None, c, d, h, w, 1, 0, op, None, wp, need, 0) == EINVAL
    assert lib.mi355_cc_filter(mp, lp, c, d, h, w, 1, 0, None, None, wp, need, 0) == EINVAL
    assert lib.mi355_cc_filter(mp, lp, c, d, h, w, 1, 0, op, None, None, need, 0) == EINVAL
    assert lib.mi355_cc_filter(mp, lp, 1, 2048, 1024, 1024, 1, 0, op, None, wp, need, 0) == EINVAL
    p = torch.rand(2, 16)
    mean = torch.zeros(16)
    assert lib.mi355_ensemble_threshold(p.data_ptr(), 2, 16, 0.5, mean.data_ptr(), None, 0) == 0
    assert lib.mi355_ensemble_threshold(None, 2, 16, 0.5, mean.data_ptr(), None, 0) == EINVAL
    assert lib.mi355_ensemble_threshold(p.data_ptr(), 0, 16, 0.5, mean.data_ptr(), None, 0) == EINVAL
    assert lib.mi355_ensemble_threshold(p.data_ptr(), 2, 0, 0.5, mean.data_ptr(), None, 0) == EINVAL
    assert lib.mi355_ensemble_threshold(p.data_ptr(), 2, 16, 0.5, None, None, 0) == EINVAL
    with pytest.raises(RuntimeError, match="cc_label"):
        _lib.check(lib.mi355_cc_label(mp, c, d, h, w, 18, lp, 0), "cc_label")


def test_header_signatures_and_launch_counts(emu_backend):
    hdr = open(os.path.join(ROOT, "include", "mi355_unet3d.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    new = {"mi355_ensemble_threshold", "mi355_cc_workspace", "mi355_cc_label", "mi355_cc_filter"}
    assert new <= declared and new <= set(_lib.SIGNATURES) and declared == set(_lib.SIGNATURES)
    for name in new:
        assert hasattr(emu_backend.lib, name)
    # a fixed number of launches, whatever the data
    fn = emu_backend.lib.emu_take_launches
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]

    def take():
        buf = ctypes.create_string_buffer(4096)
        fn(buf, 4096)
        return buf.value.decode().split()

    seen = []
    for mask in (CASES["empty"], CASES["serpentine"], K.random_mask(2, (5, 5, 70), 0.31, 1)):
        take()
        labels = emu_backend.cc_label(mask, 26)
        emu_backend.cc_filter(mask, labels, True, 2)
        seen.append(take())
    assert seen[0] == seen[1] == seen[2] and len(seen[0]) == 8, seen


def test_source_has_no_host_round_trip():
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", "components.hip")).read()
    for word in ("hipMalloc", "hipMemcpy", "Synchronize", "hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipFree"):
        assert word not in src, word
