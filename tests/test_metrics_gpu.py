"""The cases of tests/test_metrics.py through the HIP library on an MI355X, against the same oracles (tests/metrics_cases.py), plus one
3 x 48 x 56 x 70 pair of random blobs so that every launch has many workgroups in flight: integer atomics from all XCDs, hundreds of
line bundles, a thousand partial sums. Hostile memory as on the emulator: poisoned, guarded scratch and outputs, identical bits."""
import importlib

import pytest
import torch

import metrics_cases as M
import test_metrics as T

metrics = importlib.import_module("3dunetcnn_amd.metrics")
pytestmark = pytest.mark.gpu
CASES, PAIRS = T.CASES, T.PAIRS


@pytest.mark.parametrize("dhw", M.EXTENTS, ids=M.ids)
def test_random_masks_match_the_oracles(hip_backend, dhw):
    be = hip_backend
    for key, pred, truth in M.random_cases(dhw):
        M.check_counts(be, metrics, pred, truth)
        M.check_edges(be, metrics, pred)
        M.check_edt_unit(be, metrics, pred, key)
        for sp in M.SPACINGS[1:]:
            M.check_edt_spacing(be, metrics, pred, sp, key)
        for sp in M.SPACINGS:
            M.check_surface(be, metrics, pred, truth, sp, M.PERCENTILES, key)


def test_constructed_masks_match_the_oracles(hip_backend):
    be = hip_backend
    for name in sorted(CASES):
        mask = CASES[name]
        M.check_counts(be, metrics, mask, torch.roll(mask, 1, dims=3))
        M.check_edges(be, metrics, mask)
        M.check_edt_unit(be, metrics, mask, name)
        for sp in M.SPACINGS[1:]:
            M.check_edt_spacing(be, metrics, mask, sp, name)
        other = torch.roll(mask, 2, dims=2)
        for sp in M.SPACINGS:
            M.check_surface(be, metrics, mask, other, sp, 95, name)
            s = metrics.surface_distances(mask.cuda(), mask.cuda(), spacing=sp)
            assert float(s.hausdorff.abs().max()) == 0 and float(s.hausdorff_percentile.abs().max()) == 0
            assert float(s.average_surface_distance.abs().max()) == 0
        assert metrics.dice_score(mask.cuda(), mask.cuda()).tolist() == [1.0] * mask.shape[0]


def test_small_edge_sets(hip_backend):
    for name in sorted(PAIRS):
        pred, truth = PAIRS[name]
        for sp in M.SPACINGS:
            M.check_surface(hip_backend, metrics, pred, truth, sp, M.PERCENTILES, name)
            M.check_surface(hip_backend, metrics, truth, pred, sp, M.PERCENTILES, name + "_swapped")


def test_empty_set_rules_and_a_shifted_mask(hip_backend):
    empty, box = CASES["empty"][:1].cuda(), CASES["hollow_shell"].cuda()
    s = metrics.surface_distances(empty, empty)
    assert s.hausdorff.tolist() == [0.0] and s.directed.tolist() == [[0.0] * 5] and s.edge_counts.tolist() == [[0, 0]]
    for a, b in ((empty, box), (box, empty)):
        s = metrics.surface_distances(a, b)
        assert bool(torch.isinf(s.hausdorff).all() and torch.isinf(s.hausdorff_percentile).all() and torch.isinf(s.directed).all())
        assert bool(torch.isinf(s.average_surface_distance).all())
    M.check_shift(hip_backend, metrics)


def test_blobs_with_many_workgroups_per_launch(hip_backend):
    be = hip_backend
    pred, truth = M.blob_pair(3, (48, 56, 70), seed=5)
    M.check_counts(be, metrics, pred, truth)
    M.check_edges(be, metrics, pred)
    M.check_edt_unit(be, metrics, pred, "blobs")
    M.check_edt_spacing(be, metrics, truth, (2, 0.5, 1.25), "blobs_truth")
    first = M.check_surface(be, metrics, pred, truth, (1, 1, 3), 95, "blobs")
    again = metrics.evaluate(pred.cuda(), truth.cuda(), (1, 1, 3), 95.0)
    for name in first._fields:                                # identical bits on a second call
        assert torch.equal(getattr(again, name), getattr(first, name)), name


@pytest.mark.parametrize("name", sorted(T.HOSTILE))
def test_op_on_hostile_memory(hip_backend, name):
    T.hold_op(hip_backend, name)
