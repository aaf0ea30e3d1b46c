"""The case table of tests/test_components.py through the HIP library on an MI355X, plus the two real sizes (a 3 x 240 x 240 x 155
BraTS prediction and the 192^3 sppin volume): exact equality with the oracle of tests/components_cases.py, identical bits on a
second run. The workgroups of cc_merge_kernel run on eight XCDs with private L2s here: what the emulator cannot show."""
import importlib

import pytest
import torch

import components_cases as K

prepost = importlib.import_module("3dunetcnn_amd.prepost")
pytestmark = pytest.mark.gpu
CASES = K.constructed_cases()


@pytest.mark.parametrize("k", (1, 3))
def test_random_masks_match_the_oracle(hip_backend, k):
    for dhw in K.EXTENTS:
        for c in (1, 3):
            for i, p in enumerate(K.DENSITIES):
                mask = K.random_mask(c, dhw, p, seed=100 * c + i)
                labels, ref = K.check_labels(hip_backend, mask, k, prepost)
                K.check_filter(hip_backend, mask, k, True, 0, ref, labels)
                K.check_filter(hip_backend, mask, k, False, 3, ref, labels)


@pytest.mark.parametrize("k", (1, 3))
def test_constructed_masks_match_the_oracle(hip_backend, k):
    for name in sorted(CASES):
        labels, ref = K.check_labels(hip_backend, CASES[name], k, prepost)
        K.check_filter(hip_backend, CASES[name], k, True, 0, ref, labels)
    m = CASES["equal_sizes"]
    for min_size, kept in ((0, 11), (2, 10), (5, 10), (6, 0)):
        assert int(K.check_filter(hip_backend, m, k, False, min_size).sum()) == kept
    assert int(prepost.keep_largest_component(CASES["empty"].cuda(), connectivity=k).sum()) == 0


@pytest.mark.parametrize("m", (1, 5))
def test_ensemble_mean_and_threshold(hip_backend, m):
    for dhw in ((5, 6, 8), (3, 5, 7), (40, 48, 56)):
        p = K.probabilities(m, 2, dhw, seed=m)
        ref = p.double().mean(dim=0)
        assert float((ref - 0.5).abs().min()) > 1e-6
        mean, mask = hip_backend.ensemble_threshold(p.cuda(), 0.5)
        assert float((mean.cpu().double() - ref).abs().max()) <= 1e-6
        assert torch.equal(mask.cpu(), (ref >= 0.5).to(torch.uint8))
    if m == 1:
        p = torch.tensor([0.5, 0.49999997, 0.50000006, 0.0, 1.0, 0.5, 0.25, 0.75]).reshape(1, 1, 2, 2, 2)
        assert hip_backend.ensemble_threshold(p.cuda(), 0.5)[1].reshape(-1).tolist() == [1, 0, 1, 0, 1, 1, 0, 1]


@pytest.mark.parametrize("shape", ((3, 240, 240, 155), (1, 192, 192, 192)), ids=("brats", "sppin"))
def test_real_sizes_exact_and_reproducible(hip_backend, shape):
    mask = K.noisy_ellipsoids(shape[0], shape[1:], flip=0.02)
    md = mask.cuda()
    for k in (1, 3):
        labels, count = prepost.connected_components(md, connectivity=k)
        out = prepost.keep_largest_component(md, connectivity=k)
        labels2, _ = prepost.connected_components(md, connectivity=k)
        out2 = prepost.keep_largest_component(md, connectivity=k)
        assert torch.equal(labels, labels2) and torch.equal(out, out2)             # identical bits on a second run
        ref, ref_count = K.oracle_labels(mask, k)
        assert torch.equal(labels.cpu(), ref) and torch.equal(count.cpu(), ref_count)
        assert int(ref_count.min()) > 1000                                         # thousands of islands
        ref_out, ref_stats = K.oracle_filter(mask, ref, True, 0)
        _, stats = hip_backend.cc_filter(md, labels, True, 0)
        assert torch.equal(stats.cpu(), ref_stats) and torch.equal(out.cpu(), ref_out)
        K.check_filter(hip_backend, mask, k, False, 4, ref, labels)


def test_finish_prediction_on_the_device(hip_backend):
    p = K.probabilities(5, 3, (40, 48, 72), seed=3)
    mean, out = prepost.finish_prediction(p.cuda())
    ref_mask = (p.double().mean(dim=0) >= 0.5).to(torch.uint8)
    ref_labels, _ = K.oracle_labels(ref_mask, 1)
    assert float((mean.cpu().double() - p.double().mean(dim=0)).abs().max()) <= 1e-6
    assert torch.equal(out.cpu(), K.oracle_filter(ref_mask, ref_labels, True, 0)[0])
    again = prepost.finish_prediction(list(p.cuda()))
    assert torch.equal(again[0], mean) and torch.equal(again[1], out)
