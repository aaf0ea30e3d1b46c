"""DeviceStager(augment=...): the staged batches with and without the on-device augmentation, and a short training loop fed by it."""
import importlib
import math

import pytest
import torch

import augment_cases as A
from oracle import prepost_ref as P

staging = importlib.import_module("3dunetcnn_amd.staging")
ops = importlib.import_module("3dunetcnn_amd.ops")
pytestmark = pytest.mark.gpu
GROUPS = [[1, 2, 4], [1, 4], [4]]
CFG = dict(spatial_augmentations=[{"name": "RandFlipD", "spatial_axis": 0, "prob": 0.5}, {"name": "RandFlipD", "spatial_axis": 1, "prob": 0.5},
                                  {"name": "RandRotateD", "prob": 0.5, "range_x": 0.2, "range_y": 0.2, "range_z": 0.2}],
           intensity_augmentations=[{"name": "RandScaleIntensityD", "factors": 0.1, "prob": 1.0}, {"name": "RandShiftIntensityD", "offsets": 0.1, "prob": 1.0}])


def _batches(n, g, dhw=(12, 10, 14)):
    out = []
    for i in range(n):
        img = torch.randn(2, 4, *dhw, generator=g) * (i + 1) + 3 * i
        lab = torch.randint(0, 5, (2, 1, *dhw), generator=g).float()
        out.append({"image": img, "label": lab, "idx": i})
    return out


def test_stager_without_augment_is_unchanged(hip_backend):
    """augment=None: exactly the un-augmented prologue (per-sample z-score and one-hot of a Backend), as before the keyword existed."""
    data = _batches(3, torch.Generator().manual_seed(1))
    for i, b in enumerate(staging.DeviceStager(data, normalize=True, one_hot_labels=GROUPS)):
        for n in range(2):
            assert torch.equal(b["image"][n], hip_backend.zscore(data[i]["image"][n].cuda().contiguous()))
            assert torch.equal(b["label"][n], hip_backend.one_hot(data[i]["label"][n, 0].cuda().contiguous(), GROUPS))
    for i, b in enumerate(staging.DeviceStager(data)):
        assert torch.equal(b["image"].cpu(), data[i]["image"]) and torch.equal(b["label"].cpu(), data[i]["label"])


def test_identity_augmenter_equals_plain_normalisation(hip_backend):
    data = _batches(3, torch.Generator().manual_seed(2))
    zero = {k: [dict(e, prob=0.0) for e in v] for k, v in CFG.items()}
    a = A.aug.HipAugmenter(normalize=True, **zero)
    plain = list(staging.DeviceStager(data, normalize=True, one_hot_labels=GROUPS))
    for b, ref in zip(staging.DeviceStager(data, one_hot_labels=GROUPS, augment=a), plain):
        assert A.image_err(b["image"].cpu(), ref["image"].cpu().double()) <= A.TOL
        assert b["label"].dtype == torch.uint8 and torch.equal(b["label"], ref["label"]) and b["idx"] == ref["idx"]


def test_seeded_augmenter_equals_oracle_on_twin_parameters(hip_backend):
    data = _batches(4, torch.Generator().manual_seed(3), dhw=(24, 20, 28))
    a = A.aug.HipAugmenter(normalize=True, generator=torch.Generator().manual_seed(9), **CFG)
    twin = A.aug.HipAugmenter(normalize=True, generator=torch.Generator().manual_seed(9), **CFG)
    for i, b in enumerate(staging.DeviceStager(data, one_hot_labels=GROUPS, augment=a)):
        img = data[i]["image"]
        lab = torch.stack([P.compile_one_hot_encoding(data[i]["label"][n:n + 1], 3, labels=GROUPS) for n in range(2)])
        p = twin.sample_params(2, img.shape[1:])
        want, wlab, ties = A.oracle(img, lab, p.matrices, p.gains, p.offsets, p.out_shape, "border", True)
        assert A.image_err(b["image"].cpu(), want) <= A.TOL, i
        keep = ~ties[:, None].expand_as(wlab)
        assert float(ties.float().mean()) <= A.MAX_TIE_SHARE and torch.equal(b["label"].cpu()[keep], wlab[keep]), i


def test_training_loop_fed_by_the_augmenting_stager(hip_backend):
    unet = importlib.import_module("3dunetcnn_amd.unet")
    losses = importlib.import_module("3dunetcnn_amd.losses")
    optim = importlib.import_module("3dunetcnn_amd.optim")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(4)
    data = _batches(8, g, dhw=(32, 32, 32))
    m = unet.HipUNet3D(n_features=4, n_outputs=3, base_width=16, encoder_blocks=[1, 1, 2]).cuda().train()
    crit, opt = losses.HipDiceLoss(sigmoid=True), optim.HipAdam(m.parameters(), lr=1e-3)
    a = A.aug.HipAugmenter(normalize=True, generator=torch.Generator().manual_seed(5), **CFG)
    steps = 0
    for b in staging.DeviceStager(data, one_hot_labels=GROUPS, augment=a):
        opt.zero_grad(set_to_none=True)
        loss = crit(m(b["image"]), b["label"])
        loss.backward()
        opt.step()
        assert math.isfinite(float(loss.detach()))
        steps += 1
    assert steps == 8
