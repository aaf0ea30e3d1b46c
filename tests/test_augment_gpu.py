"""mi355_augment_batch on a real MI355X: the cases of tests/test_augment_emu.py through the HIP library, plus one 128^3 batch-2 case."""
import pytest
import torch

import augment_cases as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,ci,cl,dhw,ldt", [(1, 1, 0, A.EXTENTS[0], None), (2, 4, 3, A.EXTENTS[0], torch.uint8), (3, 5, 1, A.EXTENTS[1], torch.float32),
                                             (2, 3, 2, A.EXTENTS[2], torch.uint8)])
def test_exact_transforms_copy_voxels(hip_backend, n, ci, cl, dhw, ldt):
    A.check_exact(hip_backend, "cuda", n, ci, cl, dhw, ldt, seed=11)


@pytest.mark.parametrize("n,ci,cl,dhw,ldt", [(2, 4, 3, A.EXTENTS[0], torch.uint8), (1, 5, 2, A.EXTENTS[1], torch.float32), (3, 2, 0, A.EXTENTS[1], None),
                                             (2, 1, 1, A.EXTENTS[2], torch.uint8)])
def test_rotation_zoom_and_compositions(hip_backend, n, ci, cl, dhw, ldt):
    A.check_interp(hip_backend, "cuda", n, ci, cl, dhw, ldt, seed=12)


@pytest.mark.parametrize("dhw", A.EXTENTS)
def test_issue_rotations_labels(hip_backend, dhw):
    maps = [[A.rot_map(A.ROTATIONS[0], dhw), A.rot_map(A.ROTATIONS[1], dhw)]]
    A.check_interp(hip_backend, "cuda", 2, 4, 3, dhw, torch.uint8, seed=13, maps=maps)
    A.check_interp(hip_backend, "cuda", 2, 2, 1, dhw, torch.float32, seed=14, maps=maps)


def test_two_calls_give_the_same_bits(hip_backend):
    A.check_deterministic(hip_backend, "cuda", 2, 5, 2, A.EXTENTS[1], seed=15)
    A.check_deterministic(hip_backend, "cuda", 2, 4, 3, (64, 64, 64), seed=16)


def test_128_cubed_batch_2(hip_backend):
    """The flagship input size: flips exactly, rotation + zoom against the oracle, through the statistics, gain and offset."""
    dhw = (128, 128, 128)
    img, lab = A.make_batch(2, 4, 3, dhw, torch.uint8, 17)
    m = A.as_m([A.flip_map(dhw, [0, 1]), A.flip_map(dhw, [2])])
    got, glab = A.run(hip_backend, "cuda", img, lab, m, None, None, dhw, "border", False)
    assert torch.equal(got[0], torch.flip(img[0], [-3, -2])) and torch.equal(got[1], torch.flip(img[1], [-1]))
    assert torch.equal(glab[0], torch.flip(lab[0], [-3, -2])) and torch.equal(glab[1], torch.flip(lab[1], [-1]))
    m = A.as_m([A.rot_map((0.2, 0.2, 0.2), dhw) @ A.zoom_map(1.0931, dhw), A.flip_map(dhw, [0]) @ A.rot_map(A.ROTATIONS[0], dhw)])
    g, o = torch.tensor([[1.05] * 4, [0.93] * 4]), torch.tensor([[0.08] * 4, [-0.04] * 4])
    A.check_against_oracle(hip_backend, "cuda", img, lab, m, g, o, dhw, "border", True, what="128^3")
    A.check_against_oracle(hip_backend, "cuda", img, lab, m, g, o, dhw, "zeros", False, what="128^3 zeros")


def test_python_layer(hip_backend):
    kw = dict(spatial_augmentations=[{"name": "RandFlipD", "spatial_axis": 0, "prob": 0.5}, {"name": "RandRotateD", "prob": 1.0, "range_x": 0.2,
                                                                                              "range_y": 0.2, "range_z": 0.2, "padding_mode": "zeros"}],
              intensity_augmentations=[{"name": "RandScaleIntensityD", "factors": 0.1, "prob": 1.0}], random_crop=(24, 20, 20), normalize=True)
    a = A.aug.HipAugmenter(generator=torch.Generator().manual_seed(3), **kw)
    twin = A.aug.HipAugmenter(generator=torch.Generator().manual_seed(3), **kw)
    img, lab = A.make_batch(3, 4, 3, A.EXTENTS[2], torch.uint8, 18)
    got, glab = a(img.cuda(), lab.cuda())
    p = twin.sample_params(3, img.shape[1:])
    want, wlab, ties = A.oracle(img, lab, p.matrices, p.gains, p.offsets, p.out_shape, "zeros", True)
    assert A.image_err(got.cpu(), want) <= A.TOL
    keep = ~ties[:, None].expand_as(wlab)
    assert float(ties.float().mean()) <= A.MAX_TIE_SHARE and torch.equal(glab.cpu()[keep], wlab[keep])
