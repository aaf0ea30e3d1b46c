"""mi355_augment_batch on the CPU emulator (the kernels' index logic without a GPU): the oracle of tests/augment_cases.py pinned to
torch, then exact transforms, interpolating transforms, labels, determinism and the ABI's error codes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import augment_cases as A

EINVAL, EWORKSPACE = -1, -4


def test_oracle_matches_grid_sample_and_flip():
    """The oracle itself: against F.grid_sample(align_corners=True) on the voxel grid, both paddings, trilinear and nearest (away from
    ties), and against torch.flip / slicing for the exact maps."""
    dhw = (9, 8, 11)
    img, lab = A.make_batch(2, 3, 2, dhw, torch.float32, 5)
    for ms in A.interp_maps(dhw, 2)[:4]:
        m = A.as_m(ms)
        for padding in ("border", "zeros"):
            want, wlab, ties = A.oracle(img, lab, m, None, None, dhw, padding, False)
            for s in range(2):
                co = A.source_coords(m[s], dhw)
                norm = lambda c, n: 2.0 * c / max(n - 1, 1) - 1.0
                grid = torch.stack([norm(co[..., 2], dhw[2]), norm(co[..., 1], dhw[1]), norm(co[..., 0], dhw[0])], dim=-1)[None]
                ref = F.grid_sample(img[s][None].double(), grid, mode="bilinear", padding_mode=padding, align_corners=True)[0]
                assert float((want[s] - ref).abs().max()) < 1e-9 * float(ref.abs().max())
                refl = F.grid_sample(lab[s][None].double(), grid, mode="nearest", padding_mode=padding, align_corners=True)[0]
                keep = ~ties[s][None].expand_as(refl)
                assert torch.equal(wlab[s].double()[keep], refl[keep])
    for name, m4, out_shape, ref in A.exact_cases(dhw):
        want, wlab, ties = A.oracle(img, lab, A.as_m([m4, m4]), None, None, out_shape, "border", False)
        assert torch.equal(want.float(), ref(img)) and torch.equal(wlab, ref(lab)) and not bool(ties.any()), name
    x = torch.randn(1, 2, *dhw, dtype=torch.float64) * 3 + 40
    want, _, _ = A.oracle(x, None, A.as_m([A.eye()]), torch.tensor([[2.0, 0.5]]), torch.tensor([[0.25, -1.0]]), dhw, "border", True)
    z = (x - x.mean(dim=(2, 3, 4), keepdim=True)) / x.std(dim=(2, 3, 4), keepdim=True, unbiased=False)
    assert torch.allclose(want, z * torch.tensor([2.0, 0.5]).view(1, 2, 1, 1, 1) + torch.tensor([0.25, -1.0]).view(1, 2, 1, 1, 1), atol=1e-12)


@pytest.mark.parametrize("n,ci,cl,dhw,ldt", [(1, 1, 0, A.EXTENTS[0], None), (2, 4, 3, A.EXTENTS[0], torch.uint8), (3, 5, 1, A.EXTENTS[1], torch.float32),
                                             (2, 3, 2, A.EXTENTS[2], torch.uint8)])
def test_exact_transforms_copy_voxels(emu_backend, n, ci, cl, dhw, ldt):
    A.check_exact(emu_backend, "cpu", n, ci, cl, dhw, ldt, seed=11)


@pytest.mark.parametrize("n,ci,cl,dhw,ldt", [(2, 4, 3, A.EXTENTS[0], torch.uint8), (1, 5, 2, A.EXTENTS[1], torch.float32), (3, 2, 0, A.EXTENTS[1], None),
                                             (2, 1, 1, A.EXTENTS[2], torch.uint8)])
def test_rotation_zoom_and_compositions(emu_backend, n, ci, cl, dhw, ldt):
    A.check_interp(emu_backend, "cpu", n, ci, cl, dhw, ldt, seed=12)


@pytest.mark.parametrize("dhw", A.EXTENTS)
def test_issue_rotations_labels(emu_backend, dhw):
    """The two rotations about the centre on the three small extents: labels equal away from ties, tie share <= 2 %."""
    maps = [[A.rot_map(A.ROTATIONS[0], dhw), A.rot_map(A.ROTATIONS[1], dhw)]]
    A.check_interp(emu_backend, "cpu", 2, 4, 3, dhw, torch.uint8, seed=13, maps=maps)
    A.check_interp(emu_backend, "cpu", 2, 2, 1, dhw, torch.float32, seed=14, maps=maps)


def test_two_calls_give_the_same_bits(emu_backend):
    A.check_deterministic(emu_backend, "cpu", 2, 5, 2, A.EXTENTS[1], seed=15)


def test_python_layer_on_emulator(emu_backend):
    """HipAugmenter end to end with the emulator backend handed in through _be: equals the oracle on the parameters of a twin."""
    kw = dict(spatial_augmentations=[{"name": "RandFlipD", "spatial_axis": 0, "prob": 0.5}, {"name": "RandFlipD", "spatial_axis": 1, "prob": 0.5},
                                     {"name": "RandRotateD", "prob": 1.0, "range_x": 0.2, "range_y": 0.2, "range_z": 0.2},
                                     {"name": "RandZoomD", "prob": 1.0, "min_zoom": 0.9, "max_zoom": 1.1}],
              intensity_augmentations=[{"name": "RandScaleIntensityD", "factors": 0.1, "prob": 1.0}, {"name": "RandShiftIntensityD", "offsets": 0.1, "prob": 1.0}],
              random_crop=(12, 12, 8), normalize=True)
    a = A.aug.HipAugmenter(generator=torch.Generator().manual_seed(3), **kw)
    twin = A.aug.HipAugmenter(generator=torch.Generator().manual_seed(3), **kw)
    a._be = emu_backend
    img, lab = A.make_batch(2, 4, 3, A.EXTENTS[0], torch.uint8, 16)
    got, glab = a(img, lab)
    p = twin.sample_params(2, img.shape[1:])
    assert p.out_shape == (12, 12, 8) and got.shape == (2, 4, 12, 12, 8) and glab.shape == (2, 3, 12, 12, 8)
    want, wlab, ties = A.oracle(img, lab, p.matrices, p.gains, p.offsets, p.out_shape, "border", True)
    assert A.image_err(got, want) <= A.TOL
    keep = ~ties[:, None].expand_as(wlab)
    assert float(ties.float().mean()) <= A.MAX_TIE_SHARE and torch.equal(glab[keep], wlab[keep])


def test_call_refuses_cpu_without_backend():
    with pytest.raises(RuntimeError, match="MI355X"):
        A.aug.HipAugmenter()(torch.zeros(1, 1, 4, 4, 4))


def test_abi_rejects_bad_arguments(emu_backend):
    lib = emu_backend.lib
    n, ci, cl, s, d = 2, 3, 2, (6, 5, 7), (5, 5, 6)
    img, out = torch.zeros(n, ci, *s), torch.full((n, ci, *d), 99.0)
    lab, lout = torch.zeros(n, cl, *s, dtype=torch.uint8), torch.full((n, cl, *d), 9, dtype=torch.uint8)
    m = A.as_m([A.eye()] * n)
    need = lib.mi355_augment_batch_workspace(n, ci, *d)
    assert need > 0 and lib.mi355_augment_batch_workspace(n, ci, 0, 5, 6) == 0
    ws = torch.zeros(need // 4 + 1)

    def call(image=img, o=out, label=lab, lo=lout, ldt=0, n_=n, ci_=ci, cl_=cl, s_=s, d_=d, m_=m, pad=0, norm=1, w=ws, wb=need):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.mi355_augment_batch(p(image), p(o), p(label), p(lo), ldt, n_, ci_, cl_, *s_, *d_, p(m_), None, None, pad, norm, p(w), wb, 0)

    assert call(image=None) == EINVAL and call(o=None) == EINVAL and call(m_=None) == EINVAL
    assert call(lo=None) == EINVAL and call(label=None) == EINVAL                  # label and its output go together
    assert call(d_=(0, 5, 6)) == EINVAL and call(s_=(6, 0, 7)) == EINVAL and call(n_=0) == EINVAL and call(ci_=0) == EINVAL and call(cl_=0) == EINVAL
    assert call(pad=2) == EINVAL and call(pad=-1) == EINVAL and call(ldt=2) == EINVAL
    assert call(wb=need - 4) == EWORKSPACE and call(w=None) == EINVAL
    assert float(out.min()) == 99.0 and int(lout.min()) == 9                       # none of them launched
    assert call() == 0 and float(out.abs().max()) == 0.0 and int(lout.max()) == 0
    assert call(norm=0, w=None, wb=0) == 0                                         # the workspace is needed with normalize only
    with pytest.raises(RuntimeError, match="augment_batch"):
        emu_backend.augment_batch(img, None, m, None, None, (0, 5, 6), "border", False)
