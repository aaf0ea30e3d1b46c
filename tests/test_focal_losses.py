"""HipFocalLoss / HipDiceFocalLoss / HipTverskyLoss (csrc/focal.hip, the Tversky finaliser of csrc/loss_optim.hip) on the CPU emulator of
the same kernel sources, against the torch restatements of tests/focal_cases.py: value and input gradient to 1e-3 relative (fp32 autograd
against double measured ~2e-7 for these formulas), hand-worked values, extreme logits, validation, C ABI errors, launch counts,
registration and hostile memory. tests/test_focal_losses_gpu.py runs the same tables on the HIP library."""
import ctypes
import importlib
import math
import os
import re
import sys
import types

import pytest
import torch

import focal_cases as FC
import op_cases as C
import scratch_guard as G

losses = FC.losses
_lib = importlib.import_module("3dunetcnn_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
NEW = {"mi355_focal_fwd_bwd", "mi355_tversky_forward", "mi355_tversky_backward"}
DHW = (9, 8, 10)


@pytest.mark.parametrize("name,mk,ref,c", FC.CASES, ids=FC.IDS)
def test_parity_on_emulator(emu_backend, name, mk, ref, c):
    FC.check(mk(), ref, emu_backend, "cpu", 2, c, DHW, name)


def test_tversky_none_on_emulator(emu_backend):
    loss, _ = FC.check_none(FC.NONE_KW, emu_backend, "cpu", 2, 3, DHW)
    assert loss.shape == (2, 3, 1, 1, 1)
    loss, _ = FC.check_none(dict(FC.NONE_KW, batch=True, include_background=False), emu_backend, "cpu", 2, 3, DHW)
    assert loss.shape == (2, 1, 1, 1)


def test_tversky_half_half_is_dice(emu_backend):
    """alpha = beta = 0.5: 1 - (I + s) / (P/2 + Y/2 + s) = 1 - (2I + 2s) / (P + Y + 2s): Dice with twice the smoothing -- exactly; with the
    same smoothing on both sides the two differ by ~s / (P + Y) ~ 1e-8 at these sums."""
    z, t = FC.data(2, 3, DHW)
    for dice_smooth in (2e-5, 1e-5):
        tv, dc = losses.HipTverskyLoss(sigmoid=True), losses.HipDiceLoss(sigmoid=True, smooth_nr=dice_smooth, smooth_dr=dice_smooth)
        tv._be = dc._be = emu_backend
        a, b = float(tv(z, t)), float(dc(z, t))
        assert abs(a - b) / abs(b) < 1e-6, (a, b)


# ---- hand-worked values: two voxels, independent of the restatement -----------------------------------------------------------------------
def _two_voxels(be, crit, z, y):
    """z, y: per-channel values; both voxels carry the same ones, so the mean over voxels is the per-voxel value"""
    crit._be = be
    zt = torch.tensor(z, dtype=torch.float32).view(1, -1, 1, 1, 1).repeat(1, 1, 1, 1, 2)
    yt = torch.tensor(y, dtype=torch.float32).view(1, -1, 1, 1, 1).repeat(1, 1, 1, 1, 2)
    return float(crit(zt, yt))


def test_hand_worked_values(emu_backend):
    be, ln3 = emu_backend, math.log(3.0)
    for (z, y), plain, alpha in (((0.0, 1.0), 0.17328680, 0.04332170), ((ln3, 1.0), 0.01798013, 0.00449503), ((ln3, 0.0), 0.77979058, 0.58484293)):
        assert abs(_two_voxels(be, losses.HipFocalLoss(gamma=2.0), [z], [y]) - plain) < 2e-7
        assert abs(_two_voxels(be, losses.HipFocalLoss(gamma=2.0, alpha=0.25), [z], [y]) - alpha) < 2e-7
    # softmax form: p = (1, 2, 5) / 8, class 1: 0.75^2 * ln 4 = 0.77979058 in one of three channels
    got = _two_voxels(be, losses.HipFocalLoss(gamma=2.0, use_softmax=True), [0.0, math.log(2.0), math.log(5.0)], [0.0, 1.0, 0.0])
    assert abs(got - 0.25993019) < 2e-7
    assert abs(3.0 * got - 0.77979058) < 6e-7
    # Tversky on probabilities: one channel, voxels p = (0.75, 0.5), y = (1, 0): tp 0.75, fp 0.5, fn 0.25
    crit = losses.HipTverskyLoss(alpha=0.3, beta=0.7, smooth_nr=1e-5, smooth_dr=1e-5)
    crit._be = be
    got = float(crit(torch.tensor([0.75, 0.5]).view(1, 1, 1, 1, 2), torch.tensor([1.0, 0.0]).view(1, 1, 1, 1, 2)))
    assert abs(got - 0.30232277) < 2e-7


# ---- extreme logits --------------------------------------------------------------------------------------------------------------------------
ZS = [-80.0, -30.0, 0.0, 30.0, 80.0]


@pytest.mark.parametrize("kw", [dict(gamma=2.0), dict(gamma=0.5, alpha=0.25), dict(gamma=0.0)], ids=["g2", "g0.5_alpha", "g0"])
def test_extreme_logits_sigmoid(emu_backend, kw):
    z = torch.tensor(ZS).repeat(2).view(1, 1, 1, 2, 5)
    y = torch.tensor([0.0] * 5 + [1.0] * 5).view(1, 1, 1, 2, 5)
    zr = z.double().requires_grad_(True)
    ref = FC.focal_loss(zr, y.double(), **kw)
    ref.backward()
    crit = losses.HipFocalLoss(**kw)
    crit._be = emu_backend
    zg = z.clone().requires_grad_(True)
    loss = crit(zg, y)
    loss.backward()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(zg.grad).all())
    assert abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach()) < FC.TOL
    assert C.rel_err(zg.grad, zr.grad) < FC.TOL


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_extreme_logits_softmax(emu_backend, gamma):
    """Two channels, z = (z0, 0): at |z0| >= 30 the winning probability rounds to exactly 1 in fp32 (at 80 in double too, where autograd of
    the restatement's pow gives 0 * inf = NaN for gamma < 1, whichever class is labelled). The kernel gives a finite value, finite
    gradients, a ZERO gradient where the winner is the labelled class, and matches the restatement wherever that is finite."""
    z0 = torch.tensor(ZS).repeat(2).view(1, 1, 1, 2, 5)
    z = torch.cat([z0, torch.zeros_like(z0)], 1)
    lab = torch.tensor([0] * 5 + [1] * 5).view(1, 1, 1, 2, 5)
    zr = z.double().requires_grad_(True)
    ref = FC.focal_loss(zr, lab, gamma=gamma, use_softmax=True, to_onehot_y=True)
    ref.backward()
    crit = losses.HipFocalLoss(gamma=gamma, use_softmax=True, to_onehot_y=True)
    crit._be = emu_backend
    zg = z.clone().requires_grad_(True)
    loss = crit(zg, lab)
    loss.backward()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(zg.grad).all())
    assert abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach()) < FC.TOL
    winner_labelled = ((z0 >= 30) & (lab == 0)) | ((z0 <= -30) & (lab == 1))                # [1, 1, 1, 2, 5]
    assert int(winner_labelled.sum()) == 4
    assert bool((zg.grad[winner_labelled.expand_as(z)] == 0).all())
    ok = torch.isfinite(zr.grad)
    assert bool(ok[(z0.abs() < 80).expand_as(z)].all()) and (gamma < 1 or bool(ok.all()))
    assert C.rel_err(torch.where(ok, zg.grad.double(), 0.0), torch.where(ok, zr.grad, 0.0)) < FC.TOL


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
def test_constructor_validation():
    for cls in (losses.HipDiceFocalLoss, losses.HipTverskyLoss):
        with pytest.raises(ValueError, match="Incompatible values"):
            cls(sigmoid=True, softmax=True)
        with pytest.raises(TypeError, match="other_act must be None or callable"):
            cls(other_act=3)
        with pytest.raises(NotImplementedError, match="other_act"):
            cls(other_act=torch.tanh)
        with pytest.raises(ValueError, match="Unsupported reduction"):
            cls(reduction="median")
    for cls in (losses.HipFocalLoss, losses.HipDiceFocalLoss):
        with pytest.raises(ValueError, match="gamma"):
            cls(gamma=-0.5)
        with pytest.raises(ValueError, match="gamma"):
            cls(gamma=float("nan"))
        for a in (-0.1, 1.5):
            with pytest.raises(ValueError, match="alpha"):
                cls(alpha=a)
        with pytest.raises(NotImplementedError, match="reduction"):
            cls(reduction="none")
        with pytest.raises(ValueError, match="no less than 0"):
            cls(weight=[1.0, -2.0, 1.0])
    with pytest.raises(ValueError, match="no less than 0.0"):
        losses.HipDiceFocalLoss(lambda_dice=-1.0)
    with pytest.raises(ValueError, match="no less than 0.0"):
        losses.HipDiceFocalLoss(lambda_focal=-1.0)
    with pytest.raises(ValueError, match="both 0"):
        losses.HipDiceFocalLoss(lambda_dice=0.0, lambda_focal=0.0)
    assert losses.HipTverskyLoss(reduction="none").reduction == "none"


def test_forward_validation():
    z, t = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4)
    for cls in (losses.HipFocalLoss, losses.HipDiceFocalLoss):
        crit = cls(weight=[1.0, 2.0])
        crit._be = object()                                  # the checks below run before any kernel
        with pytest.raises(ValueError, match="length of the `weight` sequence"):
            crit(z, t)
        crit = cls(weight=[1.0, 2.0, 3.0], include_background=False)       # counted classes: 2
        crit._be = object()
        with pytest.raises(ValueError, match="length of the `weight` sequence"):
            crit(z, t)
        crit = cls(weight=[1.0, 2.0, 1.0])
        crit._be = object()
        crit.class_weight[2] = -0.5                          # a weight written after construction is checked as well
        with pytest.raises(ValueError, match="no less than 0"):
            crit(z, t)
    for cls in (losses.HipFocalLoss, losses.HipDiceFocalLoss, losses.HipTverskyLoss):
        crit = cls()
        crit._be = object()
        with pytest.raises(NotImplementedError, match="more than 16 classes"):
            crit(torch.zeros(1, 17, 2, 2, 2), torch.zeros(1, 17, 2, 2, 2))
        with pytest.raises(AssertionError, match="different shape"):
            crit(z, torch.zeros(1, 2, 4, 4, 4))
        crit = cls(to_onehot_y=True)
        crit._be = object()
        with pytest.raises(AssertionError, match="channel with length equal to one"):
            crit(z, t)
        crit = cls(include_background=False)
        crit._be = object()
        with pytest.raises(ValueError, match="include_background"):
            crit(torch.zeros(1, 1, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2))
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="MI355X only"):
                cls()(z, t)


def test_existing_modules_are_not_widened():
    with pytest.raises(NotImplementedError, match="weight"):
        losses.HipDiceCELoss(softmax=True, weight=[1.0, 2.0])
    with pytest.raises(NotImplementedError, match="reduction"):
        losses.HipDiceCELoss(sigmoid=True, reduction="none")
    with pytest.raises(NotImplementedError):
        losses.HipBCEWithLogitsLoss(pos_weight=torch.ones(3))
    with pytest.raises(NotImplementedError):
        losses.HipCrossEntropyLoss(label_smoothing=0.1)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments(emu_backend):
    lib = emu_backend.lib
    z = torch.zeros(1, 3, 4, 4, 4)
    f = torch.zeros(4096)
    zp, fp = z.data_ptr(), f.data_ptr()

    def fo(**kw):
        base = dict(mode=0, target_kind=0, include_background=1, reduction=0, has_alpha=0, gamma=2.0, alpha=0.0, class_weight=None)
        base.update(kw)
        return ctypes.byref(_lib.MiFocalOpts(**base))

    def focal(o, logits=zp, target=zp, n=1, c=3, v=64, loss=fp, ws=fp, ws_bytes=16384):
        return lib.mi355_focal_fwd_bwd(o, logits, target, n, c, v, 1.0, loss, 0, None, 0, 1.0, ws, ws_bytes, 0)
    assert focal(fo()) == 0 and focal(fo(mode=1, has_alpha=1, alpha=1.0, gamma=0.0)) == 0
    assert focal(fo(), ws_bytes=_lib.FOCAL_SCRATCH_BYTES) == 0
    for bad in (dict(logits=None), dict(target=None), dict(loss=None), dict(ws=None), dict(n=0), dict(c=0), dict(v=0), dict(v=-3)):
        assert focal(fo(), **bad) == EINVAL, bad
    assert focal(None) == EINVAL
    for bad in (dict(mode=2), dict(mode=-1), dict(target_kind=3), dict(target_kind=-1), dict(reduction=2), dict(gamma=-1.0),
                dict(gamma=float("nan")), dict(has_alpha=1, alpha=-0.1), dict(has_alpha=1, alpha=1.1), dict(has_alpha=1, alpha=float("nan"))):
        assert focal(fo(**bad)) == EINVAL, bad
    assert focal(fo(include_background=0), c=1) == EINVAL
    assert focal(fo(), c=17) == EUNSUPPORTED
    assert focal(fo(), ws_bytes=_lib.FOCAL_SCRATCH_BYTES - 4) == EWORKSPACE

    def to(**kw):
        base = dict(activation=1, target_kind=0, batch=0, include_background=1, reduction=0, alpha=0.3, beta=0.7, smooth_nr=1e-5, smooth_dr=1e-5)
        base.update(kw)
        return ctypes.byref(_lib.MiTverskyOpts(**base))
    tf, tb = lib.mi355_tversky_forward, lib.mi355_tversky_backward
    need = lib.mi355_dice_workspace(1, 3, 64)
    dz = torch.zeros_like(z)
    assert tf(to(), zp, zp, 1, 3, 64, fp, fp, need, 0) == 0
    assert tb(to(), zp, zp, 1, 3, 64, None, 0, dz.data_ptr(), fp, 0) == 0
    for bad in (dict(activation=3), dict(target_kind=5), dict(reduction=3), dict(alpha=float("nan")), dict(beta=float("nan"))):
        assert tf(to(**bad), zp, zp, 1, 3, 64, fp, fp, need, 0) == EINVAL, bad
        assert tb(to(**bad), zp, zp, 1, 3, 64, None, 0, zp, fp, 0) == EINVAL, bad
    for args in ((None, zp, 1, 3, 64, fp, fp), (zp, None, 1, 3, 64, fp, fp), (zp, zp, 1, 3, 64, None, fp), (zp, zp, 1, 3, 64, fp, None),
                 (zp, zp, 0, 3, 64, fp, fp), (zp, zp, 1, 0, 64, fp, fp), (zp, zp, 1, 3, 0, fp, fp)):
        assert tf(to(), *args, need, 0) == EINVAL, args
    assert tf(None, zp, zp, 1, 3, 64, fp, fp, need, 0) == EINVAL
    assert tf(to(include_background=0), zp, zp, 1, 1, 64, fp, fp, 16384, 0) == EINVAL
    assert tf(to(), zp, zp, 1, 17, 64, fp, fp, 16384, 0) == EUNSUPPORTED
    assert tf(to(), zp, zp, 1, 3, 64, fp, fp, need - 4, 0) == EWORKSPACE
    assert tb(to(), zp, zp, 1, 3, 64, None, 0, None, fp, 0) == EINVAL
    assert tb(to(), zp, zp, 1, 17, 64, None, 0, zp, fp, 0) == EUNSUPPORTED
    assert tb(to(reduction=2), zp, zp, 1, 3, 64, fp, 2, zp, fp, 0) == EINVAL               # 3 terms, 2 upstream values
    with pytest.raises(RuntimeError, match="focal_fwd_bwd failed"):
        emu_backend.focal(z, z, gamma=-1.0)


def test_header_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "mi355_unet3d.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(_lib.SIGNATURES) and declared == set(_lib.SIGNATURES)
    assert not [n for n in NEW if n.endswith(("_workspace", "_blocks"))]
    assert int(re.search(r"#define MI355_FOCAL_SCRATCH_BYTES (\d+)", hdr).group(1)) == _lib.FOCAL_SCRATCH_BYTES
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", "focal.hip")).read()
    assert int(re.search(r"#define FOCAL_BLOCKS (\d+)", src).group(1)) * 4 == _lib.FOCAL_SCRATCH_BYTES
    assert not re.search(r"atomic\w*\s*\(", src)                              # block partials + a one-block finaliser: the same bits on every call
    # the opts structures as the compiler lays them out: 5 ints + 2 floats, then the pointer on its own 8-byte boundary; 5 ints + 4 floats
    assert ctypes.sizeof(_lib.MiFocalOpts) == 40 and _lib.MiFocalOpts.class_weight.offset == 32
    assert ctypes.sizeof(_lib.MiTverskyOpts) == 36


# ---- launch counts -------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(emu_backend):
    fn = emu_backend.lib.emu_take_launches
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]

    def take():
        buf = ctypes.create_string_buffer(4096)
        fn(buf, 4096)
        return [k for k in buf.value.decode().split("\n") if k]

    def run(crit, t):
        crit._be = emu_backend
        z = torch.randn(2, 3, 6, 5, 7, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
        take()
        crit(z, t).backward()
        return take()
    empty, full = torch.zeros(2, 3, 6, 5, 7, dtype=torch.uint8), torch.ones(2, 3, 6, 5, 7, dtype=torch.uint8)
    labels = torch.randint(0, 3, (2, 1, 6, 5, 7), generator=torch.Generator().manual_seed(2))
    seen = [run(losses.HipFocalLoss(), t) for t in (empty, full)]
    assert seen[0] == seen[1] == ["(focal_kernel<0>)", "loss_finalize_kernel"], seen
    assert run(losses.HipFocalLoss(use_softmax=True, to_onehot_y=True), labels) == ["(focal_kernel<1>)", "loss_finalize_kernel"]      # label maps are read as they are
    is_ce = lambda k: k == "loss_finalize_kernel" or k.startswith("(ce_kernel<")
    is_focal = lambda k: k == "loss_finalize_kernel" or k.startswith("(focal_kernel<")
    masked = lambda ks, hit: ["*" if hit(k) else k for k in ks]
    for kw, t in ((dict(sigmoid=True), empty), (dict(sigmoid=True), full), (dict(sigmoid=True, jaccard=True, reduction="sum"), full),
                  (dict(softmax=True, to_onehot_y=True), labels)):
        ce, fo = run(losses.HipDiceCELoss(**kw), t), run(losses.HipDiceFocalLoss(**kw), t)
        assert sum(map(is_ce, ce)) == 2 and sum(map(is_focal, fo)) == 2 and masked(fo, is_focal) == masked(ce, is_ce), (kw, ce, fo)
    tv = [run(losses.HipTverskyLoss(sigmoid=True), t) for t in (empty, full)]
    assert tv[0] == tv[1] == ["dice_ex_partial_kernel", "tversky_finalize_kernel", "dice_ex_grad_kernel"], tv
    fused = ["dice_partial_kernel", "dice_finalize_kernel", "dice_grad_kernel"]
    assert run(losses.HipDiceLoss(sigmoid=True), full) == fused                                    # the training step's loss: one call
    assert run(losses.HipGeneralizedDiceLoss(sigmoid=True), full) == fused
    assert run(losses.HipDiceLoss(softmax=True), full) == ["dice_ex_partial_kernel", "dice_finalize_kernel", "dice_ex_grad_kernel"]
    assert run(losses.HipCrossEntropyLoss(), labels) == ["one_hot_kernel", "one_hot_kernel", "(ce_kernel<unsigned char>)", "loss_finalize_kernel"]


# ---- registration --------------------------------------------------------------------------------------------------------------------------
def test_register_publishes_the_losses(monkeypatch):
    """the reference resolves config["loss"]["name"] through unet3d.losses first: a stub of that module stands in for the reference"""
    register = importlib.import_module("3dunetcnn_amd.register").register
    pkg, stub = types.ModuleType("unet3d"), types.ModuleType("unet3d.losses")
    pkg.__path__ = []
    pkg.losses = stub
    monkeypatch.setitem(sys.modules, "unet3d", pkg)
    monkeypatch.setitem(sys.modules, "unet3d.losses", stub)
    had_adam = hasattr(torch.optim, "HipAdam")
    try:
        done = register()
        for name in ("HipFocalLoss", "HipDiceFocalLoss", "HipTverskyLoss"):
            assert getattr(stub, name) is getattr(losses, name) and name in done["losses"]
        assert not hasattr(stub, "FocalLoss")
        done = register(replace=True)
        for name in ("FocalLoss", "DiceFocalLoss", "TverskyLoss"):
            assert getattr(stub, name) is getattr(losses, "Hip" + name) and name in done["losses"]
        assert stub.DiceLoss is losses.HipDiceLoss             # the earlier names still resolve
        crit = stub.DiceFocalLoss(**{"include_background": False, "sigmoid": True, "gamma": 2.0, "lambda_focal": 0.5})   # a config block
        assert isinstance(crit, losses.HipDiceFocalLoss) and crit.lambda_focal == 0.5
    finally:
        if not had_adam and hasattr(torch.optim, "HipAdam"):
            del torch.optim.HipAdam


# ---- hostile memory ------------------------------------------------------------------------------------------------------------------------
ROWS = FC.rows(DHW)


@pytest.mark.parametrize("rid", sorted(ROWS))
def test_on_hostile_memory(emu_backend, rid):
    case, fills = ROWS[rid]
    assert G.hold(emu_backend, lambda: case(emu_backend), fills).results > 0
