"""Loss modules the reference's look-up reaches (unet3d/scripts/script_utils.py:61-77): HipDiceCELoss (monai.losses.DiceCELoss),
HipBCEWithLogitsLoss / HipCrossEntropyLoss (the torch.nn fallback), against plain torch on the CPU. Value and input gradient
to 1e-3 relative (measured ~1e-6)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import op_cases as C
from oracle import torch_ops as O

losses = importlib.import_module("3dunetcnn_amd.losses")
TOL = 1e-3


def _data(n, c, dhw, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, *dhw, generator=g) * 2
    t = C.nested_masks(n, dhw, seed)[:, :c] if c <= 3 else (torch.rand(n, c, *dhw, generator=g) > 0.6).to(torch.uint8)
    return z, t


def _empty(t):
    """Second class empty in sample 0 (infinite generalized-Dice weight -> largest finite weight of the sample)."""
    t = t.clone()
    t[0, 1] = 0
    return t


def _check(crit, ref_fn, be, dev, n, c, dhw, name=""):
    z, t = _data(n, c, dhw)
    if "empty" in name:
        t = _empty(t)
    if "labels" in name:                           # class-index target [N, 1, ...] (to_onehot_y / torch's index form)
        t = torch.randint(0, c, (n, 1) + tuple(dhw), generator=torch.Generator().manual_seed(5))
    zr = z.clone().requires_grad_(True)
    ref = ref_fn(zr, t)
    ref.backward()
    if be is not None:
        crit._be = be
    zg = z.to(dev).requires_grad_(True)
    loss = crit(zg, t.to(dev))
    (loss * 3.0).backward()                     # upstream factor flows through
    assert loss.dim() == 0
    assert abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach())) < TOL
    assert C.rel_err(zg.grad, 3.0 * zr.grad) < TOL


CASES = [
    ("dicece", lambda: losses.HipDiceCELoss(sigmoid=True), lambda z, t: O.dice_loss(z, t, True) + F.cross_entropy(z, t.float()), 3),
    ("dicece_weighted", lambda: losses.HipDiceCELoss(sigmoid=True, lambda_dice=0.3, lambda_ce=2.0, batch=True),
     lambda z, t: 0.3 * O.dice_loss(z, t, True, True) + 2.0 * F.cross_entropy(z, t.float()), 3),
    ("dicece_1ch", lambda: losses.HipDiceCELoss(sigmoid=True), lambda z, t: O.dice_loss(z, t, True) + F.binary_cross_entropy_with_logits(z, t.float()), 1),
    ("dice_nobg", lambda: losses.HipDiceLoss(sigmoid=True, include_background=False), lambda z, t: O.dice_loss(z, t, True, include_background=False), 3),
    ("gdl_doc_config", lambda: losses.HipGeneralizedDiceLoss(include_background=False, sigmoid=True),
     lambda z, t: O.generalized_dice_loss(z, t, True, include_background=False), 4),
    ("gdl_batch", lambda: losses.HipGeneralizedDiceLoss(sigmoid=True, batch=True), lambda z, t: O.generalized_dice_loss(z, t, True, batch=True), 3),
    ("gdl_empty_class", lambda: losses.HipGeneralizedDiceLoss(sigmoid=True), lambda z, t: O.generalized_dice_loss(z, _empty(t), True), 3),
    ("dicece_softmax_labels", lambda: losses.HipDiceCELoss(softmax=True, to_onehot_y=True),
     lambda z, t: O.dice_loss(z, t, False, softmax=True, to_onehot_y=True) + F.cross_entropy(z, t[:, 0]), 4),
    ("dicece_softmax_labels_nobg_weighted", lambda: losses.HipDiceCELoss(softmax=True, to_onehot_y=True, include_background=False,
                                                                          lambda_dice=0.5, lambda_ce=1.5),
     lambda z, t: 0.5 * O.dice_loss(z, t, False, softmax=True, to_onehot_y=True, include_background=False) + 1.5 * F.cross_entropy(z, t[:, 0]), 3),
    ("dicece_jaccard_sum", lambda: losses.HipDiceCELoss(sigmoid=True, jaccard=True, reduction="sum"),
     lambda z, t: O.dice_loss(z, t, True, jaccard=True, reduction="sum") + F.cross_entropy(z, t.float(), reduction="sum"), 3),
    ("dicece_1ch_sum", lambda: losses.HipDiceCELoss(sigmoid=True, reduction="sum"),
     lambda z, t: O.dice_loss(z, t, True, reduction="sum") + F.binary_cross_entropy_with_logits(z, t.float(), reduction="sum"), 1),
    ("ce_labels", lambda: losses.HipCrossEntropyLoss(), lambda z, t: F.cross_entropy(z, t[:, 0]), 5),
    ("bce", lambda: losses.HipBCEWithLogitsLoss(), lambda z, t: F.binary_cross_entropy_with_logits(z, t.float()), 3),
    ("ce", lambda: losses.HipCrossEntropyLoss(), lambda z, t: F.cross_entropy(z, t.float()), 4),
]


@pytest.mark.parametrize("name,mk,ref,c", CASES, ids=[c[0] for c in CASES])
def test_losses_on_emulator(emu_backend, name, mk, ref, c):
    _check(mk(), ref, emu_backend, "cpu", 2, c, (9, 8, 10), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mk,ref,c", CASES, ids=[c[0] for c in CASES])
def test_losses_gpu(name, mk, ref, c):
    _check(mk(), ref, None, "cuda", 2, c, (40, 48, 36), name)


def _check_17_channels(be, dev):
    """the one-call fused path carries any channel count with n * c <= 1024; only the two-call form stops at 16 classes"""
    _check(losses.HipDiceLoss(sigmoid=True), lambda z, t: O.dice_loss(z, t, True), be, dev, 1, 17, (5, 4, 6))
    crit = losses.HipDiceLoss(softmax=True)
    crit._be = be if be is not None else object()
    z, t = _data(1, 17, (5, 4, 6))
    with pytest.raises(NotImplementedError, match="more than 16 classes"):
        crit(z.to(dev), t.to(dev))


def test_fused_dice_17_channels_on_emulator(emu_backend):
    _check_17_channels(emu_backend, "cpu")


@pytest.mark.gpu
def test_fused_dice_17_channels_gpu():
    _check_17_channels(None, "cuda")


# monai DiceLoss options beyond the shipped configuration (the reference passes the config's loss kwargs straight to the class:
# unet3d/scripts/script_utils.py:61-77): (constructor kwargs, channels, label-map target?)
EX_CASES = [
    ("softmax", dict(softmax=True), 4, False),
    ("softmax_onehot_nobg", dict(softmax=True, to_onehot_y=True, include_background=False), 4, True),
    ("onehot_sigmoid", dict(sigmoid=True, to_onehot_y=True), 3, True),
    ("jaccard", dict(sigmoid=True, jaccard=True), 3, False),
    ("jaccard_squared_batch", dict(sigmoid=True, jaccard=True, squared_pred=True, batch=True), 3, False),
    ("weight", dict(sigmoid=True, weight=[0.2, 1.0, 3.0]), 3, False),
    ("weight_scalar_nobg", dict(sigmoid=True, weight=2.5, include_background=False), 3, False),
    ("sum", dict(sigmoid=True, reduction="sum"), 3, False),
    ("none", dict(sigmoid=True, reduction="none"), 3, False),
    ("none_batch_nobg", dict(softmax=True, reduction="none", batch=True, include_background=False), 4, False),
    ("none_softmax_weight_jaccard", dict(softmax=True, reduction="none", weight=[1.0, 0.5, 2.0, 0.0], jaccard=True), 4, False),
    ("no_activation", dict(reduction="sum", jaccard=True), 2, False),
]


def _check_ex(kw, be, dev, n, c, dhw, labels):
    z, t = _data(n, c, dhw, seed=3)
    if labels:
        t = torch.randint(0, c, (n, 1) + tuple(dhw), generator=torch.Generator().manual_seed(5))
    if not (kw.get("sigmoid") or kw.get("softmax")):
        z = torch.sigmoid(z)                                   # "probabilities in": keep the values in the range Dice is meant for
    okw = {("sigmoid" if k == "sigmoid" else k): v for k, v in kw.items()}
    okw.setdefault("sigmoid", False)
    zr = z.clone().requires_grad_(True)
    ref = O.dice_loss(zr, t, **okw)
    up = torch.rand(ref.shape, generator=torch.Generator().manual_seed(7)) + 0.5      # a different upstream gradient for every term
    (ref * up).sum().backward()
    crit = losses.HipDiceLoss(**kw)
    if be is not None:
        crit._be = be
    zg = z.to(dev).requires_grad_(True)
    loss = crit(zg, t.to(dev))
    assert loss.shape == ref.shape
    (loss * up.to(dev)).sum().backward()
    assert C.rel_err(loss.detach().cpu(), ref.detach()) < TOL
    assert C.rel_err(zg.grad.cpu(), zr.grad) < TOL


@pytest.mark.parametrize("name,kw,c,labels", EX_CASES, ids=[c[0] for c in EX_CASES])
def test_dice_options_on_emulator(emu_backend, name, kw, c, labels):
    _check_ex(kw, emu_backend, "cpu", 2, c, (9, 8, 10), labels)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,c,labels", EX_CASES, ids=[c[0] for c in EX_CASES])
def test_dice_options_gpu(name, kw, c, labels):
    _check_ex(kw, None, "cuda", 2, c, (40, 48, 36), labels)


def test_dice_option_validation_matches_monai():
    """monai.losses.DiceLoss.__init__ / forward checks (same exception types; messages restated from MONAI 1.3)."""
    with pytest.raises(ValueError, match="Incompatible values"):
        losses.HipDiceLoss(sigmoid=True, softmax=True)
    with pytest.raises(TypeError, match="other_act must be None or callable"):
        losses.HipDiceLoss(other_act=3)
    with pytest.raises(NotImplementedError, match="other_act"):
        losses.HipDiceLoss(other_act=torch.tanh)
    with pytest.raises(ValueError, match="Unsupported reduction"):
        losses.HipDiceLoss(reduction="median")
    crit = losses.HipDiceLoss(sigmoid=True, weight=[1.0, 2.0])
    crit._be = object()                                        # the checks below run before any kernel
    z, t = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4)
    with pytest.raises(ValueError, match="length of the `weight` sequence"):
        crit(z, t)
    crit = losses.HipDiceLoss(sigmoid=True, weight=[1.0, -2.0, 1.0])
    crit._be = object()
    with pytest.raises(ValueError, match="no less than 0"):
        crit(z, t)
    # a weight that arrives AFTER construction is checked as well: load_state_dict, buffer assignment, an in-place edit
    crit = losses.HipDiceLoss(sigmoid=True, weight=[1.0, 2.0, 1.0])
    crit._be = object()
    crit.load_state_dict({"class_weight": torch.tensor([1.0, -2.0, 1.0])})
    with pytest.raises(ValueError, match="no less than 0"):
        crit(z, t)
    crit = losses.HipDiceLoss(sigmoid=True, weight=[1.0, 2.0, 1.0])
    crit._be = object()
    crit.class_weight = torch.tensor([-1.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="no less than 0"):
        crit(z, t)
    crit = losses.HipDiceLoss(sigmoid=True, weight=[1.0, 2.0, 1.0])
    crit._be = object()
    crit.class_weight[2] = -0.5
    with pytest.raises(ValueError, match="no less than 0"):
        crit(z, t)
    crit = losses.HipDiceLoss(softmax=True, to_onehot_y=True)
    crit._be = object()
    with pytest.raises(AssertionError, match="channel with length equal to one"):
        crit(z, t)


def test_unsupported_options_raise():
    with pytest.raises(NotImplementedError, match="weight"):
        losses.HipDiceCELoss(softmax=True, weight=[1.0, 2.0])
    with pytest.raises(NotImplementedError, match="reduction"):
        losses.HipDiceCELoss(sigmoid=True, reduction="none")
    with pytest.raises(ValueError, match="Incompatible values"):
        losses.HipDiceCELoss(sigmoid=True, softmax=True)
    with pytest.raises(NotImplementedError):
        losses.HipBCEWithLogitsLoss(pos_weight=torch.ones(3))
    with pytest.raises(NotImplementedError):
        losses.HipCrossEntropyLoss(label_smoothing=0.1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X"):
            losses.HipBCEWithLogitsLoss()(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4))


def test_cross_entropy_index_targets_out_of_range_are_flagged_on_request():
    """torch's ignore_index is not implemented (losses.py: HipCrossEntropyLoss docstring); `validate_targets=True` turns the silent
    difference into an error before any kernel runs."""
    crit = losses.HipCrossEntropyLoss(validate_targets=True)
    crit._be = object()
    z = torch.zeros(1, 3, 2, 2, 2)
    t = torch.zeros(1, 2, 2, 2, dtype=torch.long)
    t[0, 0, 0, 0] = -100
    with pytest.raises(ValueError, match="ignore_index"):
        crit(z, t)
    t[0, 0, 0, 0] = 3
    with pytest.raises(ValueError, match="outside"):
        crit(z, t)



def test_weight_timing(emu_backend):
    """HipDiceLoss takes a negative weight at construction and raises at forward (MONAI's DiceLoss), and weights more than one counted
    class only; the focal family raises at construction as well and always applies the weight."""
    crit = losses.HipDiceLoss(sigmoid=True, weight=[1.0, -1.0, 1.0])
    crit._be = object()
    with pytest.raises(ValueError, match="no less than 0"):
        crit(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4))
    for cls in (losses.HipFocalLoss, losses.HipDiceFocalLoss):
        with pytest.raises(ValueError, match="no less than 0"):
            cls(weight=[1.0, -1.0, 1.0])
    z, t = _data(2, 2, (9, 8, 10))

    def value(crit):
        crit._be = emu_backend
        return crit(z, t)
    assert torch.equal(value(losses.HipDiceLoss(sigmoid=True, weight=[2.0], include_background=False)),
                       value(losses.HipDiceLoss(sigmoid=True, include_background=False)))
    a, b = float(value(losses.HipFocalLoss(weight=[2.0], include_background=False))), float(value(losses.HipFocalLoss(include_background=False)))
    assert abs(a - 2.0 * b) < 1e-6 * abs(b) and b > 0.0, (a, b)


def test_state_dict_keys_and_round_trip():
    for cls in (losses.HipDiceLoss, losses.HipFocalLoss, losses.HipDiceFocalLoss):
        crit = cls(weight=[0.5, 1.0, 2.0])
        assert list(crit.state_dict()) == ["class_weight"]
        other = cls(weight=[1.0, 1.0, 1.0])
        other.load_state_dict(crit.state_dict())
        assert torch.equal(other.class_weight, torch.tensor([0.5, 1.0, 2.0]))
        assert list(cls().state_dict()) == []
        cls().load_state_dict(cls().state_dict())
    for crit in (losses.HipTverskyLoss(), losses.HipDiceCELoss(sigmoid=True), losses.HipBCEWithLogitsLoss(), losses.HipCrossEntropyLoss(),
                 losses.HipGeneralizedDiceLoss(sigmoid=True)):
        assert len(crit.state_dict()) == 0
        crit.load_state_dict({})


# two faults at once: which check speaks first. (module, constructor kwargs, logits shape or None = the constructor raises, target shape,
# exception, message fragment)
Z3, Z17, Z1 = (1, 3, 4, 4, 4), (1, 17, 2, 2, 2), (1, 1, 2, 2, 2)
PRECEDENCE = [
    ("focal_17ch_before_target_shape", "HipFocalLoss", {}, Z17, (1, 3, 2, 2, 2), NotImplementedError, "more than 16 classes"),
    ("tversky_17ch_before_target_shape", "HipTverskyLoss", {}, Z17, (1, 3, 2, 2, 2), NotImplementedError, "more than 16 classes"),
    ("dice_target_shape_before_17ch", "HipDiceLoss", dict(softmax=True), Z17, (1, 3, 2, 2, 2), AssertionError, "different shape"),
    ("dicece_target_shape_before_17ch", "HipDiceCELoss", dict(sigmoid=True), Z17, (1, 3, 2, 2, 2), AssertionError, "different shape"),
    ("dice_single_channel_before_weight", "HipDiceLoss", dict(include_background=False, weight=[1.0, 2.0]), Z1, Z1, ValueError,
     "single channel prediction"),
    ("dice_weight_length_before_target_shape", "HipDiceLoss", dict(sigmoid=True, weight=[1.0, 2.0]), Z3, (1, 2, 4, 4, 4), ValueError,
     "length of the `weight` sequence"),
    ("dice_weight_length_before_sign", "HipDiceLoss", dict(sigmoid=True, weight=[1.0, -2.0]), Z3, Z3, ValueError, "length of the `weight` sequence"),
    ("dicefocal_target_shape_before_weight_length", "HipDiceFocalLoss", dict(sigmoid=True, weight=[1.0, 2.0]), Z3, (1, 2, 4, 4, 4),
     AssertionError, "different shape"),
    ("focal_target_shape_before_weight_length", "HipFocalLoss", dict(weight=[1.0, 2.0]), Z3, (1, 2, 4, 4, 4), AssertionError, "different shape"),
    ("tversky_single_channel_before_target_shape", "HipTverskyLoss", dict(include_background=False), Z1, (1, 2, 2, 2, 2), ValueError,
     "single channel prediction"),
    ("dicece_other_act_and_reduction", "HipDiceCELoss", dict(reduction="median", other_act=torch.tanh), None, None, NotImplementedError,
     "does not implement: other_act"),
    ("dicece_reduction_and_weight", "HipDiceCELoss", dict(reduction="median", weight=[1.0, 2.0]), None, None, NotImplementedError,
     "does not implement: reduction, weight"),
    ("dicece_unsupported_before_lambdas", "HipDiceCELoss", dict(label_smoothing=0.1, lambda_dice=-1.0), None, None, NotImplementedError,
     "does not implement: label_smoothing"),
    ("dice_other_act_before_reduction", "HipDiceLoss", dict(reduction="median", other_act=torch.tanh), None, None, NotImplementedError, "other_act"),
    ("dicefocal_other_act_before_reduction", "HipDiceFocalLoss", dict(reduction="median", other_act=torch.tanh), None, None,
     NotImplementedError, "other_act"),
    ("dicefocal_reduction_before_gamma", "HipDiceFocalLoss", dict(reduction="none", gamma=-1.0), None, None, NotImplementedError, "reduction"),
    ("dicefocal_lambdas_before_weight_sign", "HipDiceFocalLoss", dict(lambda_dice=-1.0, weight=[1.0, -1.0]), None, None, ValueError,
     "lambda_dice and lambda_focal"),
    ("tversky_reduction_before_nan", "HipTverskyLoss", dict(reduction="median", alpha=float("nan")), None, None, ValueError, "Unsupported reduction"),
    ("gdl_w_type_before_other_act", "HipGeneralizedDiceLoss", dict(w_type="simple", other_act=3), None, None, NotImplementedError, "w_type"),
    ("gdl_reduction_name_before_options", "HipGeneralizedDiceLoss", dict(reduction="median", softmax=True), None, None, ValueError,
     "Unsupported reduction"),
]


@pytest.mark.parametrize("name,cls,kw,zs,ts,exc,frag", PRECEDENCE, ids=[r[0] for r in PRECEDENCE])
def test_precedence_of_checks(name, cls, kw, zs, ts, exc, frag):
    if zs is None:
        with pytest.raises(exc, match=frag):
            getattr(losses, cls)(**kw)
        return
    crit = getattr(losses, cls)(**kw)
    crit._be = object()                                        # every check here runs before any kernel
    with pytest.raises(exc, match=frag):
        crit(torch.zeros(zs), torch.zeros(ts))
