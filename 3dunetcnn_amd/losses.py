"""The losses the reference's look-up reaches, each a drop-in for the MONAI / torch class of the same name without "Hip":
`criterion(output, target)` -> a tensor supporting .item() and .backward().

HipDiceLoss (monai.losses.DiceLoss as the reference configures it: examples/brats2020/brats2020_config.json:112-116 ->
unet3d/scripts/script_utils.py:61-77, evaluated at unet3d/train/training_utils.py:111) and HipGeneralizedDiceLoss: one fused HIP pass
computes sigmoid, the three per-(n,c) sums, the loss and d(loss)/d(logits) (mi355_dice_fwd_bwd, csrc/loss_optim.hip); the target may stay
uint8 one-hot (unet3d/transforms/one_hot.py:10). The options that call does not carry (softmax, label-map targets, jaccard, weight,
reduction "sum" / "none") run the two-call form (mi355_dice_ex_forward / _backward), and HipTverskyLoss (monai.losses.TverskyLoss) runs on
the same two passes with its own finaliser (mi355_tversky_forward / _backward): both through _TwoCallFunction.

The compound losses add a second fused pass onto the value and gradient of a Dice term (_dice_term): HipDiceCELoss /
HipBCEWithLogitsLoss / HipCrossEntropyLoss (monai.losses.DiceCELoss, torch.nn.BCEWithLogitsLoss / CrossEntropyLoss: script_utils.py:61-77
tries unet3d.losses, torch.nn, monai.losses in that order) the cross-entropy pass mi355_ce_fwd_bwd; HipFocalLoss / HipDiceFocalLoss
(monai.losses.FocalLoss, DiceFocalLoss: the small-lesion losses) the focal pass mi355_focal_fwd_bwd (csrc/focal.hip).

Every constructor check, the class-weight buffer (_ClassWeighted) and the forward checks of input and target exist once, below.
"""
import torch
import torch.nn as nn

from . import ops as _ops


# ---- constructor checks (MONAI's, same messages, and what the kernels do not implement) ---------------------------------------------------
def _check_activation(who, sigmoid, softmax, other_act):
    if other_act is not None and not callable(other_act):
        raise TypeError(f"other_act must be None or callable but is {type(other_act).__name__}.")
    if int(bool(sigmoid)) + int(bool(softmax)) + int(other_act is not None) > 1:
        raise ValueError("Incompatible values: more than 1 of [sigmoid=True, softmax=True, other_act is not None].")
    if other_act is not None:
        raise NotImplementedError(f"{who} does not implement: other_act (a Python callable cannot run inside the fused kernels)")


def _option_name(reduction):
    return str(getattr(reduction, "value", reduction)).lower()


def _reduction(reduction, allowed, who):
    reduction = _option_name(reduction)
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f'Unsupported reduction: {reduction}, available options are ["mean", "sum", "none"].')
    if reduction not in allowed:
        raise NotImplementedError(f"{who} does not implement: reduction={reduction!r}")
    return reduction


def _check_lambdas(who, lambda_dice, lambda_other, other):
    lambda_dice, lambda_other = float(lambda_dice), float(lambda_other)
    if lambda_dice < 0.0 or lambda_other < 0.0:
        raise ValueError(f"lambda_dice and {other} should be no less than 0.0.")
    if lambda_dice == 0.0 and lambda_other == 0.0:
        raise ValueError(f"{who}: lambda_dice and {other} are both 0 -- the loss would be identically zero")
    return lambda_dice, lambda_other


def _check_focal(gamma, alpha):
    gamma = float(gamma)
    if not gamma >= 0.0 or gamma == float("inf"):
        raise ValueError(f"gamma should be a finite number no less than 0 but is {gamma}.")
    if alpha is not None:
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"alpha should be in [0, 1] but is {alpha}.")
    return gamma, alpha


# ---- forward checks: every module calls these in the order of its MONAI counterpart ---------------------------------------------------------
def _check_device(mod, input):
    if input.device.type != "cuda" and mod._be is None:
        raise RuntimeError(f"{type(mod).__name__} runs on an MI355X only (no CPU fallback)")


def _check_input(mod, input):
    _check_device(mod, input)
    if not mod.include_background and input.shape[1] == 1:
        raise ValueError("single channel prediction, `include_background=False` ignored is not supported: pass include_background=True")


def _check_classes(input):
    if input.shape[1] > 16:
        raise NotImplementedError("more than 16 classes")


def _prepare_target(input, target, onehot):
    """target in a type the kernels read: an int32 label map [N, 1, ...] (to_onehot_y with more than one channel), else uint8 / fp32 of
    the input's shape"""
    if onehot and input.shape[1] > 1:                     # MONAI: "single channel prediction, `to_onehot_y=True` ignored."
        if target.shape[0] != input.shape[0] or target.shape[1] != 1 or target.shape[2:] != input.shape[2:]:
            raise AssertionError("labels should have a channel with length equal to one.")             # monai.networks.one_hot
        return target.to(torch.int32)
    if target.shape != input.shape:
        raise AssertionError(f"ground truth has different shape ({tuple(target.shape)}) from input ({tuple(input.shape)})")
    return target if target.dtype in (torch.uint8, torch.float32) else target.to(torch.float32)


def _activation(mod, input):
    """activation code of the two-call passes (MONAI: "single channel prediction, `softmax=True` ignored.")"""
    return "softmax" if mod.softmax and input.shape[1] > 1 else ("sigmoid" if mod.sigmoid else None)


class _ClassWeighted(nn.Module):
    """`weight` of the MONAI losses: the buffer `class_weight`, whose sign is read on the host once per VALUE -- at construction, while
    the tensor is still on the host, and again (lazily, in forward) whenever the buffer has been replaced or written since:
    load_state_dict, `crit.class_weight = ...`, an in-place edit. A device read on every forward would be a host sync inside the step.
    MONAI's DiceLoss raises on a negative weight at forward only; its FocalLoss at construction as well (reject_negative)."""
    def _init_weight(self, weight, reject_negative):
        self.register_buffer("class_weight", torch.as_tensor(weight, dtype=torch.float32) if weight is not None else None)
        self._weight_checked = None
        self._weight_negative = False
        self._check_weight_sign()
        if reject_negative and self._weight_negative:
            raise ValueError("the value/values of the `weight` should be no less than 0.")

    def _check_weight_sign(self):
        """(Re)read the sign of `class_weight` when the buffer is not the one last looked at (identity, storage, version counter)."""
        w = self.class_weight
        if w is None:
            self._weight_checked, self._weight_negative = None, False
            return
        key = (id(w), w.data_ptr(), w._version, w.device)
        if key == self._weight_checked:
            return
        if w.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return                                   # no host read inside a capture: the check happens at the next eager forward
        self._weight_negative = bool(w.numel() and float(w.min()) < 0)
        self._weight_checked = key

    def _counted_weight(self, ce):
        """the weight of this call: None, or one factor per counted class (a scalar is expanded), length and sign checked"""
        cw = self.class_weight
        if cw is None:
            return None
        if cw.ndim == 0:
            cw = cw.repeat(ce)
        elif cw.shape[0] != ce:
            raise ValueError("the length of the `weight` sequence should be the same as the number of classes. "
                             "If `include_background=False`, the weight should not include the background category class 0.")
        self._check_weight_sign()
        if self._weight_negative:
            raise ValueError("the value/values of the `weight` should be no less than 0.")
        return cw


def _on_device(cw, logits):
    return None if cw is None else cw.to(device=logits.device, dtype=torch.float32).contiguous()


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
def _leave(ctx, dlogits):
    """A fused-pass loss's forward leaves its UNSCALED d(loss)/d(logits) (or None: no gradient wanted) on its autograd node. This and
    `_take` are the one place that names where: `_scaled` (the node's own backward) and `_StackedFunction` (which scales it by
    w_l x upstream straight into the stack's slot) both read it through `_take`."""
    ctx.dlogits = dlogits


def _take(ctx):
    """The gradient `_leave` stored, released: None when the node holds none (another kind of node, or already taken)."""
    d = getattr(ctx, "dlogits", None)
    if d is not None:
        ctx.dlogits = None
    return d


def _scaled(ctx, g):
    """d(loss)/d(logits) computed by the forward pass, times the incoming scalar gradient -- in place (no second logits-sized tensor)."""
    d = _take(ctx)
    if d is None:
        raise RuntimeError("loss backward called a second time: d(loss)/d(logits) is released by the first backward")
    return d.mul_(g)


class _DiceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, mod):
        be = mod._be or _ops.default_backend(logits.device)
        want = ctx.needs_input_grad[0]
        loss, dlogits = be.dice(logits.contiguous(), target.contiguous(), sigmoid=mod.sigmoid, batch=mod.batch,
                                squared_pred=mod.squared_pred, smooth_nr=mod.smooth_nr, smooth_dr=mod.smooth_dr, want_grad=want,
                                generalized=mod.generalized, include_background=mod.include_background)
        _leave(ctx, dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        return _scaled(ctx, g), None, None


class _TwoCallFunction(torch.autograd.Function):
    """The losses on the extended Dice passes: forward = be.<op>_forward (the sums + the finalisation of `op`: "dice_ex" | "tversky"),
    backward = be.<op>_backward, one pass that applies the upstream gradient of every term. `opts`: the keywords of <op>_forward."""
    @staticmethod
    def forward(ctx, logits, target, mod, op, opts):
        be = mod._be or _ops.default_backend(logits.device)
        logits, target = logits.contiguous(), target.contiguous()
        loss, state = getattr(be, op + "_forward")(logits, target, **opts)
        ctx.saved = (getattr(be, op + "_backward"), logits, target, state)
        if mod.reduction != "none":
            return loss.reshape(())
        ce = logits.shape[1] - (0 if mod.include_background else 1)
        lead = [ce] if mod.batch else [logits.shape[0], ce]            # MONAI: f.view(list(f.shape[0:2]) + [1] * (input.dim() - 2))
        return loss.reshape(lead + [1] * (logits.dim() - 2))

    @staticmethod
    def backward(ctx, g):
        if ctx.saved is None:
            raise RuntimeError("loss backward called a second time: its saved tensors are released by the first backward")
        backward, logits, target, state = ctx.saved
        ctx.saved = None
        return backward(logits, target, state, g), None, None, None, None


def _onehot_u8(be, labels, n_classes):
    """class-index map [N, 1, ...] or [N, ...] -> uint8 one-hot [N, C, ...] on the device (mi355_one_hot, one launch per sample)."""
    if labels.dim() >= 2 and labels.shape[1] == 1 and labels.dim() > 2:
        labels = labels[:, 0]
    groups = [[c] for c in range(n_classes)]
    return torch.stack([be.one_hot(labels[i].float().contiguous(), groups) for i in range(labels.shape[0])])


def _dice_term(be, logits, target, mod, lambda_dice, want_grad, class_weight=None):
    """lambda_dice * Dice, the first term of a compound loss -> (loss [1], its d/dlogits or None). target: of the logits' shape. The
    one-call fused kernel where it carries the module's options, else the two-call form with lambda_dice as the upstream gradient."""
    if logits.shape[1] - (0 if mod.include_background else 1) == 1:
        class_weight = None                                   # MONAI's Dice weights more than one class only
    if not (mod.softmax or mod.jaccard or class_weight is not None or mod.reduction == "sum"):
        loss, dlogits = be.dice(logits, target, sigmoid=mod.sigmoid, batch=mod.batch, squared_pred=mod.squared_pred,
                                smooth_nr=mod.smooth_nr, smooth_dr=mod.smooth_dr, want_grad=want_grad, grad_scale=lambda_dice,
                                include_background=mod.include_background)
    else:
        loss, state = be.dice_ex_forward(logits, target, activation=_activation(mod, logits), batch=mod.batch, squared_pred=mod.squared_pred,
                                         include_background=mod.include_background, jaccard=mod.jaccard, reduction=mod.reduction,
                                         smooth_nr=mod.smooth_nr, smooth_dr=mod.smooth_dr, class_weight=class_weight)
        dlogits = None
        if want_grad:
            dlogits = be.dice_ex_backward(logits, target, state, torch.full((1,), lambda_dice, dtype=torch.float32, device=logits.device))
    return loss.mul_(lambda_dice), dlogits


class _CEFunction(torch.autograd.Function):
    """loss = lambda_dice * Dice + lambda_ce * CE (either weight may be 0), value and d/dlogits from the fused HIP passes."""
    @staticmethod
    def forward(ctx, logits, target, mod):
        be = mod._be or _ops.default_backend(logits.device)
        want = ctx.needs_input_grad[0]
        logits, target = logits.contiguous(), target.contiguous()
        c = logits.shape[1]
        if target.shape != logits.shape:                      # class indices (to_onehot_y / index targets): one-hot once, both terms use it
            target = _onehot_u8(be, target, c)
        loss = dlogits = None
        if mod.lambda_dice != 0.0:
            loss, dlogits = _dice_term(be, logits, target, mod, mod.lambda_dice, want)
        if mod.lambda_ce != 0.0:
            w = mod.lambda_ce
            if mod.reduction == "sum":                        # CrossEntropyLoss / BCEWithLogitsLoss(reduction="sum") = mean x count
                w *= logits.shape[0] * logits[0, 0].numel() * (1 if mod.ce_mode == "softmax" else c)
            loss, dlogits = be.cross_entropy(logits, target, mode=mod.ce_mode, weight=w, loss=loss,
                                             dlogits=dlogits if want else None, want_grad=want)
        _leave(ctx, dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        return _scaled(ctx, g), None, None


def _focal_forward(mod, input, target):
    """forward of HipFocalLoss / HipDiceFocalLoss: MONAI's FocalLoss checks the target before the weight"""
    _check_input(mod, input)
    _check_classes(input)
    target = _prepare_target(input, target, mod.to_onehot_y)
    cw = mod._counted_weight(input.shape[1] - (0 if mod.include_background else 1))
    return _DiceFocalFunction.apply(input.float(), target, mod, cw)


class _DiceFocalFunction(torch.autograd.Function):
    """loss = lambda_dice * Dice + lambda_focal * Focal (lambda_dice = 0: the focal term alone), value and d/dlogits from the fused HIP
    passes: the focal pass accumulates onto the Dice term's value and gradient the way the CE pass of _CEFunction does."""
    @staticmethod
    def forward(ctx, logits, target, mod, cw):
        be = mod._be or _ops.default_backend(logits.device)
        want = ctx.needs_input_grad[0]
        logits, target = logits.contiguous(), target.contiguous()
        cw = _on_device(cw, logits)
        loss = dlogits = None
        if mod.lambda_dice != 0.0:
            if target.shape != logits.shape:                  # a label map is expanded once, both terms use the expansion
                target = _onehot_u8(be, target, logits.shape[1])
            loss, dlogits = _dice_term(be, logits, target, mod, mod.lambda_dice, want, cw)
        if mod.lambda_focal != 0.0:
            loss, dlogits = be.focal(logits, target, mode="softmax" if mod.focal_softmax else "sigmoid", gamma=mod.gamma, alpha=mod.alpha,
                                     include_background=mod.include_background, reduction=mod.reduction, class_weight=cw,
                                     weight=mod.lambda_focal, loss=loss, dlogits=dlogits if want else None, want_grad=want)
        _leave(ctx, dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        return _scaled(ctx, g), None, None, None


# ---- Dice / generalized Dice / Tversky --------------------------------------------------------------------------------------------------
class HipDiceLoss(_ClassWeighted):
    """monai.losses.DiceLoss. The shipped configuration (sigmoid / no activation, same-shape targets, reduction="mean") is one fused
    pass (value + gradient); softmax, to_onehot_y, jaccard, weight and reduction="sum" / "none" run the two-call form. other_act (an
    arbitrary Python callable) cannot run inside a kernel and raises."""
    generalized = False

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None,
                 squared_pred=False, jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, weight=None):
        super().__init__()
        _check_activation(type(self).__name__, sigmoid, softmax, other_act)
        reduction = _reduction(reduction, ("mean", "sum", "none"), type(self).__name__)
        if self.generalized and (to_onehot_y or softmax or jaccard or weight is not None or reduction != "mean"):
            raise NotImplementedError("HipGeneralizedDiceLoss implements sigmoid / no activation, same-shape targets, reduction='mean'")
        self.sigmoid, self.softmax, self.to_onehot_y = bool(sigmoid), bool(softmax), bool(to_onehot_y)
        self.squared_pred, self.jaccard, self.batch = bool(squared_pred), bool(jaccard), bool(batch)
        self.reduction = reduction
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)
        self.include_background = bool(include_background)
        self._init_weight(weight, reject_negative=False)
        self._be = None

    def forward(self, input, target):
        _check_input(self, input)
        ce = input.shape[1] - (0 if self.include_background else 1)
        cw = self._counted_weight(ce) if ce != 1 else None    # MONAI applies the weight only for more than one class
        target = _prepare_target(input, target, self.to_onehot_y)
        activation = _activation(self, input)
        label_map = target.dtype == torch.int32
        if not (activation == "softmax" or label_map or self.jaccard or cw is not None or self.reduction != "mean"):
            return _DiceFunction.apply(input.float(), target, self)
        _check_classes(input)
        logits = input.float()
        opts = dict(activation=activation, batch=self.batch, squared_pred=self.squared_pred, include_background=self.include_background,
                    jaccard=self.jaccard, reduction=self.reduction, smooth_nr=self.smooth_nr, smooth_dr=self.smooth_dr,
                    class_weight=_on_device(cw, logits))
        return _TwoCallFunction.apply(logits, target, self, "dice_ex", opts)


class HipGeneralizedDiceLoss(HipDiceLoss):
    """monai.losses.GeneralizedDiceLoss(w_type="square") -- the loss doc/Configuration.md:41 of the reference configures
    ({"name": "GeneralizedDiceLoss", "include_background": false, "sigmoid": true})."""
    generalized = True

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, w_type="square",
                 reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False):
        if _option_name(w_type) != "square":
            raise NotImplementedError("HipGeneralizedDiceLoss implements w_type='square' (the MONAI default)")
        super().__init__(include_background=include_background, to_onehot_y=to_onehot_y, sigmoid=sigmoid, softmax=softmax,
                         other_act=other_act, reduction=reduction, smooth_nr=smooth_nr, smooth_dr=smooth_dr, batch=batch)


class HipTverskyLoss(nn.Module):
    """monai.losses.TverskyLoss: 1 - (tp + smooth_nr) / (tp + alpha fp + beta fn + smooth_dr) per (n, c) (per c with batch) on the sums of
    the extended Dice passes; activation, to_onehot_y, include_background, batch and reduction "mean" | "sum" | "none" as in HipDiceLoss."""
    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, alpha=0.5, beta=0.5,
                 reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False):
        super().__init__()
        _check_activation(type(self).__name__, sigmoid, softmax, other_act)
        self.reduction = _reduction(reduction, ("mean", "sum", "none"), type(self).__name__)
        self.alpha, self.beta = float(alpha), float(beta)
        if self.alpha != self.alpha or self.beta != self.beta:
            raise ValueError("alpha and beta should be numbers.")
        self.sigmoid, self.softmax, self.to_onehot_y, self.batch = bool(sigmoid), bool(softmax), bool(to_onehot_y), bool(batch)
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)
        self.include_background = bool(include_background)
        self._be = None

    def forward(self, input, target):
        _check_input(self, input)
        _check_classes(input)
        target = _prepare_target(input, target, self.to_onehot_y)
        opts = dict(activation=_activation(self, input), alpha=self.alpha, beta=self.beta, batch=self.batch,
                    include_background=self.include_background, reduction=self.reduction, smooth_nr=self.smooth_nr, smooth_dr=self.smooth_dr)
        return _TwoCallFunction.apply(input.float(), target, self, "tversky", opts)


# ---- cross-entropy and Dice + cross-entropy ---------------------------------------------------------------------------------------------
class _CEBase(nn.Module):
    """Options of _CEFunction as HipBCEWithLogitsLoss / HipCrossEntropyLoss run it: the CE term alone."""
    include_background = True
    sigmoid = True
    softmax = jaccard = squared_pred = batch = index_targets = False
    smooth_nr = smooth_dr = 1e-5
    lambda_dice, lambda_ce, ce_mode, reduction = 0.0, 1.0, "softmax", "mean"
    _be = None

    def forward(self, input, target):
        _check_device(self, input)
        lead, rest = input.shape[0], tuple(input.shape[2:])
        as_index = self.index_targets and input.shape[1] > 1 and tuple(target.shape) in ((lead,) + rest, (lead, 1) + rest)
        if not as_index:
            target = _prepare_target(input, target, False)
        _check_classes(input)
        return _CEFunction.apply(input.float(), target, self)


class HipDiceCELoss(_CEBase):
    """monai.losses.DiceCELoss: lambda_dice * DiceLoss(...) + lambda_ce * CrossEntropyLoss(input, target) for more than one channel,
    BCEWithLogitsLoss for a single channel. softmax / jaccard / squared_pred / batch / include_background configure the Dice term (MONAI:
    the CE term always sees the raw logits and every channel), to_onehot_y takes a class-index target [N, 1, ...] (expanded once on the
    device, both terms use the expansion: CE of indices == CE of their one-hot), reduction "mean" | "sum" applies to both terms. Not
    implemented (raise): `weight` (MONAI hands it to the CE term too), `label_smoothing`, `other_act`, reduction "none"."""
    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, squared_pred=False,
                 jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, weight=None, lambda_dice=1.0,
                 lambda_ce=1.0, label_smoothing=0.0):
        super().__init__()
        _check_activation(type(self).__name__, sigmoid, softmax, other_act)
        reduction = _option_name(reduction)
        bad = [k for k, v in dict(reduction=reduction not in ("mean", "sum"), weight=weight is not None,
                                  label_smoothing=label_smoothing != 0.0).items() if v]
        if bad:
            raise NotImplementedError("HipDiceCELoss does not implement: " + ", ".join(bad))
        self.lambda_dice, self.lambda_ce = _check_lambdas(type(self).__name__, lambda_dice, lambda_ce, "lambda_ce")
        self.sigmoid, self.softmax, self.index_targets = bool(sigmoid), bool(softmax), bool(to_onehot_y)
        self.squared_pred, self.jaccard, self.batch = bool(squared_pred), bool(jaccard), bool(batch)
        self.reduction = reduction
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)
        self.include_background = bool(include_background)

    def forward(self, input, target):
        self.ce_mode = "softmax" if input.shape[1] > 1 else "bce"
        return super().forward(input, target)


class HipBCEWithLogitsLoss(_CEBase):
    """torch.nn.BCEWithLogitsLoss(reduction="mean") on same-shape targets (the multi-label form of the BraTS nested regions)."""
    def __init__(self, weight=None, size_average=None, reduce=None, reduction="mean", pos_weight=None):
        super().__init__()
        if weight is not None or pos_weight is not None or reduction != "mean" or size_average is not None or reduce is not None:
            raise NotImplementedError("HipBCEWithLogitsLoss implements reduction='mean' without weights")
        self.ce_mode = "bce"


class HipCrossEntropyLoss(_CEBase):
    """torch.nn.CrossEntropyLoss(reduction="mean") with class-PROBABILITY targets of the input's shape (one-hot uint8 / float) or
    class-INDEX targets [N, ...] (expanded to one-hot on the device).

    `ignore_index` is NOT implemented: torch drops voxels labelled `ignore_index` (default -100) from the sum AND from the mean's
    denominator; here a label outside [0, C) expands to an all-zero one-hot row that contributes 0 to the sum but still counts in the
    denominator, so the value differs from torch's whenever such labels occur. None of the reference's configurations produces them
    (its label maps are re-encoded to {0..C-1} or to nested regions, unet3d/utils/one_hot.py). `validate_targets=True` checks every
    index target for out-of-range labels and raises (one device read = a host sync per call: a debugging aid, off by default)."""
    index_targets = True

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0,
                 validate_targets=False):
        super().__init__()
        if weight is not None or reduction != "mean" or label_smoothing != 0.0 or size_average is not None or reduce is not None:
            raise NotImplementedError("HipCrossEntropyLoss implements reduction='mean' without weights / smoothing")
        self.ce_mode = "softmax"
        self.validate_targets = bool(validate_targets)

    def forward(self, input, target):
        if self.validate_targets and target.dim() == input.dim() - 1:
            lo, hi = int(target.min()), int(target.max())
            if lo < 0 or hi >= input.shape[1]:
                raise ValueError(f"HipCrossEntropyLoss: class-index target outside [0, {input.shape[1]}) (min {lo}, max {hi}): "
                                 "ignore_index / out-of-range labels are not implemented")
        return super().forward(input, target)


# ---- focal / Dice + focal ---------------------------------------------------------------------------------------------------------------
class HipFocalLoss(_ClassWeighted):
    """monai.losses.FocalLoss: one fused pass (value + gradient, mi355_focal_fwd_bwd). Sigmoid form by default, the softmax form with
    use_softmax=True and more than one counted channel; `alpha` balances positives against negatives (sigmoid) or foreground against
    background (softmax: 1 - alpha on channel 0, alpha elsewhere); `weight`: one factor per counted class; include_background=False drops
    channel 0 before the activation; to_onehot_y takes a class-index target [N, 1, ...] (read as indices, no one-hot tensor is made).
    reduction "mean" | "sum" (MONAI's: the sum over (n, c) of the spatial mean); "none" raises."""
    lambda_dice, lambda_focal = 0.0, 1.0

    def __init__(self, include_background=True, to_onehot_y=False, gamma=2.0, alpha=None, weight=None, reduction="mean", use_softmax=False):
        super().__init__()
        self.reduction = _reduction(reduction, ("mean", "sum"), type(self).__name__)
        self.gamma, self.alpha = _check_focal(gamma, alpha)
        self.include_background, self.to_onehot_y, self.focal_softmax = bool(include_background), bool(to_onehot_y), bool(use_softmax)
        self._init_weight(weight, reject_negative=True)
        self._be = None

    def forward(self, input, target):
        return _focal_forward(self, input, target)


class HipDiceFocalLoss(_ClassWeighted):
    """monai.losses.DiceFocalLoss: lambda_dice * DiceLoss(...) + lambda_focal * FocalLoss(...). sigmoid / softmax / squared_pred / jaccard /
    batch / smooth_* configure the Dice term; the focal term sees the raw logits, in the softmax form iff softmax=True; gamma / alpha
    configure it. include_background, to_onehot_y (the label map is expanded once, both terms read the expansion), `weight` (class
    weights) and reduction "mean" | "sum" apply to both. Not implemented (raise): other_act, reduction "none"."""
    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, squared_pred=False,
                 jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, gamma=2.0, weight=None, lambda_dice=1.0,
                 lambda_focal=1.0, alpha=None):
        super().__init__()
        _check_activation(type(self).__name__, sigmoid, softmax, other_act)
        self.reduction = _reduction(reduction, ("mean", "sum"), type(self).__name__)
        self.gamma, self.alpha = _check_focal(gamma, alpha)
        self.lambda_dice, self.lambda_focal = _check_lambdas(type(self).__name__, lambda_dice, lambda_focal, "lambda_focal")
        self.sigmoid, self.softmax, self.to_onehot_y = bool(sigmoid), bool(softmax), bool(to_onehot_y)
        self.squared_pred, self.jaccard, self.batch = bool(squared_pred), bool(jaccard), bool(batch)
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)
        self.include_background = bool(include_background)
        self.focal_softmax = self.softmax
        self._init_weight(weight, reject_negative=True)
        self._be = None

    def forward(self, input, target):
        return _focal_forward(self, input, target)


# ---- deep supervision -------------------------------------------------------------------------------------------------------------------
class _StackedFunction(torch.autograd.Function):
    """sum_l w_l * loss(stacked[:, l], target) on a stacked output [N, L, C, ...]. The gradient is assembled in the STACK's memory order
    ([L][N][C]..., returned as its transpose(0, 1) view): HipDynUNetDS's backward reads that buffer as it is. Each level costs the one
    pass over its gradient that the single-output losses spend on the upstream factor (_scaled): here it scales by w_l x upstream and
    writes the level's slot. Nothing reads the device on the host; every shape is fixed by the input's."""
    @staticmethod
    def forward(ctx, stacked, target, mod, weights):
        want = ctx.needs_input_grad[0]
        levels, total = [], None
        for l, w in enumerate(weights):
            with torch.enable_grad():
                xl = stacked[:, l].detach().requires_grad_(want)
                ll = mod.loss(xl, target)
            if ll.dim() != 0:
                raise NotImplementedError("HipDeepSupervisionLoss needs a criterion that returns a scalar (reduction 'mean' or 'sum')")
            levels.append((xl, ll, w))
            term = ll.detach() * w
            total = term if total is None else total + term
        ctx.levels = levels if want else None
        ctx.stack_shape = tuple(stacked.shape)
        return total

    @staticmethod
    def backward(ctx, g):
        levels = ctx.levels
        if levels is None:
            raise RuntimeError("loss backward called a second time: the per-level gradients are released by the first backward")
        ctx.levels = None
        shape = ctx.stack_shape
        xl0 = levels[0][0]
        gbuf = torch.empty((shape[1], shape[0]) + shape[2:], dtype=torch.float32, device=xl0.device)
        for l, (xl, ll, w) in enumerate(levels):
            up = g * w
            d = _take(ll.grad_fn) if xl.dtype == torch.float32 else None
            if d is not None:                                 # a fused-pass loss: its forward already left d(loss)/d(logits) (_leave)
                torch.mul(d, up, out=gbuf[l])
            else:                                             # the two-call forms (their backward pass applies `up`), any other criterion
                (d,) = torch.autograd.grad(ll, xl, grad_outputs=up.to(ll.dtype))
                gbuf[l].copy_(d)
        return gbuf.transpose(0, 1), None, None, None


# the criteria a config block may name inside HipDeepSupervisionLoss ({"name": ..., options}), with or without the "Hip" prefix
_CRITERIA = {n: c for c in (HipDiceLoss, HipGeneralizedDiceLoss, HipTverskyLoss, HipDiceCELoss, HipBCEWithLogitsLoss, HipCrossEntropyLoss,
                            HipFocalLoss, HipDiceFocalLoss) for n in (c.__name__, c.__name__[3:])}


class HipDeepSupervisionLoss(nn.Module):
    """monai.losses.DeepSupervisionLoss(loss, weight_mode="exp", weights=None): sum_l w_l * loss(input[l], target) over the outputs of a
    deeply supervised network, weights not normalised. [MONAI-memory: restated from MONAI >= 1.2 `ds_loss.py`, parity unpinned.]
    weight_mode "exp": w_l = max(0.5 ** l, 0.0625); "same": 1; "two": 1 for level 0 and 0.5 for the others; explicit `weights` are used when
    there are at least as many as levels. `loss`: any criterion of this module (scalar reduction).

    input: a list / tuple of [N, C, D, H, W] tensors (MONAI's form), or -- an extension for HipDynUNetDS, whose training output is the
    stack -- one 6-D tensor [N, L, C, D, H, W], unbound along dim 1; its gradient comes back in the stack's own memory order, so the
    network's backward takes it without a copy. A 5-D tensor goes straight to `loss`. Every entry must have the target's spatial shape:
    MONAI would down-sample the target for a coarser entry, which is not implemented (NotImplementedError)."""
    def __init__(self, loss, weight_mode="exp", weights=None):
        super().__init__()
        if isinstance(loss, dict):                            # a JSON config cannot hold a module: {"name": "DiceLoss", ...its options}
            opts = dict(loss)
            name = opts.pop("name")
            if name not in _CRITERIA:
                raise ValueError(f"HipDeepSupervisionLoss: unknown criterion {name!r}; one of {sorted(_CRITERIA)}")
            loss = _CRITERIA[name](**opts)
        self.loss = loss
        self.weight_mode = _option_name(weight_mode)
        self.weights = None if weights is None else [float(w) for w in weights]

    def get_weights(self, levels=1):
        levels = max(1, levels)
        if self.weights is not None and len(self.weights) >= levels:
            return self.weights[:levels]
        if self.weight_mode == "exp":
            return [max(0.5 ** l, 0.0625) for l in range(levels)]
        if self.weight_mode == "two":
            return [1.0 if l == 0 else 0.5 for l in range(levels)]
        return [1.0] * levels                                 # "same" (and, as in MONAI, any other name)

    def forward(self, input, target):
        if isinstance(input, torch.Tensor) and input.dim() != 6:
            return self.loss(input, target)
        entries = list(input) if isinstance(input, (list, tuple)) else None
        spatial = [tuple(e.shape[2:]) for e in entries] if entries is not None else [tuple(input.shape[3:])]
        if any(s != tuple(target.shape[2:]) for s in spatial):
            raise NotImplementedError("HipDeepSupervisionLoss: an entry's spatial shape differs from the target's (MONAI would down-sample "
                                      "the target; up-sample the heads instead, as DynUNet does)")
        weights = self.get_weights(len(entries) if entries is not None else input.shape[1])
        if entries is None:
            return _StackedFunction.apply(input, target, self, weights)
        total = None
        for e, w in zip(entries, weights):
            term = self.loss(e, target) * w
            total = term if total is None else total + term
        return total
