"""TEST INFRASTRUCTURE: torch restatements of the focal, Dice + focal and Tversky losses (the formulas of include/mi355_unet3d.h, written
with F.binary_cross_entropy_with_logits / F.logsigmoid / F.log_softmax and autograd; MONAI is not a dependency) and the case tables
tests/test_focal_losses.py (emulator) and tests/test_focal_losses_gpu.py (HIP library) share."""
import importlib

import torch
import torch.nn.functional as F

import op_cases as C
from oracle import torch_ops as O

losses = importlib.import_module("3dunetcnn_amd.losses")
TOL = 1e-3                      # the project's loss tolerance (tests/test_losses.py): relative value, op_cases.rel_err of the gradient


def _onehot(z, t):
    return torch.zeros_like(z).scatter_(1, t.long(), 1.0)


def focal_loss(z, t, gamma=2.0, alpha=None, weight=None, include_background=True, to_onehot_y=False, use_softmax=False, reduction="mean"):
    c = z.shape[1]
    y = _onehot(z, t) if (to_onehot_y and c > 1) else t.to(z.dtype)
    first = 0                                                    # channel index of the first counted channel
    if not include_background:
        z, y, first = z[:, 1:], y[:, 1:], 1                      # dropped BEFORE the activation
    ce = z.shape[1]
    shape = [1, ce] + [1] * (z.dim() - 2)
    if use_softmax and ce > 1:
        ls = F.log_softmax(z, 1)
        loss = -y * (1.0 - ls.exp()).pow(gamma) * ls
        if alpha is not None:
            a = torch.tensor([(1.0 - alpha) if first + j == 0 else alpha for j in range(ce)], dtype=z.dtype)
            loss = loss * a.view(shape)
    else:
        bce = F.binary_cross_entropy_with_logits(z, y, reduction="none")
        loss = bce * (F.logsigmoid(-z * (2.0 * y - 1.0)) * gamma).exp()
        if alpha is not None:
            loss = loss * (alpha * y + (1.0 - alpha) * (1.0 - y))
    if weight is not None:
        w = torch.as_tensor(weight, dtype=z.dtype)
        loss = loss * (w.repeat(ce) if w.ndim == 0 else w).view(shape)
    if reduction == "mean":
        return loss.mean()
    return loss.mean(dim=list(range(2, z.dim()))).sum()           # "sum": over (n, c) of the spatial mean


def dice_focal_loss(z, t, lambda_dice=1.0, lambda_focal=1.0, gamma=2.0, alpha=None, weight=None, include_background=True,
                    to_onehot_y=False, sigmoid=False, softmax=False, squared_pred=False, jaccard=False, batch=False, reduction="mean"):
    d = O.dice_loss(z, t, sigmoid, batch, squared_pred, include_background=include_background, softmax=softmax, to_onehot_y=to_onehot_y,
                    jaccard=jaccard, weight=weight, reduction=reduction)
    f = focal_loss(z, t, gamma, alpha, weight, include_background, to_onehot_y, softmax, reduction)
    return lambda_dice * d + lambda_focal * f


def tversky_loss(z, t, alpha=0.5, beta=0.5, sigmoid=False, softmax=False, to_onehot_y=False, include_background=True, batch=False,
                 reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5):
    c = z.shape[1]
    p = torch.sigmoid(z) if sigmoid else z
    if softmax and c > 1:
        p = torch.softmax(p, 1)
    y = _onehot(z, t) if (to_onehot_y and c > 1) else t.to(p.dtype)
    if not include_background:
        p, y = p[:, 1:], y[:, 1:]
    axes = ([0] if batch else []) + list(range(2, p.dim()))
    tp, fp, fn = (p * y).sum(axes), (p * (1 - y)).sum(axes), ((1 - p) * y).sum(axes)
    f = 1.0 - (tp + smooth_nr) / (tp + alpha * fp + beta * fn + smooth_dr)
    if reduction == "mean":
        return f.mean()
    if reduction == "sum":
        return f.sum()
    return f.view(list(f.shape) + [1] * (z.dim() - 2))


def data(n, c, dhw, name="", seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, *dhw, generator=g) * 2
    t = C.nested_masks(n, dhw, seed)[:, :c] if c <= 3 else (torch.rand(n, c, *dhw, generator=g) > 0.6).to(torch.uint8)
    if "labels" in name:                             # class-index target [N, 1, ...]
        t = torch.randint(0, c, (n, 1) + tuple(dhw), generator=torch.Generator().manual_seed(5))
    if "float_target" in name:                       # any float in [0, 1]
        t = torch.rand(n, c, *dhw, generator=g)
    return z, t


def check(crit, ref_fn, be, dev, n, c, dhw, name=""):
    """tests/test_losses.py's _check: scalar output, upstream factor 3.0, value and gradient to TOL. Returns what a hostile-memory row
    compares bit for bit."""
    z, t = data(n, c, dhw, name)
    zr = z.clone().requires_grad_(True)
    ref = ref_fn(zr, t)
    ref.backward()
    if be is not None:
        crit._be = be
    zg = z.to(dev).requires_grad_(True)
    loss = crit(zg, t.to(dev))
    (loss * 3.0).backward()
    assert loss.dim() == 0
    lv, rv = float(loss.detach()), float(ref.detach())
    print(f"{name}: loss {lv:.8g} ref {rv:.8g} rel {abs(lv - rv) / abs(rv):.3g} grad rel {C.rel_err(zg.grad, 3.0 * zr.grad):.3g}")
    assert abs(lv - rv) / abs(rv) < TOL
    assert C.rel_err(zg.grad, 3.0 * zr.grad) < TOL
    return loss.detach().reshape(1), zg.grad


def check_none(kw, be, dev, n, c, dhw, name=""):
    """reduction="none": one value per term, a different upstream gradient for every term (tests/test_losses.py's _check_ex)"""
    z, t = data(n, c, dhw, name, seed=3)
    zr = z.clone().requires_grad_(True)
    ref = tversky_loss(zr, t, **kw)
    up = torch.rand(ref.shape, generator=torch.Generator().manual_seed(7)) + 0.5
    (ref * up).sum().backward()
    crit = losses.HipTverskyLoss(**kw)
    if be is not None:
        crit._be = be
    zg = z.to(dev).requires_grad_(True)
    loss = crit(zg, t.to(dev))
    assert loss.shape == ref.shape
    (loss * up.to(dev)).sum().backward()
    assert C.rel_err(loss.detach().cpu(), ref.detach()) < TOL
    assert C.rel_err(zg.grad.cpu(), zr.grad) < TOL
    return loss.detach(), zg.grad


L = losses
W3 = [0.2, 1.0, 3.0]
# (id [words in it select the data: labels / float_target], module, restatement, channels)
CASES = [
    ("focal_g2", lambda: L.HipFocalLoss(), lambda z, t: focal_loss(z, t), 3),
    ("focal_g0_is_bce", lambda: L.HipFocalLoss(gamma=0.0), lambda z, t: F.binary_cross_entropy_with_logits(z, t.float()), 3),
    ("focal_g1.5_alpha", lambda: L.HipFocalLoss(gamma=1.5, alpha=0.25), lambda z, t: focal_loss(z, t, 1.5, 0.25), 3),
    ("focal_weight", lambda: L.HipFocalLoss(weight=W3), lambda z, t: focal_loss(z, t, weight=W3), 3),
    ("focal_nobg", lambda: L.HipFocalLoss(include_background=False), lambda z, t: focal_loss(z, t, include_background=False), 3),
    ("focal_sum", lambda: L.HipFocalLoss(reduction="sum"), lambda z, t: focal_loss(z, t, reduction="sum"), 3),
    ("focal_softmax_labels", lambda: L.HipFocalLoss(use_softmax=True, to_onehot_y=True),
     lambda z, t: focal_loss(z, t, use_softmax=True, to_onehot_y=True), 4),
    ("focal_softmax_labels_alpha", lambda: L.HipFocalLoss(use_softmax=True, to_onehot_y=True, alpha=0.25),
     lambda z, t: focal_loss(z, t, alpha=0.25, use_softmax=True, to_onehot_y=True), 4),
    ("focal_softmax_labels_nobg", lambda: L.HipFocalLoss(use_softmax=True, to_onehot_y=True, include_background=False),
     lambda z, t: focal_loss(z, t, use_softmax=True, to_onehot_y=True, include_background=False), 4),
    ("focal_float_target", lambda: L.HipFocalLoss(gamma=2.0, alpha=0.4), lambda z, t: focal_loss(z, t, 2.0, 0.4), 3),
    ("focal_1ch", lambda: L.HipFocalLoss(), lambda z, t: focal_loss(z, t), 1),
    ("dicefocal", lambda: L.HipDiceFocalLoss(sigmoid=True), lambda z, t: dice_focal_loss(z, t, sigmoid=True), 3),
    ("dicefocal_softmax_labels", lambda: L.HipDiceFocalLoss(softmax=True, to_onehot_y=True),
     lambda z, t: dice_focal_loss(z, t, softmax=True, to_onehot_y=True), 4),
    ("dicefocal_lambdas_batch", lambda: L.HipDiceFocalLoss(sigmoid=True, lambda_dice=0.3, lambda_focal=2.0, batch=True),
     lambda z, t: dice_focal_loss(z, t, 0.3, 2.0, sigmoid=True, batch=True), 3),
    ("dicefocal_jaccard_sum", lambda: L.HipDiceFocalLoss(sigmoid=True, jaccard=True, reduction="sum"),
     lambda z, t: dice_focal_loss(z, t, sigmoid=True, jaccard=True, reduction="sum"), 3),
    ("dicefocal_weight", lambda: L.HipDiceFocalLoss(sigmoid=True, weight=W3), lambda z, t: dice_focal_loss(z, t, sigmoid=True, weight=W3), 3),
    ("dicefocal_lambda_dice_0", lambda: L.HipDiceFocalLoss(sigmoid=True, lambda_dice=0.0, gamma=1.0),
     lambda z, t: focal_loss(z, t, gamma=1.0), 3),
    ("tversky_half_half", lambda: L.HipTverskyLoss(sigmoid=True), lambda z, t: tversky_loss(z, t, sigmoid=True), 3),
    ("tversky_03_07", lambda: L.HipTverskyLoss(sigmoid=True, alpha=0.3, beta=0.7), lambda z, t: tversky_loss(z, t, 0.3, 0.7, sigmoid=True), 3),
    ("tversky_batch", lambda: L.HipTverskyLoss(sigmoid=True, alpha=0.3, beta=0.7, batch=True),
     lambda z, t: tversky_loss(z, t, 0.3, 0.7, sigmoid=True, batch=True), 3),
    ("tversky_softmax_labels", lambda: L.HipTverskyLoss(softmax=True, to_onehot_y=True, alpha=0.6, beta=0.4),
     lambda z, t: tversky_loss(z, t, 0.6, 0.4, softmax=True, to_onehot_y=True), 4),
    ("tversky_nobg", lambda: L.HipTverskyLoss(sigmoid=True, alpha=0.3, beta=0.7, include_background=False),
     lambda z, t: tversky_loss(z, t, 0.3, 0.7, sigmoid=True, include_background=False), 3),
]
IDS = [c[0] for c in CASES]
NONE_KW = dict(sigmoid=True, alpha=0.3, beta=0.7, reduction="none")


def case(name):
    return next(c for c in CASES if c[0] == name)


# ---- hostile-memory rows (tests/scratch_guard.hold): one per new entry point -----------------------------------------------------------
def row_module(name, dhw):
    _, mk, ref, c = case(name)
    return lambda be: check(mk(), ref, be, be.device.type, 2, c, dhw, name)


def row_focal_onto_dice(dhw):
    """the op layer, as tests/op_cases.case_ce runs the CE pass: 0.7 * Dice, then 0.4 * focal accumulated onto value and gradient"""
    def run(be):
        z, t = data(2, 3, dhw, seed=11)
        zr = z.clone().requires_grad_(True)
        ref = 0.7 * O.dice_loss(zr, t, True) + 0.4 * focal_loss(zr, t, 1.5, 0.25)
        (dz_ref,) = torch.autograd.grad(ref, zr)
        zd, td = C.dev(be, z), C.dev(be, t)
        loss, dz = be.dice(zd, td, True, grad_scale=0.7)
        loss.mul_(0.7)
        loss, dz = be.focal(zd, td, gamma=1.5, alpha=0.25, weight=0.4, loss=loss, dlogits=dz)
        assert abs(float(loss.cpu()) - float(ref.detach())) / abs(float(ref.detach())) < TOL
        assert C.rel_err(dz, dz_ref) < TOL
        return loss, dz
    return run


def row_tversky_none(dhw):
    return lambda be: check_none(NONE_KW, be, be.device.type, 2, 3, dhw)


def rows(dhw):
    """id -> (case(be), fills): focal sigmoid, focal softmax with labels, focal accumulating onto Dice, Tversky forward + backward"""
    import scratch_guard as G
    return {"focal_sigmoid": (row_module("focal_g1.5_alpha", dhw), (G.QNAN, G.ONES)),
            "focal_nobg": (row_module("focal_nobg", dhw), (G.QNAN, G.ONES)),               # channel 0 of the gradient is written too
            "focal_softmax_labels": (row_module("focal_softmax_labels_alpha", dhw), (G.QNAN, G.ONES)),
            "focal_onto_dice": (row_focal_onto_dice(dhw), (G.QNAN, G.ONES)),
            "tversky": (row_module("tversky_03_07", dhw), (G.QNAN, G.ONES)),
            "tversky_none": (row_tversky_none(dhw), (G.QNAN, G.ONES))}
