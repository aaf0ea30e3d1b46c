"""TEST INFRASTRUCTURE: cases of the deep-supervision heads (csrc/deep_supervision.hip: mi355_ds_head_fwd / mi355_ds_head_bwd), of
HipDynUNetDS and of HipDeepSupervisionLoss, shared by the emulator tests (tests/test_deep_supervision.py) and their GPU twins
(tests/test_deep_supervision_gpu.py).

OP LEVEL. Inputs are drawn as stream_form_cases.proj_case draws them (values the storage type holds exactly, ld > c views with POISON
around them) and both ops are judged against a float64 evaluation of the operation on the values the kernel read; nothing is compared
with another run of the library. Criterion: launch_audit.store_err <= 1e-5 (stream_form_cases.BOUND, the projection's bound in
tests/test_launch_audit.py::BOUNDS); for the accumulated dx the reference is float64(dx_before) + wT pool(dout) and store_err's half-ulp
allowance is the storage type's. The forward additionally requires the factor^3 fine voxels of a coarse voxel to be bit-identical.
CASES cross: cin 4 / 100 (past the projection's 96-channel cap, no multiple of 16) / 320 (the cap); cout 1 / 3 / 8; the three storage
types; prologue and bias on and off; dx present and NULL; factor 2 on (3, 5, 7) = 105 coarse voxels (above the kernel's 32-voxel tile,
ragged last tile), factor 4 on (2, 3, 5) = 30 and factor 16 on (1, 2, 3) = 6 (below it); and one case each for factor 8 and 32, whose
rows are 2 and 8 sixteen-byte pieces per coarse voxel.

NETWORK LEVEL. The oracle is a plain-torch restatement of MONAI's DynUNet(deep_supervision=True) forward [MONAI-memory, parity
unpinned, like oracle/dynunet_ref.py on which it is built]: heads on the up blocks' outputs, F.interpolate (nearest), torch.stack(dim=1);
loss oracle sum_l w_l * oracle.torch_ops.dice_loss(out[:, l], y). Judged as tests/test_dynunet.py::_pair judges the plain model.
"""
import ctypes
import importlib

import torch

import launch_audit as A
import op_cases as C
import stream_form_cases as SF
from oracle import conditioning, dynunet_ref as D, torch_ops as O, unet3d_ref as R

ops = importlib.import_module("3dunetcnn_amd.ops")
_lib = importlib.import_module("3dunetcnn_amd._lib")
dyn = importlib.import_module("3dunetcnn_amd.dynunet")
losses = importlib.import_module("3dunetcnn_amd.losses")
optim = importlib.import_module("3dunetcnn_amd.optim")
F32, BF16, F16 = SF.F32, SF.BF16, SF.F16
TOL = 1e-3
EINVAL, EWORKSPACE = -1, -4

# id -> (storage, cin, cout, coarse dhw, factor, bias, prologue, with_dx)
CASES = {
    "f32-c4-k1-f2": (F32, 4, 1, (3, 5, 7), 2, True, True, True),
    "bf16-c100-k3-f2": (BF16, 100, 3, (3, 5, 7), 2, False, True, True),
    "f16-c320-k8-f2": (F16, 320, 8, (3, 5, 7), 2, True, False, True),
    "f32-c100-k8-f4-nodx": (F32, 100, 8, (2, 3, 5), 4, True, True, False),
    "bf16-c320-k3-f4": (BF16, 320, 3, (2, 3, 5), 4, True, True, True),
    "f16-c4-k3-f4": (F16, 4, 3, (2, 3, 5), 4, False, False, True),
    "f32-c320-k3-f16": (F32, 320, 3, (1, 2, 3), 16, True, True, True),
    "bf16-c4-k8-f16-nodx": (BF16, 4, 8, (1, 2, 3), 16, True, False, False),
    "f16-c100-k1-f16": (F16, 100, 1, (1, 2, 3), 16, False, True, True),
    "f32-c8-k2-f8": (F32, 8, 2, (2, 3, 2), 8, True, True, True),
    "f32-c4-k1-f32": (F32, 4, 1, (1, 1, 2), 32, True, False, True),
    "f32-c320-k8-f32": (F32, 320, 8, (1, 1, 2), 32, True, True, True),          # every limit at once: the largest LDS tile of both kernels
}
REFUSALS = {"cin324": (324, 3, 2), "cin6": (6, 3, 2), "cout9": (8, 9, 2), "factor1": (8, 3, 1), "factor3": (8, 3, 3), "factor64": (8, 3, 64)}


def fenced(be, shape):
    """A contiguous fp32 device tensor of NaN the op must overwrite completely, followed in the same allocation by 64 POISON values it must
    not touch -> (tensor, check)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 64,), float("nan"))
    buf[numel:] = SF.POISON
    buf = buf.to(be.device)

    def check():
        assert bool((buf[numel:].cpu() == SF.POISON).all()), "wrote past the end of its output"
    return buf[:numel].view(shape), check


def upsampled(t, f):
    return t.repeat_interleave(f, 2).repeat_interleave(f, 3).repeat_interleave(f, 4)


def pooled(t, f):
    n, k, d, h, w = t.shape
    return t.reshape(n, k, d // f, f, h // f, f, w // f, f).sum((3, 5, 7))


def head_case(be, dtype, cin, cout, dhw, factor, bias, prologue, with_dx, seed=11):
    """mi355_ds_head_fwd and mi355_ds_head_bwd on one input. Returns what the ops wrote (scratch_guard.hold compares it across runs)."""
    g = torch.Generator().manual_seed(seed)
    n = 2
    x = SF.act(be, SF.values((n, cin, *dhw), g, dtype), dtype, cin + 4, 4)
    w = torch.randn(cout, cin, generator=g) * 0.2
    b = torch.randn(cout, generator=g) if bias else None
    sc = torch.rand(n, cin, generator=g) + 0.5 if prologue else None
    sh = torch.randn(n, cin, generator=g) * 0.3 if prologue else None
    slope = 0.01
    pk = dict(scale=SF.dev(be, sc), shift=SF.dev(be, sh), slope=slope) if prologue else {}
    fine = tuple(s * factor for s in dhw)
    dz = torch.randn(n, cout, *fine, generator=g)
    t = SF.widen(x)
    if prologue:
        u = t * sc.double()[:, :, None, None, None] + sh.double()[:, :, None, None, None]
        t = torch.maximum(u, u * float(torch.tensor(slope, dtype=F32)))
    what = f"ds_head {dtype} {cin}->{cout} {dhw} x{factor} bias={bias} prologue={prologue} dx={with_dx}"
    # forward
    out, out_fence = fenced(be, (n, cout, *fine))
    be.ds_head_fwd(x, SF.dev(be, w), SF.dev(be, b), out, factor, **pk)
    ref = torch.einsum("ncdhw,kc->nkdhw", t, w.double())
    if bias:
        ref = ref + b.double()[None, :, None, None, None]
    SF.bounded(A.store_err(out, upsampled(ref, factor), F32), what + " out")
    oc = out.cpu()
    assert torch.equal(oc, upsampled(oc[:, :, ::factor, ::factor, ::factor], factor)), what + ": the fine voxels of one coarse voxel differ"
    out_fence()
    # backward, twice: bitwise reproducible
    runs = []
    dx_first = SF.values((n, cin, *dhw), g, dtype) if with_dx else None      # what the level's gradient holds before the head adds to it
    for _ in range(2):
        dx = SF.act(be, dx_first, dtype, cin + 8, 8) if with_dx else None
        dw, dw_fence = fenced(be, (cout, cin))
        dbias, db_fence = fenced(be, (cout,)) if bias else (None, lambda: None)
        be.ds_head_bwd(x, SF.dev(be, w), SF.dev(be, dz), dx, dw, dbias, factor, **pk)
        dw_fence(), db_fence()
        runs.append((dw, dbias, dx))
    dw, dbias, dx = runs[0]
    pz = pooled(dz.double(), factor)
    SF.bounded(A.store_err(dw, torch.einsum("nkdhw,ncdhw->kc", pz, t), F32), what + " dw")
    got = [out, dw]
    if bias:
        SF.bounded(A.store_err(dbias, pz.sum((0, 2, 3, 4)), F32), what + " dbias")
        got.append(dbias)
    if with_dx:
        SF.bounded(A.store_err(SF.widen(dx), dx_first.double() + torch.einsum("nkdhw,kc->ncdhw", pz, w.double()), dtype), what + " dx")
        SF.outside_untouched(dx)
        got.append(dx.tensor())
    for a_, b_ in zip(runs[0], runs[1]):
        if a_ is not None:
            SF.same_bits(a_.tensor() if hasattr(a_, "buf") else a_, b_.tensor() if hasattr(b_, "buf") else b_, what + " second run")
    SF.outside_untouched(x)
    return got


def refusal(be, cin, cout, factor):
    """(status of mi355_ds_head_fwd, of mi355_ds_head_bwd) for a call whose only fault is (cin, cout, factor)."""
    n, dhw = 1, (2, 2, 2)
    x = ops.Act(torch.zeros(n, *dhw, cin).to(be.device), 0, cin)
    fine = tuple(s * max(factor, 1) for s in dhw)
    out = torch.zeros(n, cout, *fine).to(be.device)
    w, b = torch.zeros(cout, cin).to(be.device), torch.zeros(cout).to(be.device)
    dw, db = torch.zeros(cout, cin).to(be.device), torch.zeros(cout).to(be.device)
    ws = torch.zeros(1 << 18).to(be.device)
    xd = x.desc()
    rf = be.lib.mi355_ds_head_fwd(ctypes.byref(xd), None, None, 0.0, w.data_ptr(), b.data_ptr(), out.data_ptr(), cout, factor, be.stream())
    rb = be.lib.mi355_ds_head_bwd(ctypes.byref(xd), None, None, 0.0, w.data_ptr(), out.data_ptr(), None, dw.data_ptr(), db.data_ptr(), cout,
                                  factor, ws.data_ptr(), ws.numel() * 4, be.stream())
    return rf, rb


def abi_contract(be):
    """The parts of the C ABI no network call reaches: the scratch query of a NULL view is 0; a workspace one float short is
    MI355_STATUS_EWORKSPACE and the exact size is taken; a scale / shift that is not 16-byte aligned (the prologue reads four channels per
    load) and an fp32 pointer that is not 4-byte aligned are MI355_STATUS_EINVAL. Every refused call launches nothing and writes nothing."""
    n, dhw, cin, cout, factor = 2, (3, 5, 7), 8, 3, 2
    g = torch.Generator().manual_seed(3)
    x = ops.Act(torch.randn(n, *dhw, cin, generator=g).to(be.device), 0, cin)
    fine = tuple(s * factor for s in dhw)
    dz = torch.randn(n, cout, *fine, generator=g).to(be.device)
    w, b = (torch.randn(cout, cin, generator=g) * 0.2).to(be.device), torch.randn(cout, generator=g).to(be.device)
    pro = torch.rand(2 * n * cin + 8, generator=g).to(be.device) + 0.5            # scale | shift, with room to shift them by one float
    sc, sh = pro[:n * cin], pro[n * cin:2 * n * cin]
    sc1, sh1 = pro[1:n * cin + 1], pro[n * cin + 1:2 * n * cin + 1]
    assert sc.data_ptr() % 16 == 0 and sh.data_ptr() % 16 == 0 and sc1.data_ptr() % 16 == 4
    xd = x.desc()
    assert be.lib.mi355_ds_head_scratch_bytes(None, cout) == 0
    need = be.lib.mi355_ds_head_scratch_bytes(ctypes.byref(xd), cout)
    tiles = n * -(-(dhw[0] * dhw[1] * dhw[2]) // 32)
    assert 0 < need <= tiles * (cout * cin + cout) * 4 and need % 4 == 0, need
    ws = torch.zeros(need // 4 + 16).to(be.device)
    out = torch.full((n, cout, *fine), 5.0).to(be.device)
    dw, db = torch.full((cout, cin), 5.0).to(be.device), torch.full((cout,), 5.0).to(be.device)

    def fwd(scale=sc, shift=sh, weight=w.data_ptr(), bias=b.data_ptr()):
        return be.lib.mi355_ds_head_fwd(ctypes.byref(xd), scale.data_ptr(), shift.data_ptr(), 0.01, weight, bias, out.data_ptr(), cout, factor,
                                        be.stream())

    def bwd(ws_bytes=need, scale=sc, shift=sh, dwp=dw.data_ptr(), dbp=db.data_ptr()):
        return be.lib.mi355_ds_head_bwd(ctypes.byref(xd), scale.data_ptr(), shift.data_ptr(), 0.01, w.data_ptr(), dz.data_ptr(), None, dwp, dbp,
                                        cout, factor, ws.data_ptr(), ws_bytes, be.stream())
    SF.take(be)
    got = dict(short_ws=bwd(ws_bytes=need - 4), no_ws=bwd(ws_bytes=0), scale_bwd=bwd(scale=sc1), shift_bwd=bwd(shift=sh1),
               dw=bwd(dwp=dw.data_ptr() + 2), dbias=bwd(dbp=db.data_ptr() + 1), scale_fwd=fwd(scale=sc1), shift_fwd=fwd(shift=sh1),
               w_fwd=fwd(weight=w.data_ptr() + 2), bias_fwd=fwd(bias=b.data_ptr() + 1))
    want = dict.fromkeys(got, EINVAL)
    want.update(short_ws=EWORKSPACE, no_ws=EWORKSPACE)
    assert got == want, got
    assert not SF.take(be), "a refused call launched a kernel"                 # (the emulator's launch list; None on a device)
    assert bool((out == 5.0).all()) and bool((dw == 5.0).all()) and bool((db == 5.0).all()) and bool((ws == 0).all())
    assert fwd() == 0 and bwd() == 0                      # the same calls with valid arguments, the workspace at its exact size
    assert bool((ws[need // 4:] == 0).all()), "wrote past the workspace it asked for"
    assert bool(torch.isfinite(out).all()) and not bool((dw == 5.0).any()) and not bool((db == 5.0).any())


class audited_heads:
    """with audited_heads(be) as seen: every Backend.ds_head_bwd call inside (a network's backward, whatever its storage type) is held to
    the op-level criterion on the tensors the network really handed it: dw, dbias and the sum left in dx against float64 from the same x,
    prologue, weight, slot gradient and dx-before, store_err <= BOUND. `seen` counts the calls."""

    def __init__(self, be):
        self.be, self.seen = be, []

    def __enter__(self):
        be, inner = self.be, self.be.ds_head_bwd

        def audited(x, w, dout, dx, dw, dbias, factor, scale=None, shift=None, slope=0.0):
            before = SF.widen(dx)
            inner(x, w, dout, dx, dw, dbias, factor, scale, shift, slope)
            t = SF.widen(x)
            if scale is not None:
                u = t * scale.cpu().double()[:, :, None, None, None] + shift.cpu().double()[:, :, None, None, None]
                t = torch.maximum(u, u * float(torch.tensor(slope, dtype=F32)))
            pz = pooled(dout.cpu().double(), factor)
            what = f"network ds_head_bwd {x.dtype} {x.c}->{w.shape[0]} x{factor}"
            SF.bounded(A.store_err(dw, torch.einsum("nkdhw,ncdhw->kc", pz, t), F32), what + " dw")
            SF.bounded(A.store_err(dbias, pz.sum((0, 2, 3, 4)), F32), what + " dbias")
            SF.bounded(A.store_err(SF.widen(dx), before + torch.einsum("nkdhw,kc->ncdhw", pz, w.cpu().double()), x.dtype), what + " dx")
            self.seen.append((x.dtype, x.c, factor))
        be.ds_head_bwd = audited
        return self.seen

    def __exit__(self, *exc):
        del self.be.ds_head_bwd                          # the instance attribute: the class's method is back


# ---- network ---------------------------------------------------------------------------------------------------------------------------
def kw(filters, K=1, **more):
    L = len(filters)
    return dict(spatial_dims=3, in_channels=4, out_channels=3, kernel_size=[3] * L, strides=[1] + [2] * (L - 1),
                upsample_kernel_size=[2] * (L - 1), filters=filters, deep_supervision=K > 0, deep_supr_num=max(K, 1), **more)


def dynunet_ds_forward(sd, x, n_levels, K):
    """MONAI DynUNet(deep_supervision=True, deep_supr_num=K).train()(x) as a function of a state dict: oracle.dynunet_ref's forward with
    the K heads on the outputs of the up blocks at levels 1 .. K, nearest-up-sampled and stacked behind the logits. Every torch.nn.functional
    call goes through D.F, so oracle.conditioning's perturbations reach the heads too."""
    skips = [D._basic_block(sd, "input_block", x, 1)]
    for i in range(n_levels - 2):
        skips.append(D._basic_block(sd, f"downsamples.{i}", skips[-1], 2))
    x = D._basic_block(sd, "bottleneck", skips[-1], 2)
    level_out = {}
    for k in range(n_levels - 1):
        lvl = n_levels - 2 - k
        x = D.F.conv_transpose3d(x, sd[f"upsamples.{k}.transp_conv.conv.weight"], None, stride=2)
        x = torch.cat((x, skips[lvl]), 1)
        x = level_out[lvl] = D._basic_block(sd, f"upsamples.{k}.conv_block", x, 1)
    out = D.F.conv3d(x, sd["output_block.conv.conv.weight"], sd["output_block.conv.conv.bias"])
    heads = [D.F.conv3d(level_out[i + 1], sd[f"deep_supervision_heads.{i}.conv.conv.weight"], sd[f"deep_supervision_heads.{i}.conv.conv.bias"])
             for i in range(K)]
    return torch.stack([out] + [D.F.interpolate(h, out.shape[2:]) for h in heads], dim=1)


def ds_weights(levels, mode="exp"):
    """monai.losses.DeepSupervisionLoss.get_weights, restated."""
    return [{"exp": max(0.5 ** l, 0.0625), "same": 1.0, "two": 1.0 if l == 0 else 0.5}[mode] for l in range(levels)]


def oracle_loss(stack, y, mode="exp"):
    return sum(w * O.dice_loss(stack[:, l], y) for l, w in enumerate(ds_weights(stack.shape[1], mode)))


def bind(be, *mods):
    for m in mods:
        if be is not None:
            m._be = be
            if hasattr(m, "loss"):
                m.loss._be = be


def pair(m, be, dhw, n, dev):
    """Kernels vs the CPU oracle graph (tests/test_dynunet.py::_pair with the stacked output and the deep-supervision loss)."""
    import os
    L, K = len(m.filters), m.deep_supr_num
    x, y = R.synthetic_case(n, 4, dhw, 3)
    torch.set_num_threads(min(32, os.cpu_count() or 1))

    def run(dt):
        sd = {k: v.detach().cpu().clone().to(dt).requires_grad_(True) for k, v in m.named_parameters()}
        ref = dynunet_ds_forward(sd, x.to(dt), L, K)
        l = oracle_loss(ref, y)
        l.backward()
        return ref.detach(), l.detach(), {k: v.grad for k, v in sd.items()}
    ref, lref, g32 = run(torch.float32)
    _, _, g64 = run(torch.float64)
    floor, perturbed = conditioning.noise_floor(D, lambda: run(torch.float32)[2], return_evals=True)
    crit = losses.HipDeepSupervisionLoss(losses.HipDiceLoss(sigmoid=True))
    bind(be, m, crit)
    out = m(x.to(dev))
    assert tuple(out.shape) == (n, 1 + K, 3) + tuple(dhw) and all(out[:, l].is_contiguous() for l in range(1 + K))
    loss = crit(out, y.to(dev))
    loss.backward()
    errs = {"logits": C.rel_err(out, ref), "loss": abs(float(loss.detach()) - float(lref)) / abs(float(lref))}
    w = C.grad_parity({k: p.grad for k, p in m.named_parameters()}, g32, g64, floor, TOL, perturbed=perturbed)
    errs["grad"] = w.pop("ratio")
    errs.update(w)
    return errs


def train_step(m, crit, x, y, opt=None):
    """One step; returns (loss, {name: gradient clone})."""
    if opt is not None:
        opt.zero_grad(set_to_none=True)
    loss = crit(m(x), y)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    if opt is not None:
        opt.step()
    return loss.detach(), grads
