"""TEST INFRASTRUCTURE: cases of the residual-block kernels (csrc/res_block.hip: mi355_res_join_fwd / _bwd, mi355_conv1x1_s2_fwd / _wgrad /
_dgrad_add) and of HipDynUNet / HipDynUNetDS with res_block=True, shared by the emulator tests (tests/test_res_block.py) and their GPU
twins (tests/test_res_block_gpu.py).

OP LEVEL. Inputs are drawn as stream_form_cases draws them (values the storage type holds exactly, ld > c views with POISON around them, a
NaN sample behind the tensors a kernel reads, fenced fp32 outputs) and every op is judged against a float64 evaluation of its formula on the
values the kernel read (the statistics, scale and shift are the float64 ones rounded once to the fp32 the kernel is handed; the backward's
mask is taken from the A the forward stored); nothing is compared with another run of the library.
  join forward / backward: launch_audit.store_err <= stream_form_cases.BOUND (1e-5, what gn_act_bwd is held to), the half-ulp allowance the
    storage type's. JOIN crosses 4 / 12 / 100 (no multiple of 16) / 320 channels, the three storage types, the extents (1, 1, 2), (3, 5, 7) =
    105 voxels and (1, 3, 11) = 33 voxels -- the first pass gives a workgroup at least 16 voxels (RJ_MIN_VOXELS_PER_BLOCK), so 33 is the
    smallest plane with two partial records per (n, c): the cross-workgroup sum runs (105: six) --, outputs at channel offset c of a 2c-wide
    buffer, and gamma with a zero and negative entries. 16-bit cases with c % 8 == 0 take the 8-channel-per-lane kernels, the others the
    4-channel ones. The backward runs twice: once into a d_r2 of its own, once with d_r2 = dA in place (what the engine does); both must
    give the same bits.
  shortcut conv: store_err <= 1e-5, the bound tests/test_launch_audit.py::BOUNDS gives conv_fwd and conv_wgrad (tests/test_res_block.py
    asserts the two numbers are the same). For dgrad_add the reference is float64(before) + WT d_r3 on the even voxels and `before`
    elsewhere, where the bits must not have changed. SHORTCUT crosses 4->8, 12->16, 64->96, 256->384 with outputs (3, 5, 7) from (6, 10, 14)
    and (1, 1, 1) from (2, 2, 2) and the three storage types. Weight gradient and dgrad_add run twice: same bits.

NETWORK LEVEL. The oracle is a plain-torch restatement of MONAI's DynUNet(res_block=True) [MONAI-memory, parity unpinned, like
oracle/dynunet_ref.py on which it is built]: UnetResBlock in the input block, every down-sampling block, the bottleneck and every up block's
conv_block. Judged as tests/test_dynunet.py::_pair judges the plain model (logits and loss 1e-3, gradients by op_cases.grad_parity with
conditioning.noise_floor); with heads, as tests/deep_supervision_cases.py::pair does.
"""
import ctypes
import importlib
import os

import torch

import deep_supervision_cases as DS
import launch_audit as A
import op_cases as C
import stream_form_cases as SF
from oracle import conditioning, dynunet_ref as D, torch_ops as O, unet3d_ref as R

ops = importlib.import_module("3dunetcnn_amd.ops")
dyn = importlib.import_module("3dunetcnn_amd.dynunet")
losses = importlib.import_module("3dunetcnn_amd.losses")
optim = importlib.import_module("3dunetcnn_amd.optim")
F32, BF16, F16 = SF.F32, SF.BF16, SF.F16
TOL = 1e-3
CONV_BOUND = 1e-5                 # tests/test_launch_audit.py::BOUNDS["conv_fwd"] == BOUNDS["conv_wgrad"]
SLOPE = 0.01
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4

# id -> (storage, channels, dhw, output at channel offset c of a 2c-wide buffer)
JOIN = {
    "f32-c4-v2": (F32, 4, (1, 1, 2), False),
    "bf16-c4-v33": (BF16, 4, (1, 3, 11), False),
    "f16-c12-v105": (F16, 12, (3, 5, 7), False),
    "f32-c12-v33": (F32, 12, (1, 3, 11), False),
    "bf16-c12-v2": (BF16, 12, (1, 1, 2), True),
    "f32-c100-v105-offset": (F32, 100, (3, 5, 7), True),
    "bf16-c100-v33": (BF16, 100, (1, 3, 11), False),
    "f16-c100-v2": (F16, 100, (1, 1, 2), False),
    "f32-c320-v33": (F32, 320, (1, 3, 11), False),
    "bf16-c320-v105-offset": (BF16, 320, (3, 5, 7), True),
    "f16-c320-v33-offset": (F16, 320, (1, 3, 11), True),
    "f16-c16-v105": (F16, 16, (3, 5, 7), False),
}
# id -> (storage, cin, cout, output dhw)
SHORTCUT = {
    "f32-4-8-v105": (F32, 4, 8, (3, 5, 7)),
    "bf16-4-8-v1": (BF16, 4, 8, (1, 1, 1)),
    "f16-12-16-v105": (F16, 12, 16, (3, 5, 7)),
    "f32-12-16-v1": (F32, 12, 16, (1, 1, 1)),
    "bf16-64-96-v105": (BF16, 64, 96, (3, 5, 7)),
    "f16-64-96-v1": (F16, 64, 96, (1, 1, 1)),
    "f32-64-96-v105": (F32, 64, 96, (3, 5, 7)),
    "f32-256-384-v105": (F32, 256, 384, (3, 5, 7)),
    "bf16-256-384-v1": (BF16, 256, 384, (1, 1, 1)),
    "f16-256-384-v105": (F16, 256, 384, (3, 5, 7)),
}


def _gamma(c, g):
    """Affine weights with a zero and negative entries among them."""
    ga = torch.randn(c, generator=g)
    ga[0], ga[1], ga[c - 1] = 0.0, -0.75, -abs(float(ga[c - 1])) - 0.1
    return ga


def _bc(t):
    return t.double()[:, :, None, None, None]


def join_case(be, dtype, c, dhw, offset, seed=21):
    """mi355_res_join_fwd and mi355_res_join_bwd on one pair of raw tensors. Returns what the ops wrote (scratch_guard.hold compares it)."""
    g = torch.Generator().manual_seed(seed)
    n, shape = 2, (2, c, *dhw)
    V = dhw[0] * dhw[1] * dhw[2]
    r2 = SF.act(be, SF.values(shape, g, dtype, 1.7, 0.4), dtype, c + 8, 8, guard=True)
    r3 = SF.act(be, SF.values(shape, g, dtype, 1.3, -0.2), dtype, c + 16, 8, guard=True)
    ga2, ga3 = _gamma(c, g), _gamma(c, g)
    be2, be3 = torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.3
    x2, x3 = SF.widen(r2), SF.widen(r3)
    st = []
    for xv, ga, bt in ((x2, ga2, be2), (x3, ga3, be3)):
        mean, rstd, scale, shift = SF.stats_oracle(xv, c, ga, bt)
        st.append((torch.stack((mean, rstd), -1).float(), scale.float(), shift.float()))       # what the kernels read: rounded once
    dst = [tuple(SF.dev(be, t) for t in s) for s in st]
    slope = float(torch.tensor(SLOPE, dtype=F32))
    view = (2 * c, c) if offset else (c + 8, 0)
    what = f"res_join {dtype} C={c} {dhw} offset={offset}"
    # forward
    a = SF.out_act(be, shape, dtype, *view)
    be.res_join_fwd(r2, dst[0], r3, dst[1], a, SLOPE)
    u = x2 * _bc(st[0][1]) + _bc(st[0][2]) + x3 * _bc(st[1][1]) + _bc(st[1][2])
    SF.bounded(A.store_err(SF.widen(a), torch.maximum(u, u * slope), dtype), what + " A")
    SF.outside_untouched(a)
    # backward: the mask from the A the forward stored
    av = SF.widen(a)
    dA_first = SF.values(shape, g, dtype)
    gr = dA_first.double() * torch.where(av > 0, 1.0, slope)
    refs = []
    for xv, (mr, _, _), ga in ((x2, st[0], ga2), (x3, st[1], ga3)):
        mean, rstd = _bc(mr[..., 0]), _bc(mr[..., 1])
        xh = (xv - mean) * rstd
        s0, s1 = gr.sum((2, 3, 4), keepdim=True), (gr * xh).sum((2, 3, 4), keepdim=True)
        refs.append((ga.double()[None, :, None, None, None] * rstd * (gr - s0 / V - xh * s1 / V), s1.sum(0).flatten(), s0.sum(0).flatten()))
    runs = []
    for inplace in (False, True):
        dA = SF.act(be, dA_first, dtype, *view, guard=True)
        d2 = dA if inplace else SF.out_act(be, shape, dtype, *view)
        d3 = SF.out_act(be, shape, dtype, c + 8, 8)
        params = [DS.fenced(be, (c,)) for _ in range(4)]
        be.res_join_bwd(a, dA, r2, dst[0], SF.dev(be, ga2), r3, dst[1], SF.dev(be, ga3), d2, d3, *(p[0] for p in params), SLOPE)
        for _, fence in params:
            fence()
        SF.outside_untouched(d2), SF.outside_untouched(d3)
        if not inplace:
            SF.same_bits(dA.tensor(), dA_first.permute(0, 2, 3, 4, 1).to(dtype), what + ": dA was written")
        runs.append([d2.tensor(), d3.tensor()] + [p[0] for p in params])
    d2, d3, dg2, db2, dg3, db3 = runs[0]
    for name, got, ref, dt in (("d_r2", d2, refs[0][0], dtype), ("d_r3", d3, refs[1][0], dtype)):
        SF.bounded(A.store_err(got.detach().cpu().double().permute(0, 4, 1, 2, 3), ref, dt), f"{what} {name}")
    for name, got, ref in (("dgamma2", dg2, refs[0][1]), ("dbeta2", db2, refs[0][2]), ("dgamma3", dg3, refs[1][1]), ("dbeta3", db3, refs[1][2])):
        SF.bounded(A.store_err(got, ref, F32), f"{what} {name}")
    for i, (x_, y_) in enumerate(zip(*runs)):
        SF.same_bits(x_, y_, f"{what}: output {i} of the in-place second run")
    for t in (r2, r3, a):
        SF.outside_untouched(t)
    return [a.tensor()] + runs[0]


def shortcut_case(be, dtype, cin, cout, out_dhw, seed=31):
    """mi355_conv1x1_s2_fwd, _wgrad and _dgrad_add on one input. Returns what the ops wrote."""
    g = torch.Generator().manual_seed(seed)
    n = 2
    fine = tuple(2 * s for s in out_dhw)
    x = SF.act(be, SF.values((n, cin, *fine), g, dtype), dtype, cin + 4, 4, guard=True)
    w = torch.randn(cout, cin, 1, 1, 1, generator=g) * 0.2
    wd, w2 = SF.dev(be, w), w.double().reshape(cout, cin)
    what = f"conv1x1_s2 {dtype} {cin}->{cout} {out_dhw}"
    xe = SF.widen(x)[:, :, ::2, ::2, ::2]
    y = SF.out_act(be, (n, cout, *out_dhw), dtype, cout + 8, 8)
    be.conv1x1_s2_fwd(x, wd, y)
    SF.bounded(A.store_err(SF.widen(y), torch.einsum("ncdhw,kc->nkdhw", xe, w2), dtype), what + " y", CONV_BOUND)
    SF.outside_untouched(y)
    dy = SF.act(be, SF.values((n, cout, *out_dhw), g, dtype), dtype, cout + 4, 4, guard=True)
    dyv = SF.widen(dy)
    before = SF.values((n, cin, *fine), g, dtype)
    ref_dx = before.double().clone()
    ref_dx[:, :, ::2, ::2, ::2] += torch.einsum("nkdhw,kc->ncdhw", dyv, w2)
    odd = torch.ones(fine, dtype=torch.bool)
    odd[::2, ::2, ::2] = False
    runs = []
    for _ in range(2):
        dw, fence = DS.fenced(be, (cout, cin, 1, 1, 1))
        be.conv1x1_s2_wgrad(x, dy, dw)
        fence()
        dx = SF.act(be, before, dtype, cin + 8, 8, guard=True)
        be.conv1x1_s2_dgrad_add(dy, wd, dx)
        SF.outside_untouched(dx)
        runs.append((dw, dx.tensor()))
    dw, dxt = runs[0]
    SF.bounded(A.store_err(dw.reshape(cout, cin), torch.einsum("nkdhw,ncdhw->kc", dyv, xe), F32), what + " dw", CONV_BOUND)
    got_dx = dxt.detach().cpu().permute(0, 4, 1, 2, 3)
    SF.bounded(A.store_err(got_dx.double(), ref_dx, dtype), what + " dx", CONV_BOUND)
    SF.same_bits(got_dx[:, :, odd], before.to(dtype)[:, :, odd], what + ": a voxel that is not even on all three axes changed")
    for i, (x_, y_) in enumerate(zip(*runs)):
        SF.same_bits(x_, y_, f"{what}: output {i} of the second run")
    SF.outside_untouched(x), SF.outside_untouched(dy)
    return [y.tensor(), dw, dxt]


def _plain(be, shape5, fill=0.0, dtype=F32):
    n, c, d, h, w = shape5
    return ops.Act(torch.full((n, d, h, w, c), fill, dtype=dtype).to(be.device), 0, c)


def refusals(be):
    """Every refused call of the five entry points: its status, nothing launched (the emulator's launch record), nothing written; then the
    same calls with valid arguments and the scratch at its exact size."""
    lib, st = be.lib, be.stream()
    n, cin, cout, out_dhw = 1, 8, 12, (1, 2, 3)
    fine = tuple(2 * s for s in out_dhw)
    x, y, dx = _plain(be, (n, cin, *fine), 1.0), _plain(be, (n, cout, *out_dhw), 5.0), _plain(be, (n, cin, *fine), 5.0)
    w = torch.ones(cout, cin).to(be.device)
    dw = torch.full((cout, cin), 5.0).to(be.device)
    xd, yd = x.desc(), y.desc()
    need = lib.mi355_conv1x1_s2_scratch_bytes(ctypes.byref(xd), ctypes.byref(yd))
    assert need == cin * cout * 4 and lib.mi355_conv1x1_s2_scratch_bytes(None, ctypes.byref(yd)) == 0
    ws = torch.zeros(need // 4 + 16).to(be.device)

    def conv(xv=x, yv=y, dxv=dx, ws_bytes=need):
        a, b, c_ = (None if v is None else v.desc() for v in (xv, yv, dxv))
        ref = lambda d_: None if d_ is None else ctypes.byref(d_)        # noqa: E731
        return (lib.mi355_conv1x1_s2_fwd(ref(a), w.data_ptr(), ref(b), st), lib.mi355_conv1x1_s2_wgrad(ref(a), ref(b), dw.data_ptr(), ws.data_ptr(), ws_bytes, st),
                lib.mi355_conv1x1_s2_dgrad_add(ref(b), w.data_ptr(), ref(c_), st))
    SF.take(be)
    odd = _plain(be, (n, cin, 2, 4, 5), 1.0)
    got = {"odd": conv(xv=odd, dxv=odd), "null": conv(xv=None, dxv=None), "short": conv(ws_bytes=need - 4)}
    bad = ops.MiAct(x.ptr(), n, *fine, 6, 8, 0)              # a view of 6 channels: ops.Act itself refuses to build one
    got["c6"] = (lib.mi355_conv1x1_s2_fwd(ctypes.byref(bad), w.data_ptr(), ctypes.byref(yd), st),
                 lib.mi355_conv1x1_s2_wgrad(ctypes.byref(bad), ctypes.byref(yd), dw.data_ptr(), ws.data_ptr(), need, st),
                 lib.mi355_conv1x1_s2_dgrad_add(ctypes.byref(yd), w.data_ptr(), ctypes.byref(bad), st))
    wide = _plain(be, (n, 388, *fine), 1.0)
    big_w = torch.ones(cout, 388).to(be.device)
    wided = wide.desc()
    got["c388"] = (lib.mi355_conv1x1_s2_fwd(ctypes.byref(wided), big_w.data_ptr(), ctypes.byref(yd), st),
                   lib.mi355_conv1x1_s2_wgrad(ctypes.byref(wided), ctypes.byref(yd), big_w.data_ptr(), ws.data_ptr(), 1 << 30, st),
                   lib.mi355_conv1x1_s2_dgrad_add(ctypes.byref(yd), big_w.data_ptr(), ctypes.byref(wided), st))
    want = {"odd": (EINVAL,) * 3, "c6": (EINVAL,) * 3, "null": (EINVAL,) * 3, "short": (0, EWORKSPACE, 0), "c388": (EUNSUPPORTED,) * 3}
    launched = SF.take(be)
    assert got == want, got
    assert launched is None or launched == ["(c1s2_gemm_kernel<T, 1>)", "(c1s2_gemm_kernel<T, 0>)"], launched      # the two valid calls of "short"
    assert bool((dw == 5.0).all()) and bool((ws == 0).all()) and bool((big_w == 1.0).all()), "a refused weight gradient wrote"
    y.buf.fill_(5.0), dx.buf.fill_(5.0)
    SF.take(be)
    # the join
    c, dhw = 8, (1, 3, 11)
    t = {k: _plain(be, (2, c, *dhw), 5.0 if k in ("a", "d2", "d3") else 1.0) for k in ("r2", "r3", "a", "da", "d2", "d3")}
    vec = torch.ones(2 * 2 * c * 2 + 8).to(be.device)
    sc = vec[:2 * c]
    outs = torch.full((4, c), 5.0).to(be.device)
    ad = t["a"].desc()
    jneed = lib.mi355_res_join_scratch_bytes(ctypes.byref(ad))
    assert jneed == (2 * 2 * c * 3 + 2 * c * 6) * 8 and lib.mi355_res_join_scratch_bytes(None) == 0          # 33 voxels: two records per (n, c)
    jws = torch.zeros(jneed // 4 + 16).to(be.device)

    def jf(r2=t["r2"], a=t["a"], scale=sc):
        d_ = [None if v is None else v.desc() for v in (r2, t["r3"], a)]
        ref = lambda v: None if v is None else ctypes.byref(v)          # noqa: E731
        return lib.mi355_res_join_fwd(ref(d_[0]), ref(d_[1]), scale.data_ptr(), sc.data_ptr(), sc.data_ptr(), sc.data_ptr(), SLOPE, ref(d_[2]), st)

    def jb(a=t["a"], d3=t["d3"], ws_bytes=jneed):
        d_ = [None if v is None else v.desc() for v in (a, t["da"], t["r2"], t["r3"], t["d2"], d3)]
        ref = lambda v: None if v is None else ctypes.byref(v)          # noqa: E731
        return lib.mi355_res_join_bwd(ref(d_[0]), ref(d_[1]), ref(d_[2]), ref(d_[3]), SLOPE, sc.data_ptr(), vec.data_ptr(), sc.data_ptr(), vec.data_ptr(),
                                      ref(d_[4]), ref(d_[5]), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                      jws.data_ptr(), ws_bytes, st)
    other = _plain(be, (2, c, 1, 3, 10), 1.0)
    half = _plain(be, (2, c, *dhw), 1.0, BF16)
    got = {"null_fwd": jf(a=None), "null_bwd": jb(a=None), "shape_fwd": jf(r2=other), "shape_bwd": jb(d3=other), "type_fwd": jf(r2=half),
           "type_bwd": jb(d3=half), "scale_unaligned": jf(scale=vec[1:2 * c + 1]), "short": jb(ws_bytes=jneed - 4), "alias": jb(d3=t["r3"])}
    want = dict.fromkeys(got, EINVAL)
    want.update(type_fwd=EUNSUPPORTED, type_bwd=EUNSUPPORTED, short=EWORKSPACE)
    assert got == want, got
    assert not SF.take(be), "a refused call launched a kernel"
    assert all(bool((t[k].buf == 5.0).all()) for k in ("a", "d2", "d3")) and bool((outs == 5.0).all()) and bool((jws == 0).all())
    # valid arguments, scratch at its exact size
    assert conv() == (0, 0, 0) and jf() == 0 and jb() == 0
    assert bool((ws[need // 4:] == 0).all()) and bool((jws[jneed // 4:] == 0).all()), "wrote past the scratch it asked for"
    assert not bool((dw == 5.0).any()) and not bool((outs == 5.0).any()) and not bool((t["d3"].buf == 5.0).any())


# ---- network ---------------------------------------------------------------------------------------------------------------------------
def kw(filters, K=0, **more):
    return dict(DS.kw(filters, K), res_block=True, **more)


def _res_block(sd, pre, x, stride):
    """MONAI UnetResBlock with cin != cout or stride != 1, as a function of a state dict. Every call goes through D.F (oracle.conditioning
    perturbs that namespace)."""
    out = D.F.conv3d(x, sd[pre + ".conv1.conv.weight"], None, stride=stride, padding=1)
    out = D.F.leaky_relu(D.F.instance_norm(out, None, None, sd[pre + ".norm1.weight"], sd[pre + ".norm1.bias"], True, 0.1, 1e-5), 0.01)
    out = D.F.conv3d(out, sd[pre + ".conv2.conv.weight"], None, stride=1, padding=1)
    out = D.F.instance_norm(out, None, None, sd[pre + ".norm2.weight"], sd[pre + ".norm2.bias"], True, 0.1, 1e-5)
    res = D.F.conv3d(x, sd[pre + ".conv3.conv.weight"], None, stride=stride)
    res = D.F.instance_norm(res, None, None, sd[pre + ".norm3.weight"], sd[pre + ".norm3.bias"], True, 0.1, 1e-5)
    return D.F.leaky_relu(out + res, 0.01)


def res_dynunet_forward(sd, x, n_levels, K=0):
    """DynUNet(res_block=True)(x); K > 0: the training-mode stack of DynUNet(res_block=True, deep_supervision=True, deep_supr_num=K)."""
    skips = [_res_block(sd, "input_block", x, 1)]
    for i in range(n_levels - 2):
        skips.append(_res_block(sd, f"downsamples.{i}", skips[-1], 2))
    x = _res_block(sd, "bottleneck", skips[-1], 2)
    level_out = {}
    for k in range(n_levels - 1):
        lvl = n_levels - 2 - k
        x = D.F.conv_transpose3d(x, sd[f"upsamples.{k}.transp_conv.conv.weight"], None, stride=2)
        x = torch.cat((x, skips[lvl]), 1)
        x = level_out[lvl] = _res_block(sd, f"upsamples.{k}.conv_block", x, 1)
    out = D.F.conv3d(x, sd["output_block.conv.conv.weight"], sd["output_block.conv.conv.bias"])
    if not K:
        return out
    heads = [D.F.conv3d(level_out[i + 1], sd[f"deep_supervision_heads.{i}.conv.conv.weight"], sd[f"deep_supervision_heads.{i}.conv.conv.bias"])
             for i in range(K)]
    return torch.stack([out] + [D.F.interpolate(h, out.shape[2:]) for h in heads], dim=1)


def restatement_parameter_count(cin, cout, filters):
    """Parameters of the restated network, counted from its structure (no module of the package involved)."""
    def block(ci, co):
        return 27 * ci * co + 27 * co * co + ci * co + 6 * co
    L = len(filters)
    total = block(cin, filters[0]) + sum(block(filters[i - 1], filters[i]) for i in range(1, L))
    total += sum(8 * filters[i + 1] * filters[i] + block(2 * filters[i], filters[i]) for i in range(L - 1))
    return total + filters[0] * cout + cout


def make_criterion(K):
    inner = losses.HipDiceLoss(sigmoid=True)
    return losses.HipDeepSupervisionLoss(inner) if K else inner


def pair(m, be, dhw, n, dev):
    """Kernels vs the CPU oracle graph, as tests/test_dynunet.py::_pair (K == 0) and tests/deep_supervision_cases.py::pair (heads)."""
    L = len(m.filters)
    K = m.deep_supr_num if getattr(m, "deep_supervision", False) else 0
    x, y = R.synthetic_case(n, 4, dhw, 3)
    torch.set_num_threads(min(32, os.cpu_count() or 1))

    def run(dt):
        sd = {k: v.detach().cpu().clone().to(dt).requires_grad_(True) for k, v in m.named_parameters()}
        ref = res_dynunet_forward(sd, x.to(dt), L, K)
        l = DS.oracle_loss(ref, y) if K else O.dice_loss(ref, y)
        l.backward()
        return ref.detach(), l.detach(), {k: v.grad for k, v in sd.items()}
    ref, lref, g32 = run(torch.float32)
    _, _, g64 = run(torch.float64)
    floor, perturbed = conditioning.noise_floor(D, lambda: run(torch.float32)[2], return_evals=True)
    crit = make_criterion(K)
    DS.bind(be, m, crit)
    if be is not None:
        crit._be = be
    out = m(x.to(dev))
    assert tuple(out.shape) == ((n, 1 + K, 3) if K else (n, 3)) + tuple(dhw)
    loss = crit(out, y.to(dev))
    loss.backward()
    errs = {"logits": C.rel_err(out, ref), "loss": abs(float(loss.detach()) - float(lref)) / abs(float(lref))}
    w = C.grad_parity({k: p.grad for k, p in m.named_parameters()}, g32, g64, floor, TOL, perturbed=perturbed)
    errs["grad"] = w.pop("ratio")
    errs.update(w)
    return errs


def step_case(be, dev, filters=(8, 12, 16), dhw=(4, 8, 4), seed=7):
    """One training step of the residual network; what scratch_guard.hold compares across runs."""
    torch.manual_seed(seed)
    m = dyn.HipDynUNet(**kw(list(filters))).to(dev).train()
    crit = make_criterion(0)
    DS.bind(be, m, crit)
    crit._be = be
    x, y = (t.to(dev) for t in R.synthetic_case(1, 4, dhw, 3))
    out = m(x)
    loss = crit(out, y)
    loss.backward()
    return [out.detach(), loss.detach().reshape(1)] + [p.grad for p in m.parameters()]
