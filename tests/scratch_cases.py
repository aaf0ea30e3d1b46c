"""TEST INFRASTRUCTURE: the rows tests/test_scratch_emu.py and tests/test_scratch_gpu.py run under tests/scratch_guard.py, and the
table of which row covers which entry point of include/mi355_unet3d.h.

A row is (id, case, configuration, fills). The case is an existing case of the shared tables (op_cases, act_storage_cases,
augment_cases, components_cases, the checks of test_losses / test_prepost) at a shape those tables already use, with its own assertion:
the same cases on hostile memory, not new shapes. ROWS run on both backends (the emulator's small shapes cost nothing on the GPU);
GPU_ROWS add, per route, the smallest shape of tests/test_ops_gpu.py / test_wino_gpu.py that reaches its multi-chunk / multi-workgroup
path. Rows about one kernel or entry point assert that it ran (_wino_was_routed, _calls, _launches): a silent fall-back fails the row.
Networks: HipUNet3D in its default configuration on the GPU, a reduced one on the emulator (UNET_REDUCED says why), the smallest HipDynUNet. Fills: QNAN everywhere; ONES in addition where a route has integer scratch or outputs (components, label maps, index targets)
and on the whole-network cases.

COVERAGE: every entry point of the header that takes a workspace, writes records, or writes an output the Python layer allocates with
`empty` -> the rows that reach it (test_scratch_emu.py::test_every_size_query_has_a_row fails when the header gains a `_workspace(` /
`_blocks(` query without an entry here, and when an entry names a row that does not exist). Left out on purpose, having neither scratch
nor an `empty` output: mi355_adam_step (in-place on four caller tensors), the pure queries (`*_supported`, `*_config`, `*_elems`,
`*_bytes_bf16`, `mi355_conv3d_uses_bf16`), mi355_pack_weights_batch (rewrites packs in place; the single-weight pack entry points it
must agree with are covered through every conv row: PackedWeight allocates its packs with `empty`), mi355_sw_accumulate (the
one-window form; the inferer runs the batch form), and the stream test (no memory of its own).
"""
import ctypes
import importlib

import torch

import act_storage_cases as S
import augment_cases as A
import components_cases as K
import op_cases as C
from scratch_guard import ONES, QNAN

TOL = C.TOL
BF16_TOL = {"bf16x3": 1e-4, "bf16x6": 5e-6, "bf16": 3e-2, "fp16": 4e-3}      # tests/test_ops_emu.py
DIRECT = dict(winograd=False, wgrad_form="direct")
WINO = lambda form: dict(winograd=True, wino_form=form, WINO_MIN_VOXELS=0)      # noqa: E731 -- product routing, size threshold lifted
WGRAD_WINO = dict(wgrad_form="wino", WINO_MIN_VOXELS=0)


def below(r, tol=TOL, **special):
    """The case's own bound on every error it returns (NaN fails `<`)."""
    items = r.items() if isinstance(r, dict) else [("err", r)]
    bad = {k: v for k, v in items if not isinstance(v, bool) and not v < special.get(k, tol)}
    assert not bad, (bad, r)


def B(case, tol=TOL, **special):
    """case(be) -> errors, held to `tol`."""
    return lambda be: below(case(be), tol, **special)


def _zring(form, splits, prec="bf16"):
    return dict(precision=prec, env={"MI355_BF16_FORM": form, "MI355_BF16_ZSPLITS": splits}, **DIRECT)


def _fused(r):
    assert r["gnb_fused"]
    return r


def _prepost(be):
    import test_prepost as TP
    dev = be.device.type
    TP._cases(dev, be, (6, 7, 9))
    TP._resample_cases(dev, be, (6, 7, 9))
    # the assertions above are test_prepost's; what is compared bit for bit between the clean and the guarded run:
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(4, 6, 7, 9, generator=g) * 3 + 1).to(be.device)
    probs, lab = be.postprocess(x[:3].contiguous(), "softmax", 0.5, [2, 1, 4], True)
    oh = be.one_hot(torch.randint(0, 5, (6, 7, 9), generator=g).float().to(be.device), [[2, 1], [4]])
    rs = be.resample_affine(x, (9, 5, 11), [0.6, 0.1, 0, 0.2, 0, 1.3, 0, -0.4, 0.05, 0, 0.8, 0.3], "trilinear", "zeros")
    return [be.zscore(x), probs, lab, oh, rs]


def _dice_ex(name):
    import test_losses as TL
    kw, c, labels = next((r[1], r[2], r[3]) for r in TL.EX_CASES if r[0] == name)
    return lambda be: TL._check_ex(kw, be, be.device.type, 2, c, (9, 8, 10), labels)


def _loss(name):
    import test_losses as TL
    mk, ref, c = next((r[1], r[2], r[3]) for r in TL.CASES if r[0] == name)
    return lambda be: TL._check(mk(), ref, be, be.device.type, 2, c, (9, 8, 10), name)


def _cast(be):
    S.case_cast(be)                            # exact against torch's own rounding
    x = C.to_act(be, torch.randn(2, 8, 3, 5, 7, generator=torch.Generator().manual_seed(0)) * 5.0, ld=12, c0=4)
    y = be.cast(x, torch.bfloat16)
    h = be.cast(x, torch.float16)
    return [y.tensor(), h.tensor(), be.cast(y, torch.float32).tensor()]


def _components(dhw, k, c=2, p=0.31):
    prepost = importlib.import_module("3dunetcnn_amd.prepost")

    def run(be):
        mask = K.random_mask(c, dhw, p, seed=100 * c + 3)
        labels, ref = K.check_labels(be, mask, k, prepost)
        keep = K.check_filter(be, mask, k, True, 0, ref, labels)
        small = K.check_filter(be, mask, k, False, 3, ref, labels)
        return labels, keep, small
    return run


def _ensemble(be):
    """Both paths of mi355_ensemble_threshold: 16-byte vectors (5 x 6 x 8) and the scalar one (3 x 5 x 7)."""
    out = []
    for dhw in ((5, 6, 8), (3, 5, 7)):
        p = K.probabilities(5, 2, dhw, seed=5)
        ref = p.double().mean(dim=0)
        mean, mask = be.ensemble_threshold(p.to(be.device), 0.5)
        assert float((mean.cpu().double() - ref).abs().max()) <= 1e-6 and torch.equal(mask.cpu(), (ref >= 0.5).to(torch.uint8))
        out += [mean, mask]
    return out


def _augment(normalize):
    def run(be):
        n, ci, cl, dhw = 2, 4, 3, A.EXTENTS[0]
        img, lab = A.make_batch(n, ci, cl, dhw, torch.uint8, 7)
        m = A.as_m(A.interp_maps(dhw, n)[3])
        g = torch.linspace(0.9, 1.1, n * ci).view(n, ci)
        o = torch.linspace(-0.1, 0.1, n * ci).view(n, ci)
        return A.check_against_oracle(be, be.device, img, lab, m, g, o, dhw, "zeros", normalize, what="scratch")
    return run


def _inferer(be):
    import test_inferer as TI
    from oracle import sliding_window_ref as SW
    inferer = importlib.import_module("3dunetcnn_amd.inferer")
    x = torch.randn(2, 4, 11, 16, 9, generator=torch.Generator().manual_seed(1))
    inf = inferer.HipSlidingWindowInferer((8, 8, 8), sw_batch_size=3, overlap=0.25, mode="gaussian")
    inf._be = be
    got = inf(x.to(be.device), TI._predictor())
    ref = SW.sliding_window_inference(x, (8, 8, 8), 3, TI._predictor(), 0.25, "gaussian")
    assert C.rel_err(got, ref) < 1e-6


def _records_reduce(be):
    """More epilogue records than Backend.RECORDS_MAX: mi355_gn_records_reduce folds them before the statistics are finalised (the
    threshold is lowered instead of the shape raised: the fold's index logic does not depend on the count)."""
    old = (be.RECORDS_MAX, be.RECORDS_FOLD)
    be.RECORDS_MAX, be.RECORDS_FOLD = 4, 3
    try:
        below(C.case_conv_moments(be, 2, 8, 32, (5, 6, 9)), 2e-5)
        below(C.case_gn_bwd_fused(be, 2, 32, 32, (5, 6, 9)), 2e-5)
    finally:
        del be.RECORDS_MAX, be.RECORDS_FOLD
        assert (be.RECORDS_MAX, be.RECORDS_FOLD) == old


UNET_DEFAULT = dict(n_features=4, n_outputs=3)          # HipUNet3D as tests/test_model_gpu.py runs it: base width 32, blocks [1, 2, 2, 4], up to 256 channels
# The emulator's network is a REDUCED configuration: three levels, at most 64 channels, at 14 x 15 x 13. Reason: cost. One row is four
# emulated training steps on one CPU worker; this reduced network at 30 x 31 x 29 measured 340 s, and the default configuration has a
# fourth level, twice the width and twice the blocks on top of that. The reduced row keeps every kind of buffer a network allocates
# (empty_act, concat halves, records, dx / dw, the fused first-layer backward) at an odd extent. What it does not reach -- the fourth
# level, the multi-block levels, the >= 256-channel routes -- the GPU rows do: they run UNET_DEFAULT.
UNET_REDUCED = dict(n_features=4, n_outputs=3, base_width=16, encoder_blocks=[1, 1, 2])


def _unet(kw, dhw, n, conv_precision=None, storage=None):
    """One forward + backward of HipUNet3D(**kw): logits, loss and every gradient are returned, so the harness holds them to bit identity;
    their values are tests/test_model_gpu.py's and test_launch_audit.py's business."""
    unet = importlib.import_module("3dunetcnn_amd.unet")
    losses = importlib.import_module("3dunetcnn_amd.losses")
    from oracle import unet3d_ref as R
    made = {}                                  # backend -> (model, data): the clean and the guarded runs of one hold() share the weights

    def run(be):
        if id(be) not in made:
            torch.manual_seed(0)
            m = unet.HipAutocastUNet(autocast_dtype=conv_precision, activation_storage=storage, **kw) if storage else unet.HipUNet3D(**kw)
            m = m.to(be.device).eval()
            m._be = be
            made[id(be)] = (be, m, R.synthetic_case(n, 4, dhw, 3))
        _, m, (x, y) = made[id(be)]
        crit = losses.HipDiceLoss(sigmoid=True)
        crit._be = be
        m.zero_grad(set_to_none=True)
        out = m(x.to(be.device))
        loss = crit(out, y.to(be.device))
        loss.backward()
        res = [out.detach().float(), loss.detach()] + [p.grad for p in m.parameters()]
        assert all(bool(torch.isfinite(t).all()) for t in res)
        return res
    return run


def _dynunet(be):
    import test_dynunet as TD
    dyn = importlib.import_module("3dunetcnn_amd.dynunet")
    losses = importlib.import_module("3dunetcnn_amd.losses")
    from oracle import unet3d_ref as R
    torch.manual_seed(5)
    m = dyn.HipDynUNet(**TD._kw([8, 12, 16])).to(be.device).eval()
    m._be = be
    crit = losses.HipDiceLoss(sigmoid=True)
    crit._be = be
    x, y = R.synthetic_case(2, 4, (8, 12, 8), 3)
    out = m(x.to(be.device))
    loss = crit(out, y.to(be.device))
    loss.backward()
    res = [out.detach(), loss.detach()] + [p.grad for p in m.parameters()]
    assert all(bool(torch.isfinite(t).all()) for t in res)
    return res


def _wino_was_routed(case):
    """The row is about the Winograd kernels: fail if product routing did not take the call there."""
    def run(be):
        calls, orig = [], be.conv_fwd_wino
        be.conv_fwd_wino = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            r = case(be)
        finally:
            del be.conv_fwd_wino
        assert calls, "the call did not reach the Winograd kernel"
        return r
    return run


def _calls(entry, case):
    """The row is about one library entry point (Backend.conv_wgrad falls back to the direct kernel silently when the Winograd
    workspace query answers 0): fail if the case never called it."""
    def run(be):
        calls, orig = [], getattr(be.lib, entry)
        setattr(be.lib, entry, lambda *a: (calls.append(1), orig(*a))[1])
        try:
            r = case(be)
        finally:
            setattr(be.lib, entry, orig)
        assert calls, f"the case did not call {entry}"
        return r
    return run


def _launches(prefix, case, entry="mi355_conv3d_fwd", exclude=None):
    """The row is about one kernel (an environment switch or a storage type selects it): fail unless some launch of `entry` in the case is
    one whose configuration query (mi355_conv3d_fwd_config / _wgrad_config: the name a trace shows) starts with `prefix`."""
    def run(be):
        names, orig, config = [], getattr(be.lib, entry), getattr(be.lib, entry + "_config")
        buf = ctypes.create_string_buffer(96)

        def launch(*a):
            config(a[0], a[2] if entry == "mi355_conv3d_fwd" else a[1], a[3], buf, 96)
            names.append(buf.value.decode())
            return orig(*a)
        setattr(be.lib, entry, launch)
        try:
            r = case(be)
        finally:
            setattr(be.lib, entry, orig)
        assert any(k.startswith(prefix) and not (exclude and k.startswith(exclude)) for k in names), (prefix, names)
        return r
    return run


# id -> (case(be), configuration for scratch_guard.configured, fills)
ROWS = {}


def row(rid, case, cfg=None, fills=(QNAN,)):
    assert rid not in ROWS, rid
    ROWS[rid] = (case, cfg or {}, fills)


# ---- convolution forward / dgrad, direct kernels -----------------------------------------------------------------------------------
row("fwd_generic", B(lambda be: C.case_conv_fwd(be, 1, 8, 32, (6, 7, 9))), DIRECT)
row("fwd_generic_epilogue_slice", B(lambda be: C.case_conv_fwd(be, 1, 32, 32, (6, 6, 8), norm=True, yld=64, yc0=32, residual=True, chscale=True)), DIRECT)
row("fwd_s2c32", B(lambda be: C.case_conv_fwd(be, 1, 32, 32, (9, 10, 12), stride=2)), DIRECT)
row("fwd_s2_generic", B(lambda be: C.case_conv_fwd(be, 2, 8, 64, (8, 8, 8), stride=2, norm=True, slope=0.01)), DIRECT)
row("fwd_k1", B(lambda be: C.case_conv_fwd(be, 2, 64, 32, (5, 6, 7), kd=1)), DIRECT)
row("fwd_k1_bias", B(lambda be: C.case_conv_fwd(be, 1, 32, 64, (9, 6, 7), kd=1, bias=True)), DIRECT)
row("fwd_c4", B(lambda be: C.case_conv_fwd(be, 1, 4, 32, (7, 6, 10), norm=True, xld=8, yld=64, yc0=32, residual=True, chscale=True)), DIRECT)
row("fwd_narrow", B(lambda be: C.case_conv_fwd(be, 2, 8, 4, (4, 9, 8), yld=8, yc0=4)), DIRECT)
row("dgrad_generic", B(lambda be: C.case_conv_dgrad(be, 1, 32, 64, (6, 7, 8))), DIRECT)
row("dgrad_s2c32", B(lambda be: C.case_conv_dgrad(be, 1, 32, 32, (10, 9, 16), stride=2, residual=True)), DIRECT)
row("dgrad_zero_insert_generic", B(lambda be: C.case_conv_dgrad(be, 1, 64, 32, (6, 8, 10), stride=2, residual=True)), DIRECT)
row("dgrad_first_layer", B(lambda be: C.case_conv_dgrad(be, 2, 4, 32, (5, 9, 11))), DIRECT)
row("tconv_k3s2", B(lambda be: C.case_tconv3(be, 1, 32, 32, (4, 5, 6))), DIRECT)
row("tconv_k3s2_window", B(lambda be: C.case_tconv3(be, 2, 16, 64, (3, 4, 4), pad_to=(6, 8, 8))), DIRECT)
row("tconv_k2s2", B(lambda be: C.case_tconv2(be, 2, 32, 32, (3, 4, 5))), DIRECT)                      # D2S forward, S2D dgrad, D2S wgrad
row("tconv_k2s2_wide", B(lambda be: C.case_tconv2(be, 1, 64, 36, (2, 2, 3), norm=False, yld=72)), DIRECT)
row("cat_slope", B(lambda be: C.case_conv_cat_slope(be, 1, 32, 32, 64, (5, 6, 7), stride=2)), DIRECT)
# ... with the fused statistics (records sized by mi355_conv3d_stats_blocks)
row("moments_generic", B(lambda be: C.case_conv_moments(be, 2, 8, 32, (5, 6, 9)), 2e-5), DIRECT)
row("moments_2x2_waves", B(lambda be: C.case_conv_moments(be, 1, 16, 64, (3, 5, 8), residual=True, chscale=True), 2e-5), DIRECT)
row("moments_partial_tile", B(lambda be: C.case_conv_moments(be, 1, 8, 40, (4, 4, 8), groups_out=40), 2e-5), DIRECT)
row("moments_c4", B(lambda be: C.case_conv_moments(be, 1, 4, 32, (5, 9, 9)), 2e-5), DIRECT)
row("moments_s2c32", B(lambda be: C.case_conv_moments(be, 1, 32, 32, (9, 8, 8), stride=2, norm=False), 2e-5), DIRECT)
row("moments_slice", B(lambda be: C.case_conv_moments(be, 1, 8, 32, (4, 4, 8), yld=64, yc0=32), 2e-5), DIRECT)
row("cat_moments", B(lambda be: C.case_cat_moments(be, 2, 8, 24, (3, 5, 8)), 2e-5), DIRECT)             # gn_moments + gn_finalize from two producers
row("gnb_generic", B(lambda be: C.case_gn_bwd_fused(be, 2, 32, 32, (5, 6, 9)), 2e-5), DIRECT)
row("gnb_two_n_tiles", B(lambda be: C.case_gn_bwd_fused(be, 1, 64, 16, (3, 5, 8), slope=0.01), 2e-5), DIRECT)
row("gnb_partial_tile", B(lambda be: C.case_gn_bwd_fused(be, 1, 40, 8, (4, 4, 8), groups=40), 2e-5), DIRECT)
row("records_reduce", _records_reduce, DIRECT)
row("stats_unfused", lambda be: (below(C.case_conv_moments(be, 1, 8, 32, (4, 4, 8), expect_fused=False), 2e-5),
                                 below(C.case_gn_bwd_fused(be, 1, 32, 32, (4, 4, 8), expect_fused=False), 2e-5))[0], dict(fused_stats=False, **DIRECT))
# ---- Winograd forms (product routing with the size threshold lifted) ---------------------------------------------------------------
for _f in ("2d", "3d"):
    row(f"wino{_f}_fwd", _wino_was_routed(B(lambda be: C.case_conv_fwd(be, 1, 16, 64, (3, 9, 19), norm=True, residual=True, chscale=True), 1e-5)), WINO(_f))
    row(f"wino{_f}_fwd_slice", _wino_was_routed(B(lambda be: C.case_conv_fwd(be, 1, 8, 64, (4, 4, 16), norm=True, yld=128, yc0=32), 1e-5)), WINO(_f))
    row(f"wino{_f}_dgrad", _wino_was_routed(B(lambda be: C.case_conv_dgrad(be, 1, 32, 64, (3, 4, 18)), 1e-5)), WINO(_f))
    row(f"wino{_f}_moments", _wino_was_routed(B(lambda be: C.case_conv_moments(be, 1, 32, 32, (3, 5, 19), residual=True, chscale=True), 2e-5)), WINO(_f))
    row(f"wino{_f}_gnb", _wino_was_routed(B(lambda be: C.case_gn_bwd_fused(be, 1, 32, 32, (3, 5, 19)), 2e-4)), WINO(_f))
# ---- precision modes of the 3x3x3 stride-1 kernels ----------------------------------------------------------------------------------
for _p in ("bf16x3", "bf16", "fp16"):
    _c = dict(precision=_p, **DIRECT)
    row(f"{_p}_fwd", B(lambda be: C.case_conv_fwd(be, 1, 32, 32, (3, 5, 19), norm=True, residual=True, chscale=True), BF16_TOL[_p]), _c)
    row(f"{_p}_fwd_c4", B(lambda be: C.case_conv_fwd(be, 1, 4, 48, (3, 4, 5), bias=True, yld=64, yc0=16), BF16_TOL[_p]), _c)
    row(f"{_p}_dgrad", B(lambda be: C.case_conv_dgrad(be, 1, 32, 64, (3, 4, 18)), BF16_TOL[_p]), _c)
    row(f"{_p}_wgrad", B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (3, 5, 18), norm=True), BF16_TOL[_p]), _c)
    row(f"{_p}_wgrad_splits", B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (5, 8, 32), norm=True), BF16_TOL[_p]), _c)      # 40 tiles in 5 splits
    row(f"{_p}_moments", B(lambda be, t=BF16_TOL[_p]: C.case_conv_moments(be, 1, 16, 64, (4, 4, 16), yld=128, yc0=32, ytol=t, strict_vs_oracle=False), 2e-5), _c)
    row(f"{_p}_gnb", B(lambda be: C.case_gn_bwd_fused(be, 1, 32, 32, (3, 5, 19), compare_unfused=True), 2e-5), _c)
# ---- plane-ring forms of the 16-bit forward / dgrad: the z-range split is where a slot can stay unwritten ---------------------------
ZR2, ZR = "conv3d_k3_lp_zring2", "conv3d_k3_lp_zring"       # the kernels MI355_BF16_FORM=zring / zring1 select (tests/test_routing_emu.py)
for _form, _k, _x in (("zring", ZR2, None), ("zring1", ZR, ZR2)):
    for _s in ("2", "5"):
        _c, _t = _zring(_form, _s), BF16_TOL["bf16"]
        row(f"{_form}_z{_s}_fwd", _launches(_k, B(lambda be: C.case_conv_fwd(be, 1, 20, 32, (9, 8, 32), norm=True, slope=0.01, yld=64, yc0=32), _t), exclude=_x), _c)
        row(f"{_form}_z{_s}_fwd_22planes", _launches(_k, B(lambda be: C.case_conv_fwd(be, 1, 32, 32, (22, 8, 16), residual=True), _t), exclude=_x), _c)
        row(f"{_form}_z{_s}_dgrad", _launches(_k, B(lambda be: C.case_conv_dgrad(be, 1, 32, 32, (6, 8, 16)), _t), exclude=_x), _c)
        row(f"{_form}_z{_s}_moments", _launches(_k, B(lambda be, t=_t: C.case_conv_moments(be, 1, 32, 32, (5, 8, 16), residual=True, chscale=True, ytol=t,
                                                                                       strict_vs_oracle=False), 2e-5), exclude=_x), _c)
        # (zring2 has no norm-backward epilogue: a 32 -> 32 dgrad with the sums takes the round-3 ring kernel in either form)
        row(f"{_form}_z{_s}_gnb", _launches(ZR, B(lambda be: C.case_gn_bwd_fused(be, 1, 32, 32, (5, 8, 16), compare_unfused=True), 2e-5), exclude=ZR2), _c)
row("zring_z2_fwd_ks2", _launches(ZR2, B(lambda be: C.case_conv_fwd(be, 1, 64, 32, (6, 8, 16), norm=True, residual=True, chscale=True), BF16_TOL["bf16"])),
    _zring("zring", "2"))
row("zring_z2_moments_two_tiles", _launches(ZR2, B(lambda be: C.case_conv_moments(be, 1, 64, 64, (9, 8, 16), residual=True, ytol=BF16_TOL["bf16"],
                                                                                  strict_vs_oracle=False), 2e-5)), _zring("zring", "2"))
row("zring_fp16_fwd", _launches(ZR2, B(lambda be: C.case_conv_fwd(be, 1, 32, 32, (5, 8, 16), norm=True, residual=True, chscale=True), BF16_TOL["fp16"])),
    _zring("zring", "", "fp16"))
# ---- 16-bit activation storage (act_storage_cases) ------------------------------------------------------------------------------------
_BF, _FP = dict(precision="bf16", **DIRECT), dict(precision="fp16", storage=torch.float16, **DIRECT)
row("act16_cast", _cast, DIRECT)
row("act16_pointwise", B(S.case_pointwise, S.TOL), DIRECT)                                       # upsample2x, add, chscale, layout
row("act16_norm", B(S.case_norm, S.TOL, dgamma=1e-5, dbeta=1e-5), DIRECT)
row("act16_proj", B(S.case_proj, S.TOL, dw=1e-5), DIRECT)
row("act16_k1_stream", _launches("conv3d_k1_stream_bf16", B(lambda be: S.case_conv_k1(be, cin=64, cout=64, residual=True), S.TOL)), DIRECT)
row("act16_s2", B(S.case_conv_s2, S.TOL, moments=2e-5), DIRECT)
row("act16_zero_insert", B(S.case_conv_zero_insert, S.TOL), DIRECT)
row("act16_zero_insert_window", B(lambda be: S.case_conv_zero_insert(be, window=True), S.TOL), DIRECT)
row("act16_k3_tile", B(lambda be: S.case_conv_k3_tile(be, 64, 32, (4, 8, 16), norm=True, residual=True, drop=True, moments=True, n=2), S.TOL, moments=2e-5), _BF)
row("act16_k3_tile_gnb", B(lambda be: _fused(S.case_conv_k3_tile(be, 32, 64, (4, 5, 17), gnb=True, mode=1)), S.TOL, gnb=1e-5), _BF)
row("act16_k3_zring", _launches(ZR2, B(lambda be: S.case_conv_k3_tile(be, 64, 32, (5, 8, 32), norm=True, residual=True, drop=True, moments=True, n=2), S.TOL, moments=2e-5)),
    dict(env={"MI355_BF16_FORM": "zring"}, **_BF))
row("act16_k3_zring1_gnb", _launches(ZR, B(lambda be: _fused(S.case_conv_k3_tile(be, 32, 32, (5, 8, 16), gnb=True, mode=1)), S.TOL, gnb=1e-5), exclude=ZR2),
    dict(env={"MI355_BF16_FORM": "zring1"}, **_BF))
row("act16_first_layer", B(S.case_first_layer, S.TOL, moments=2e-5, wgrad=1e-5, c4bwd_vs_wgrad=1e-5), _BF)
row("act16_wgrad_k1_lp_tr", B(lambda be: S.case_wgrad(be, 1, 1, 64, 32, (4, 5, 7)), S.TOL, dw=1e-5), _BF)
row("act16_wgrad_s2", B(lambda be: S.case_wgrad(be, 3, 2, 32, 32, (9, 8, 11), n=2), S.TOL, dw=1e-5), _BF)
row("act16_wgrad_k3", B(lambda be: S.case_wgrad(be, 3, 1, 32, 96, (3, 4, 17), norm=True), S.TOL, dw=1e-5), _BF)
row("act16_wgrad_lp_tr", B(lambda be: S.case_wgrad(be, 3, 1, 32, 32, (5, 9, 18), norm=True), S.TOL, dw=1e-5), _BF)
row("act16_wgrad_lp_tr_z_chunks", B(lambda be: S.case_wgrad(be, 3, 1, 64, 32, (17, 8, 16), n=2), S.TOL, dw=1e-5), _BF)
row("act16_fp16_k3_tile", B(lambda be: S.case_conv_k3_tile(be, 32, 32, (5, 6, 18), norm=True, moments=True), S.TOL, moments=2e-5), _FP)
row("act16_fp16_first_layer", B(S.case_first_layer, S.TOL, moments=2e-5, wgrad=1e-5, c4bwd_vs_wgrad=1e-5), _FP)
# ---- weight gradients -----------------------------------------------------------------------------------------------------------------
row("wgrad_ring", B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (6, 7, 8))), DIRECT)
row("wgrad_ring_z_chunks", B(lambda be: C.case_conv_wgrad(be, 1, 32, 64, (17, 5, 9), norm=True)), DIRECT)
row("wgrad_ring_many_columns", B(lambda be: C.case_conv_wgrad(be, 1, 64, 64, (2, 40, 104), norm=True)), DIRECT)
row("wgrad_ring_tall_planes", B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (3, 34, 9), norm=True)), DIRECT)
row("wgrad_generic_partial", B(lambda be: C.case_conv_wgrad(be, 1, 64, 96, (5, 5, 9), norm=True, slope=0.01)), DIRECT)
row("wgrad_c4", B(lambda be: C.case_conv_wgrad(be, 2, 4, 48, (8, 8, 16), norm=True, slope=0.01)), DIRECT)
row("wgrad_s2c32", B(lambda be: C.case_conv_wgrad(be, 1, 32, 32, (9, 8, 12), stride=2)), DIRECT)
row("wgrad_s2_generic", B(lambda be: C.case_conv_cat_slope(be, 1, 32, 32, 32, (5, 6, 7))), DIRECT)
row("wgrad_k1_stream", B(lambda be: C.case_conv_wgrad(be, 2, 64, 32, (5, 6, 7), kd=1)), DIRECT)
row("wgrad_k1_stream_2x4", B(lambda be: C.case_conv_wgrad(be, 2, 64, 128, (7, 9, 17), kd=1)), DIRECT)
row("wgrad_k1_generic", B(lambda be: C.case_conv_wgrad(be, 1, 64, 64, (4, 5, 7), kd=1)), DIRECT)
row("wgrad_wino", _calls("mi355_conv3d_wgrad_wino", B(lambda be: C.case_conv_wgrad(be, 1, 8, 64, (4, 9, 17)), 1e-4)), WGRAD_WINO)
row("wgrad_wino_columns", _calls("mi355_conv3d_wgrad_wino", B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (7, 16, 32), norm=True), 1e-4)), WGRAD_WINO)
row("wgrad_wino_partial", _calls("mi355_conv3d_wgrad_wino", B(lambda be: C.case_conv_wgrad(be, 1, 40, 96, (5, 3, 7), norm=True, slope=0.01), 1e-4)), WGRAD_WINO)
row("c4_bwd", B(lambda be: C.case_c4_bwd(be, 2, (5, 9, 19), groups=2, slope=0.01), 1e-4), DIRECT)
row("c4_bwd_two_z_chunks", B(lambda be: C.case_c4_bwd(be, 1, (17, 8, 16), groups=1), 1e-4), DIRECT)
row("c4_bwd_wide_views", B(lambda be: C.case_c4_bwd(be, 1, (2, 3, 5), xld=8, dyld=64), 1e-4), DIRECT)
# ---- norm, projection, pointwise ------------------------------------------------------------------------------------------------------
row("gn", B(lambda be: C.case_gn(be, 2, 32, (5, 6, 7), 8)), DIRECT)
row("gn_c4", B(lambda be: C.case_gn(be, 2, 4, (5, 6, 7), 4)), DIRECT)
row("gn_instance_wide", B(lambda be: C.case_gn(be, 1, 96, (4, 4, 4), 96, slope=0.01, ld=128)), DIRECT)
row("proj", B(lambda be: C.case_proj(be, 2, 32, 3, (5, 6, 7))), DIRECT)
row("proj_bias", B(lambda be: C.case_proj(be, 1, 64, 3, (9, 6, 7), bias=True)), DIRECT)
row("proj_prologue", B(lambda be: C.case_proj(be, 1, 32, 3, (5, 6, 7), bias=True, norm=True)), DIRECT)
row("upsample", B(lambda be: C.case_upsample(be, 2, 8, (4, 3, 5), (7, 5, 9))), DIRECT)
row("upsample_padded", B(lambda be: C.case_upsample(be, 2, 8, (2, 2, 2), (5, 4, 4))), DIRECT)
row("layout", lambda be: below(C.case_layout(be, 2, 4, (5, 6, 7)), 1e-30), DIRECT)
# ---- losses ---------------------------------------------------------------------------------------------------------------------------
row("dice", B(lambda be: C.case_dice(be, 2, 3, (12, 12, 12))), DIRECT)
row("dice_batch_squared_f32", B(lambda be: C.case_dice(be, 2, 3, (12, 12, 12), batch=True, squared=True, u8=False)), DIRECT)
for _m, _kw in (("softmax", {}), ("bce", {}), ("softmax_dice", dict(u8=False, with_dice=True)), ("bce_dice", dict(with_dice=True))):
    row(f"ce_{_m}", B(lambda be, kw=_kw, m=_m.split("_")[0]: C.case_ce(be, 1, 5, (6, 7, 9), mode=m, **kw)), DIRECT)
for _n in ("softmax", "softmax_onehot_nobg", "onehot_sigmoid", "jaccard", "jaccard_squared_batch", "weight", "weight_scalar_nobg", "sum", "none",
           "none_batch_nobg", "none_softmax_weight_jaccard", "no_activation"):
    row(f"dice_ex_{_n}", _dice_ex(_n), DIRECT, (QNAN, ONES) if "onehot" in _n else (QNAN,))     # forward's workspace is read by backward
row("loss_ce_labels", _loss("ce_labels"), DIRECT, (QNAN, ONES))                                  # class-index targets
row("loss_dicece_softmax_labels", _loss("dicece_softmax_labels"), DIRECT, (QNAN, ONES))
row("loss_gdl_empty_class", _loss("gdl_empty_class"), DIRECT)
# ---- either side of the network -------------------------------------------------------------------------------------------------------
row("prepost", _prepost, DIRECT, (QNAN, ONES))                                                  # zscore, postprocess, one_hot, resample_affine
row("ensemble_threshold", _ensemble, DIRECT, (QNAN, ONES))
row("components_6", _components((19, 13, 70), 1), DIRECT, (QNAN, ONES))
row("components_26", _components((19, 13, 70), 3), DIRECT, (QNAN, ONES))
row("components_single_row", _components((1, 9, 130), 1, c=1), DIRECT, (QNAN, ONES))
row("inferer", _inferer, DIRECT)                                                                # sw_gather / sw_accumulate_batch / sw_normalize
row("augment", _augment(False), DIRECT, (QNAN, ONES))
row("augment_normalize", _augment(True), DIRECT, (QNAN, ONES))

# ---- whole networks: every empty_act, concat half and gradient buffer dirty at once ----------------------------------------------------
NETWORK_ROWS = {
    "unet3d_reduced_odd_extent": (_unet(UNET_REDUCED, (14, 15, 13), 1), {}, (QNAN, ONES)),
    "dynunet_smallest": (_dynunet, {}, (QNAN, ONES)),
}
GPU_NETWORK_ROWS = {
    "unet3d_default_odd_extent": (_unet(UNET_DEFAULT, (30, 31, 29), 1), {}, (QNAN, ONES)),
    "unet3d_default_32cube_bf16_storage": (_unet(UNET_DEFAULT, (32, 32, 32), 2, "bf16", "bf16"), {}, (QNAN, ONES)),
}

# ---- GPU only: the smallest existing shape that reaches each route's multi-chunk / multi-workgroup path ---------------------------------
GPU_ROWS = {
    "gpu_fwd_s2c32_z_chunks": (B(lambda be: C.case_conv_fwd(be, 2, 32, 32, (65, 31, 36), stride=2, xld=64, yld=64, yc0=32)), DIRECT, (QNAN,)),
    "gpu_dgrad_s2c32_z_chunks": (B(lambda be: C.case_conv_dgrad(be, 2, 32, 32, (65, 31, 37), stride=2, residual=True)), DIRECT, (QNAN,)),
    "gpu_fwd_two_level_accumulation": (B(lambda be: C.case_conv_fwd(be, 1, 40, 96, (31, 33, 38))), DIRECT, (QNAN,)),
    "gpu_moments_two_level": (B(lambda be: C.case_conv_moments(be, 2, 128, 256, (16, 16, 16), residual=True), 2e-5), DIRECT, (QNAN,)),
    "gpu_moments_c4_ragged": (B(lambda be: C.case_conv_moments(be, 1, 4, 64, (33, 30, 36), groups_out=64), 2e-5), DIRECT, (QNAN,)),
    "gpu_moments_s2c32_ragged": (B(lambda be: C.case_conv_moments(be, 1, 32, 32, (65, 31, 36), stride=2, norm=False), 2e-5), DIRECT, (QNAN,)),
    "gpu_gnb_ragged": (B(lambda be: C.case_gn_bwd_fused(be, 1, 96, 64, (17, 19, 23), groups=96, slope=0.01), 2e-5), DIRECT, (QNAN,)),
    "gpu_wgrad_ring_z_chunks": (B(lambda be: C.case_conv_wgrad(be, 1, 32, 64, (17, 5, 9), norm=True)), DIRECT, (QNAN,)),
    "gpu_wgrad_ring_many_columns": (B(lambda be: C.case_conv_wgrad(be, 1, 32, 32, (8, 96, 190), norm=True)), DIRECT, (QNAN,)),
    "gpu_wgrad_k1_stream_chunks": (B(lambda be: C.case_conv_wgrad(be, 2, 64, 32, (33, 31, 29), kd=1)), DIRECT, (QNAN,)),
    "gpu_wgrad_s2c32": (B(lambda be: C.case_conv_wgrad(be, 1, 32, 32, (33, 32, 36), stride=2)), DIRECT, (QNAN,)),
    "gpu_wgrad_wino_32cube": (_calls("mi355_conv3d_wgrad_wino", B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (32, 32, 32), norm=True), 1e-4)), WGRAD_WINO, (QNAN,)),
    "gpu_wino2d_32cube": (_wino_was_routed(B(lambda be: C.case_conv_moments(be, 1, 32, 32, (32, 32, 32), yld=64, yc0=32), 2e-5)), WINO("2d"), (QNAN,)),
    "gpu_wino3d_32cube": (_wino_was_routed(B(lambda be: C.case_conv_moments(be, 1, 32, 32, (32, 32, 32), yld=64, yc0=32), 2e-5)), WINO("3d"), (QNAN,)),
    "gpu_c4_bwd_z_chunks": (B(lambda be: C.case_c4_bwd(be, 2, (33, 30, 36), groups=2, slope=0.01), 1e-4), DIRECT, (QNAN,)),
    "gpu_bf16_zring_16_z_tiles": (B(lambda be: C.case_conv_fwd(be, 2, 32, 32, (32, 32, 64), norm=True, residual=True), BF16_TOL["bf16"]),
                                  dict(precision="bf16", **DIRECT), (QNAN,)),
    "gpu_bf16_wgrad_splits": (B(lambda be: C.case_conv_wgrad(be, 2, 32, 32, (32, 32, 32), norm=True), BF16_TOL["bf16"]), dict(precision="bf16", **DIRECT), (QNAN,)),
    "gpu_gn_64cube": (B(lambda be: C.case_gn(be, 2, 32, (64, 64, 64), 8)), DIRECT, (QNAN,)),
    "gpu_dice_ce": (B(lambda be: C.case_ce(be, 2, 3, (48, 40, 56), mode="softmax", u8=False, with_dice=True)), DIRECT, (QNAN,)),
    "gpu_proj": (B(lambda be: C.case_proj(be, 2, 32, 3, (33, 30, 36), bias=True, norm=True)), DIRECT, (QNAN,)),
    "gpu_components": (_components((40, 48, 130), 3, c=3), DIRECT, (QNAN, ONES)),
}

_CONV = ("fwd_generic", "fwd_s2c32", "fwd_k1", "fwd_c4", "fwd_narrow", "dgrad_generic", "dgrad_s2c32", "dgrad_first_layer", "tconv_k3s2", "tconv_k2s2")
COVERAGE = {
    "mi355_pack_conv_weight": _CONV, "mi355_pack_conv_weight_bf16": ("bf16_fwd", "fp16_fwd", "bf16x3_fwd"),
    "mi355_conv3d_fwd": _CONV + ("bf16_fwd", "bf16x3_fwd", "fp16_fwd", "zring_z2_fwd", "zring_z5_fwd", "zring1_z2_fwd", "zring1_z5_fwd", "act16_k1_stream",
                                 "act16_k3_tile"),
    "mi355_conv3d_stats_blocks": ("moments_generic", "moments_c4", "moments_s2c32", "gnb_generic", "zring_z2_moments", "zring_z5_moments", "zring1_z5_gnb",
                                  "bf16_moments", "act16_k3_zring"),
    "mi355_conv3d_wgrad_workspace": ("wgrad_ring", "wgrad_ring_z_chunks", "wgrad_ring_many_columns", "wgrad_c4", "wgrad_s2c32", "wgrad_k1_stream",
                                     "wgrad_k1_generic", "tconv_k2s2", "bf16_wgrad_splits", "act16_wgrad_lp_tr", "act16_wgrad_k1_lp_tr"),
    "mi355_conv3d_wgrad": ("wgrad_ring", "wgrad_generic_partial", "wgrad_s2_generic"),
    "mi355_gn_workspace": ("gn", "gn_c4", "gn_instance_wide", "c4_bwd"), "mi355_gn_stats": ("gn", "act16_norm"),
    "mi355_gn_moments_blocks": ("cat_moments",), "mi355_gn_moments": ("cat_moments",), "mi355_gn_records_reduce": ("records_reduce",),
    "mi355_gn_finalize": ("moments_generic", "cat_moments"), "mi355_gn_act_bwd": ("gn", "act16_norm"),
    "mi355_gn_act_bwd_fused": ("gnb_generic", "wino2d_gnb", "wino3d_gnb"), "mi355_gn_bwd_params": ("c4_bwd",),
    "mi355_upsample2x_fwd": ("upsample", "act16_pointwise"), "mi355_upsample2x_bwd": ("upsample", "act16_pointwise"),
    "mi355_ncdhw_to_ndhwc": ("layout", "act16_pointwise"), "mi355_ndhwc_to_ncdhw": ("layout", "act16_pointwise"),
    "mi355_add": ("act16_pointwise",), "mi355_chscale": ("act16_pointwise",), "mi355_cast": ("act16_cast",),
    "mi355_proj_fwd": ("proj", "proj_bias", "proj_prologue"), "mi355_proj_workspace": ("proj", "proj_bias", "proj_prologue"), "mi355_proj_bwd": ("proj", "act16_proj"),
    "mi355_sw_gather": ("inferer",), "mi355_sw_accumulate_batch": ("inferer",), "mi355_sw_normalize": ("inferer",),
    "mi355_postprocess": ("prepost",), "mi355_one_hot": ("prepost",), "mi355_zscore_workspace": ("prepost",), "mi355_zscore": ("prepost",),
    "mi355_resample_affine": ("prepost",), "mi355_augment_batch_workspace": ("augment_normalize",), "mi355_augment_batch": ("augment", "augment_normalize"),
    "mi355_conv3d_c4_bwd_blocks": ("c4_bwd", "c4_bwd_two_z_chunks", "c4_bwd_wide_views"), "mi355_conv3d_c4_bwd_workspace": ("c4_bwd", "c4_bwd_two_z_chunks"),
    "mi355_conv3d_c4_bwd": ("c4_bwd", "act16_first_layer"),
    "mi355_wino_pack_weight": ("wino2d_fwd",), "mi355_conv3d_wino_fwd": ("wino2d_fwd", "wino2d_fwd_slice", "wino2d_dgrad"),
    "mi355_conv3d_wino_stats_blocks": ("wino2d_moments", "wino3d_moments", "wino2d_gnb", "wino3d_gnb"),
    "mi355_wino3d_pack_weight": ("wino3d_fwd",), "mi355_conv3d_wino3d_fwd": ("wino3d_fwd", "wino3d_fwd_slice", "wino3d_dgrad"),
    "mi355_conv3d_wgrad_wino_workspace": ("wgrad_wino", "wgrad_wino_columns", "wgrad_wino_partial"), "mi355_conv3d_wgrad_wino": ("wgrad_wino",),
    "mi355_dice_workspace": ("dice", "dice_ex_none", "dice_ex_softmax"), "mi355_dice_fwd_bwd": ("dice", "dice_batch_squared_f32"),
    "mi355_dice_ex_forward": ("dice_ex_softmax", "dice_ex_none"), "mi355_dice_ex_backward": ("dice_ex_softmax", "dice_ex_none"),
    "mi355_ce_workspace": ("ce_softmax", "ce_bce"), "mi355_ce_fwd_bwd": ("ce_softmax", "ce_bce", "ce_softmax_dice", "ce_bce_dice", "loss_ce_labels"),
    "mi355_ensemble_threshold": ("ensemble_threshold",), "mi355_cc_workspace": ("components_6", "components_26"),
    "mi355_cc_label": ("components_6", "components_26", "components_single_row"), "mi355_cc_filter": ("components_6", "components_26"),
}
