"""TEST INFRASTRUCTURE: the 16-bit-storage forms of the convolutions that only HipDynUNet / HipDynUNetDS send to the library (HipUNet3D's
are tests/act_storage_cases.py): a stride-2 3x3x3 convolution that normalises its input, the ConvTranspose3d(k2, s2) as a 1x1x1 GEMM
(depth-to-space output, norm prologue), its data gradient (space-to-depth input), and the weight gradients of the two.

The property is that of act_storage_cases: on 16-bit tensors a kernel computes in fp32 what it computes on fp32 tensors holding the same
values and rounds once on store (`stored_ok`, remainder 1e-6); a weight gradient (an fp32 result either way) agrees to 1e-5, the bound
tests/test_act_storage_emu.py holds `dw` to. The fp32 forms of the same kernels are held to their oracles by the existing suite."""
import importlib

import torch

import act_storage_cases as S
import op_cases as C

ops = importlib.import_module("3dunetcnn_amd.ops")
TOL = {"dw": 1e-5, "moments": 2e-5}          # everything else: S.TOL
SLOPE = 0.01


def _prologue(be, x32, cin, g):
    """Per-(n, c) scale and shift of an InstanceNorm over x (the statistics of the fp32 tensor in both runs) + LeakyReLU."""
    st = be.gn_stats(x32, cin, 1e-5, C.dev(be, torch.rand(cin, generator=g) + 0.5), C.dev(be, torch.randn(cin, generator=g) * 0.3))
    return dict(in_mode=ops.IN_AFFINE_ACT, scale=st[1], shift=st[2], slope=SLOPE)


def case_s2_norm(be, cin=12, cout=40, dhw=(6, 10, 14), moments=True):
    """Down block conv1: ragged tiles (3 x 5 x 7 outputs against 4 x 4 x 8), cin no multiple of the 8-channel chunk, cout across the 32-channel
    wave tile, ld > c on both sides."""
    g = torch.Generator().manual_seed(21)
    t = S.bf16_values((2, cin, *dhw), g, 1.3, 0.2)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05
    kw = _prologue(be, S.acts(be, t)[0], cin, g)
    odhw = tuple(s // 2 for s in dhw)
    return S._conv_both(be, t, w, 0, 3, (2, cout, *odhw), dict(stride=2, moments=moments, **kw), x_ld=cin + 4, x_c0=4, y_ld=2 * cout, y_c0=cout)


def case_transposed(be, cin=24, co=12, dhw=(3, 5, 7), norm=True):
    """ConvTranspose3d(k2, s2) forward: [8 co, cin] GEMM over the coarse voxels, written to the fine tensor's first co channels of 2 co (the
    concat buffer)."""
    g = torch.Generator().manual_seed(22)
    t = S.bf16_values((2, cin, *dhw), g, 1.3, 0.2)
    w = torch.randn(8 * co, cin, 1, 1, 1, generator=g) * 0.1
    kw = _prologue(be, S.acts(be, t)[0], cin, g) if norm else {}
    fine = tuple(2 * s for s in dhw)
    return S._conv_both(be, t, w, 0, 1, (2, co, *fine), dict(out_mode=ops.OUT_D2S, **kw), y_ld=2 * co)


def case_transposed_dgrad(be, cin=24, co=12, dhw=(3, 5, 7)):
    """Its data gradient: the fine gradient (a slice of the concat buffer's gradient) read space-to-depth."""
    g = torch.Generator().manual_seed(23)
    fine = tuple(2 * s for s in dhw)
    t = S.bf16_values((2, co, *fine), g)
    w = torch.randn(8 * co, cin, 1, 1, 1, generator=g) * 0.1
    return S._conv_both(be, t, w, 1, 1, (2, cin, *dhw), dict(in_mode=ops.IN_S2D), x_ld=2 * co)


def case_wgrad(be, kind, cin=12, cout=24, dhw=(6, 10, 14)):
    """kind "s2": the weight gradient of case_s2_norm's conv; "d2s": of the transposed conv ([8 co, cin], fine gradient). Both with the
    norm prologue on x."""
    g = torch.Generator().manual_seed(24)
    if kind == "d2s":
        dhw = tuple(s // 2 for s in dhw)
    t = S.bf16_values((2, cin, *dhw), g, 1.3, 0.2)
    x32, x16 = S.acts(be, t, ld=cin + 4, c0=4)
    kw = _prologue(be, x32, cin, g)
    if kind == "s2":
        dy32, dy16 = S.acts(be, S.bf16_values((2, cout, *(s // 2 for s in dhw)), g))
        shape, call = (cout, cin, 3, 3, 3), dict(kd=3, stride=2)
    else:
        dy32, dy16 = S.acts(be, S.bf16_values((2, cout, *(2 * s for s in dhw)), g), ld=2 * cout)
        shape, call = (8 * cout, cin), dict(kd=1, out_mode=ops.OUT_D2S)
    dws = []
    for x, dy in ((x32, dy32), (x16, dy16)):
        dw = C.out_host(shape, 3.0).to(be.device)
        be.conv_wgrad(x, dy, dw, **call, **kw)
        dws.append(dw.cpu())
    assert bool(torch.isfinite(dws[0]).all()) and float(dws[0].abs().max()) > 0
    return {"dw": C.rel_err(dws[1], dws[0])}


CASES = {
    "s2-norm-moments": lambda be: case_s2_norm(be),
    "s2-norm-wide": lambda be: case_s2_norm(be, cin=32, cout=64, dhw=(8, 8, 16), moments=False),      # whole tiles, the 64-channel workgroup
    "transposed-norm": lambda be: case_transposed(be),
    "transposed-plain-wide": lambda be: case_transposed(be, cin=64, co=8, dhw=(4, 4, 20), norm=False),      # more than one 256-voxel tile
    "transposed-dgrad": lambda be: case_transposed_dgrad(be),
    "transposed-dgrad-wide": lambda be: case_transposed_dgrad(be, cin=64, co=8, dhw=(4, 4, 20)),
    "wgrad-s2-norm": lambda be: case_wgrad(be, "s2"),
    "wgrad-d2s-norm": lambda be: case_wgrad(be, "d2s"),
}


def run(be, cid, precision, storage):
    saved = be.precision
    be.set_precision(precision)
    try:
        with S.storage_type(storage):
            errs = CASES[cid](be)
    finally:
        be.precision = saved
    print("record", cid, precision, errs)
    bad = {k: v for k, v in errs.items() if not isinstance(v, bool) and v > TOL.get(k, S.TOL)}
    assert not bad, (bad, errs)
