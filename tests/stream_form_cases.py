"""TEST INFRASTRUCTURE: every kernel form of the streaming ops (csrc/pointwise.hip, csrc/norm.hip, the storage conversions of
csrc/act_io.h, adam_kernel of csrc/loss_optim.hip) against a float64 evaluation of the operation on the values the kernel read. Shared by
the emulator twin (tests/test_stream_forms_emu.py: which kernel a view launches, and the values) and the GPU twin
(tests/test_stream_forms_gpu.py: the same views, the values).

THE FORM TABLE. `ROWS` holds one row per (entry point, kernel expression, storage type) an entry point can launch in a default environment,
with the smallest view that reaches it. The kernel choice is host code shared by both builds and depends on the view only (storage type;
act_vw8(): c % 8, ld % 8, 16-byte alignment of the base pointer; 256 % (C / VW)), so the emulator twin pins the choice -- `launches` is
exactly what tools/emu records for the call -- and the GPU twin runs the same view. The forms behind MI355_UPSAMPLE_ROWS=0 /
MI355_GN_APPLY_ROWS=0 are the grid-stride kernels the table reaches through channel counts. No form turned out unreachable by a valid view.
(Of the forms here, gn_bwd_apply_kernel<T, 8> was already launched by tests/act_storage_cases.py::case_norm(c=24), which compares a 16-bit
run with an fp32 run and fails when that kernel's store is displaced; upsample2x_fwd_kernel had no test: swapped taps in it passed the suite.)

CRITERIA (float64, element by element; 16-bit inputs are widened exactly; nothing is compared with another run of the library).

Linear ops: |got - ref| <= (k + 1) * 2^-24 * cond + storage. cond = the same operation in float64 on the absolute values of the inputs
(weights: their absolute values); storage = half an ulp of the output's storage type at ref (ulp arithmetic of launch_audit.store_err), 0
for fp32; k = the rounded fp32 operations on the longest path from an input to the output -- the standard forward bound of a sum of
products, no free tolerance:
  up-sampling forward  k = 9   pointwise.hip `o[e] += w * v[e]` (upsample2x_fwd_kernel) / `o[e] += w[k] * v[k][e]` (rows form): the
                               weights are products of 0, 1/4, 3/4, 1 and exact (27/64 has 5 significant bits), so a term is one rounded
                               product and goes through at most eight rounded additions
  up-sampling backward k = 65  pointwise.hip `o[e] += w * v[c][e]` (upsample2x_bwd_kernel): exact weights again (a clamped tap adds
                               1/4 + 3/4), one rounded product and at most 4 x 4 x 4 = 64 rounded additions
  add                  k = 1   pointwise.hip add_kernel `av.x + bv.x`
  chscale              k = 1   pointwise.hip chscale_kernel `xv[e] *= sv[e]`
An output voxel outside the up-sampling window must be +0, bit for bit.

cast and the two layout ops: bitwise torch's .to(dtype), NaN for NaN at any payload.

Norm and projection (not linear in their inputs): launch_audit.store_err against the float64 oracle under the bounds
tests/test_launch_audit.py::BOUNDS records on MI355X: gn_stats 1e-5, gn_act_bwd 1e-5, proj_fwd / proj_bwd 1e-5. The norm inputs carry a
mean (0.4) next to their spread (1.7) so that no group of a case is four nearly equal values; no case needed another seed or scale to
meet its bound on the emulator. The tensors a norm case reads are followed, in the same allocation, by one more sample of NaN: a read
past the last voxel is then a NaN in the result and not whatever the allocator left there.

Adam (adam_case): one step from a given state against oracle.torch_ops.adam_step in float64 on the same fp32 inputs,
  |m - m_ref| <= (6 + 1) * 2^-24 * (|b1 m| + (1 - b1)(|g gs| + |wd p|))       loss_optim.hip adam_kernel: g * gscale, wd * p, +, the fp32
                                                                                 (1 - b1), omb1 * gg, the final + : 6 on the longest path
  |v - v_ref| <= (10 + 1) * 2^-24 * (b2 v + (1 - b2)(|g gs| + |wd p|)^2)      gg twice (3 + 3), the fp32 (1 - b2), two products, +
  |p - p_ref| <= 1/2 ulp32(p_ref) + (19 + 1) * 2^-24 * |update_ref|           m (6), sqrt(v) (10 / 2), sqrtf, the fp32 sqrt(bc2), /, the fp32
                                                                                 eps, +, m / denom, the fp32 lr / bc1, * : 19; the final
                                                                                 subtraction is the half ulp
The bound on p holds where m and gg do not cancel (a cancelled sum has no relative error bound): the state is drawn with the sign of
exp_avg and of the parameter equal to the gradient's, which is what makes |m_ref| the sum of the absolute values of its two terms.

EXHAUSTIVE CONVERSIONS (conversion_inputs): through mi355_cast on c = 4 views, every 16-bit pattern widened, every rounding boundary of
both narrowings (each pattern, the midpoint to its upper neighbour, the two fp32 values beside the midpoint, fp16's overflow threshold,
fp32 subnormals, zeros, infinities, NaNs), and the two 16-bit types into each other over all patterns. tests/test_volume_bits.py and
tests/test_conv_bits.py pin outputs of whole kernels on a few hundred values and exercise no conversion exhaustively, so no direction is
skipped. pack_bf16x2 / pack_f16x2 are instructions on gfx950 and C++ twins in tools/emu: this is what says the two agree.
"""
import ctypes
import importlib
import os
import re

import torch
import torch.nn.functional as F

import launch_audit as A
from oracle import torch_ops as O

ops = importlib.import_module("3dunetcnn_amd.ops")
_lib = importlib.import_module("3dunetcnn_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
LP = (BF16, F16)
ALL = (F32, BF16, F16)
U = 2.0 ** -24
BOUND = 1e-5                 # gn_stats, gn_act_bwd, proj_fwd, proj_bwd: tests/test_launch_audit.py::BOUNDS
K_UP_FWD, K_UP_BWD, K_ADD, K_CHSCALE = 9, 65, 1, 1
K_ADAM_M, K_ADAM_V, K_ADAM_P = 6, 10, 19
POISON = 7.0                 # the channels of a wider buffer outside a view: never written


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def take(be):
    """Kernel expressions LAUNCHed since the previous call (emulator), one per launch; None on a real device."""
    if be.device.type != "cpu":
        return None
    fn = be.lib.emu_take_launches
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(65536)
    fn(buf, 65536)
    return [line for line in buf.value.decode().split("\n") if line]


def launched(be, want):
    got = take(be)
    assert got is None or got == list(want), (got, want)


def values(shape, g, dtype, scale=1.0, shift=0.0):
    """fp32 tensor of values `dtype` holds exactly."""
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).float()


def act(be, t, dtype, ld=None, c0=0, guard=False):
    """NCDHW fp32 tensor of `dtype`-representable values -> Act of `dtype` with leading dimension ld at channel c0, POISON in the other
    channels. guard: one more sample of NaN follows the view in the same allocation."""
    n, c, d, h, w = t.shape
    ld = ld or c
    buf = torch.full((n + (1 if guard else 0), d, h, w, ld), POISON, dtype=dtype)
    if guard:
        buf[n:] = float("nan")
    buf[:n, ..., c0:c0 + c] = t.permute(0, 2, 3, 4, 1).to(dtype)
    return ops.Act(buf.to(be.device).contiguous()[:n], c0, c)


def out_act(be, shape5, dtype, ld=None, c0=0):
    """An output view the kernel must overwrite completely: NaN inside, POISON outside."""
    return act(be, torch.full(shape5, float("nan")), dtype, ld, c0)


def widen(a):
    """The view's values, NCDHW float64 on the host."""
    return a.tensor().detach().cpu().double().permute(0, 4, 1, 2, 3).contiguous()


def outside_untouched(a):
    other = torch.ones(a.ld, dtype=torch.bool)
    other[a.c0:a.c0 + a.c] = False
    assert bool((a.buf.cpu()[..., other].float() == POISON).all()), "wrote outside its channel slice"


def dev(be, t):
    return None if t is None else t.detach().clone().to(be.device).contiguous()


def half_ulp(ref, dtype):
    """Half the spacing of `dtype` at |ref| (the arithmetic of launch_audit.store_err); 0 for fp32."""
    if dtype == BF16:
        return 0.5 * torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126))) - 7.0)
    if dtype == F16:
        return 0.5 * torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -14))) - 10.0)
    return torch.zeros_like(ref)


def linear_ok(got, ref, cond, k, dtype, what):
    got, ref, cond = got.double(), ref.double(), cond.double()
    allow = (k + 1) * U * cond + half_ulp(ref, dtype)
    err = (got - ref).abs()
    bad = ~(err <= allow)                                   # a NaN fails
    print(f"{what}: worst error / allowance {float((err / allow.clamp(min=1e-300)).max()):.3f}")
    assert not bool(bad.any()), (what, int(bad.sum()), float(err[bad].max()), float(allow[bad].min()))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(got, want, what):
    """Bitwise equal, NaN for NaN at any payload."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (what, "NaNs differ")
    ok = (bits(got) == bits(want)) | nan
    assert bool(ok.all()), (what, int((~ok).sum()), got[~ok][:4], want[~ok][:4])


def bounded(err, what, bound=BOUND):
    print(f"{what}: {err:.3e} (bound {bound:g})")
    assert err <= bound, (what, err, bound)          # a NaN fails


# ---- up-sampling -----------------------------------------------------------------------------------------------------------------------
# lo -> cat extents. Over the rows each axis sees a low-resolution size of 1, a crop (cat = 2 lo - 1, off = -1), padding at the end only
# (cat = 2 lo + 1, off = 0) and padding on both sides (cat = 2 lo + 2, off = 1): test_geometry_is_covered counts them.
GEOMETRY = {
    "g1": ((1, 2, 3), (3, 3, 7)),       # z: size 1, end     y: crop           x: end
    "g2": ((3, 1, 2), (5, 4, 5)),       # z: crop            y: size 1, both   x: end
    "g3": ((2, 3, 1), (6, 5, 4)),       # z: both            y: crop           x: size 1, both
    "g4": ((2, 2, 2), (5, 5, 3)),       # z: end             y: end            x: crop
    "xloop": ((1, 1, 3), (2, 2, 7)),    # Wc = 7 > XPB = 4 at C = 256: the x loop of the rows form runs twice
}


def offsets(lo, cat):
    return tuple((t - 2 * l) // 2 for t, l in zip(cat, lo))


def upsample_fwd_case(be, dtype, c, geom, launches, lo_view=(None, 0), cat_view=(None, 0), seed=0):
    lo_dhw, cat_dhw = GEOMETRY[geom]
    g = torch.Generator().manual_seed(seed)
    lo = act(be, values((2, c, *lo_dhw), g, dtype), dtype, *lo_view)
    cat = out_act(be, (2, c, *cat_dhw), dtype, *cat_view)
    off = offsets(lo_dhw, cat_dhw)
    take(be)
    be.upsample2x_fwd(lo, cat, off)
    launched(be, launches)
    x = widen(lo)
    linear_ok(widen(cat), O.upsample_pad(x, cat_dhw), O.upsample_pad(x.abs(), cat_dhw), K_UP_FWD, dtype, f"upsample fwd {dtype} C={c} {geom}")
    inside = torch.ones(cat_dhw, dtype=torch.bool)
    for ax in range(3):
        u = torch.arange(cat_dhw[ax]) - off[ax]
        shape = [1, 1, 1]
        shape[ax] = -1
        inside &= ((u >= 0) & (u < 2 * lo_dhw[ax])).view(shape)
    raw = bits(cat.tensor()).permute(0, 4, 1, 2, 3)[:, :, ~inside]
    assert bool((raw == 0).all()), "a voxel outside the up-sampling window is not +0"
    outside_untouched(cat)


def upsample_bwd_case(be, dtype, c, geom, launches, dcat_view=(None, 0), dlo_view=(None, 0), seed=1):
    lo_dhw, cat_dhw = GEOMETRY[geom]
    g = torch.Generator().manual_seed(seed)
    dcat = act(be, values((2, c, *cat_dhw), g, dtype), dtype, *dcat_view)
    dlo = out_act(be, (2, c, *lo_dhw), dtype, *dlo_view)
    take(be)
    be.upsample2x_bwd(dcat, dlo, offsets(lo_dhw, cat_dhw))
    launched(be, launches)
    with torch.enable_grad():
        lo = torch.zeros(2, c, *lo_dhw, dtype=torch.float64, requires_grad=True)
        up = O.upsample_pad(lo, cat_dhw)
        d = widen(dcat)
        (ref,) = torch.autograd.grad(up, lo, d, retain_graph=True)
        (cond,) = torch.autograd.grad(up, lo, d.abs())
    linear_ok(widen(dlo), ref, cond, K_UP_BWD, dtype, f"upsample bwd {dtype} C={c} {geom}")
    outside_untouched(dlo)


# ---- add / chscale / cast / layout -------------------------------------------------------------------------------------------------------
SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 65504.0, 65520.0, 65519.996, 1e-40, -1e-40, 3.0e38, 5.9e-8, 2.0 ** -25)


def add_case(be, dtype, launches, alias=False, seed=2):
    g = torch.Generator().manual_seed(seed)
    shape = (2, 12, 3, 3, 5)
    a = act(be, values(shape, g, dtype), dtype, 12, 0)
    b = act(be, values(shape, g, dtype), dtype, 16, 4)
    y = a if alias else out_act(be, shape, dtype, 20, 8)
    av, bv = widen(a), widen(b)
    take(be)
    be.add(a, b, y)
    launched(be, launches)
    linear_ok(widen(y), av + bv, av.abs() + bv.abs(), K_ADD, dtype, f"add {dtype} alias={alias}")
    outside_untouched(y)
    outside_untouched(b)


def chscale_case(be, dtype, c, launches, view=(None, 0), alias=False, seed=3):
    g = torch.Generator().manual_seed(seed)
    shape = (2, c, 3, 3, 5)
    x = act(be, values(shape, g, dtype), dtype, *view)
    y = x if alias else out_act(be, shape, dtype, *view)
    s = torch.rand(2, c, generator=g) * 2.0 - 0.5
    xv = widen(x)
    take(be)
    be.chscale(x, dev(be, s), y)
    launched(be, launches)
    sv = s.double()[:, :, None, None, None]
    linear_ok(widen(y), xv * sv, xv.abs() * sv.abs(), K_CHSCALE, dtype, f"chscale {dtype} C={c} alias={alias}")
    outside_untouched(y)


def cast_case(be, src, dst, launches, seed=4):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(2, 8, 3, 5, 7, generator=g) * torch.exp2(torch.randint(-30, 30, (2, 8, 3, 5, 7), generator=g).float())
    t.view(-1)[:len(SPECIALS)] = torch.tensor(SPECIALS)
    x = act(be, t.to(src).float(), src, 12, 4)
    y = out_act(be, (2, 8, 3, 5, 7), dst, 16, 8)
    take(be)
    be.cast(x, out=y)
    launched(be, launches)
    same_bits(y.tensor(), x.tensor().cpu().to(dst), f"cast {src} -> {dst}")
    outside_untouched(y)


def layout_case(be, dtype, c, launches, seed=5):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(2, c, 3, 4, 5, generator=g) * 3.0
    src.view(-1)[:len(SPECIALS)] = torch.tensor(SPECIALS)
    dst = out_act(be, (2, c, 3, 4, 5), dtype, 8, 4 if c <= 4 else 0)
    take(be)
    be.ncdhw_to_ndhwc(dev(be, src), dst)
    launched(be, launches[:1])
    same_bits(dst.tensor().cpu().permute(0, 4, 1, 2, 3), src.to(dtype), f"ncdhw -> ndhwc {dtype} C={c}")
    outside_untouched(dst)
    back = torch.full(src.shape, float("nan")).to(be.device)
    be.ndhwc_to_ncdhw(dst, back)
    launched(be, launches[1:])
    same_bits(back, src.to(dtype).float(), f"ndhwc -> ncdhw {dtype} C={c}")


# ---- norm --------------------------------------------------------------------------------------------------------------------------------
def stats_oracle(x, groups, gamma, beta, eps=1e-5):
    """(mean, rstd [n, G], scale, shift [n, C]) of GroupNorm(groups) over the NCDHW float64 tensor x."""
    n, c = x.shape[:2]
    xg = x.reshape(n, groups, -1)
    mean, rstd = xg.mean(-1), (xg.var(-1, unbiased=False) + eps).rsqrt()
    cpg = c // groups
    scale = (gamma.double()[None] if gamma is not None else 1.0) * rstd.repeat_interleave(cpg, 1)
    shift = (beta.double()[None] if beta is not None else 0.0) - mean.repeat_interleave(cpg, 1) * scale
    return mean, rstd, scale, shift


def norm_input(be, dtype, c, dhw, view, seed):
    g = torch.Generator().manual_seed(seed)
    x = act(be, values((2, c, *dhw), g, dtype, 1.7, 0.4), dtype, *view, guard=True)
    return g, x, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3


def moments_case(be, dtype, c, dhw, launches, view=(None, 0), seed=6):
    """mi355_gn_moments: the (count, sum, M2) records of every block, merged in float64 (Chan's formula), against the channel's float64
    count, mean and centred sum of squares; an empty trailing block leaves (0, 0, 0)."""
    _, x, _, _ = norm_input(be, dtype, c, dhw, view, seed)
    take(be)
    (rec, nb, _), = be.moments(x)
    x.mom = None
    launched(be, launches)
    V = dhw[0] * dhw[1] * dhw[2]
    per = (V + nb - 1) // nb
    counts = torch.tensor([max(0, min(V, (b + 1) * per) - b * per) for b in range(nb)], dtype=torch.float64)
    r = rec.detach().cpu().double()                                  # [n, B, c, 3]
    assert torch.equal(r[..., 0], counts[None, :, None].expand(2, nb, c)), "record counts"
    empty = counts == 0
    if dhw == (1, 17, 17):
        assert nb == 18 and per == 17 and int(empty.sum()) == 1, (nb, per)
    assert bool((r[:, empty] == 0).all()), ("an empty block's record is not (0, 0, 0)", r[:, empty])
    xv = widen(x).reshape(2, c, V)
    mean = r[..., 1].sum(1) / V
    bm = r[..., 1] / counts.clamp(min=1)[None, :, None]
    m2 = (r[..., 2] + counts[None, :, None] * (bm - mean[:, None]) ** 2 * (~empty)[None, :, None]).sum(1)
    ref_mean = xv.mean(-1)
    bounded(A.store_err(mean, ref_mean, F32), f"moments mean {dtype} C={c} {dhw}")
    bounded(A.store_err(m2, ((xv - ref_mean[..., None]) ** 2).sum(-1), F32), f"moments M2 {dtype} C={c} {dhw}")


def stats_case(be, dtype, c, dhw, groups, launches, view=(None, 0), seed=6, fold=0):
    """mi355_gn_stats; fold > 0: the records of mi355_gn_moments folded to `fold` blocks (mi355_gn_records_reduce, k = 3) and finalised
    by mi355_gn_finalize."""
    _, x, gamma, beta = norm_input(be, dtype, c, dhw, view, seed)
    take(be)
    if fold:
        (rec, nb, _), = be.moments(x)
        out = torch.full((2, fold, c, 3), float("nan")).to(be.device)
        _lib.check(be.lib.mi355_gn_records_reduce(rec.data_ptr(), 2, nb, c, 3, out.data_ptr(), fold, be.stream()), "gn_records_reduce")
        x.mom = [(out, fold, c)]
    mr, sc, sh = be.gn_stats(x, groups, 1e-5, dev(be, gamma), dev(be, beta))
    launched(be, launches)
    mean, rstd, scale, shift = stats_oracle(widen(x), groups, gamma, beta)
    what = f"gn_stats {dtype} C={c} G={groups} {dhw} fold={fold}"
    bounded(max(A.store_err(mr[..., 0], mean, F32), A.store_err(mr[..., 1], rstd, F32), A.store_err(sc, scale, F32),
                A.store_err(sh, shift, F32)), what)


def gn_bwd_oracle(xv, dAv, addv, groups, slope, gamma, scale32, shift32):
    """dx, dgamma, dbeta of act(GroupNorm(x)) in float64; the activation mask is taken from the scale / shift the kernel reads."""
    u = xv * scale32.double()[:, :, None, None, None] + shift32.double()[:, :, None, None, None]
    mask = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, float(torch.tensor(slope, dtype=F32))))
    with torch.enable_grad():
        xin = xv.clone().requires_grad_(True)
        ga = gamma.double().clone().requires_grad_(True)
        be_ = torch.zeros_like(ga).requires_grad_(True)
        dx, dg, db = torch.autograd.grad(F.group_norm(xin, groups, ga, be_, 1e-5), (xin, ga, be_), dAv * mask)
    return (dx + addv if addv is not None else dx), dg, db


def gn_bwd_case(be, dtype, c, dhw, groups, slope, launches, addend=None, params="gb", view=(None, 0), dx_view=(None, 0), route="plain", seed=7):
    """mi355_gn_act_bwd. addend: None or its (ld, c0) view. params: which of dgamma ("g") / dbeta ("b") are asked for.
    route "fused": mi355_gn_act_bwd_fused and mi355_gn_bwd_params, fed the records mi355_gn_act_bwd's own first pass left in the workspace,
    folded to another block count by mi355_gn_records_reduce (k = 2); `launches` is then those of the four calls in turn."""
    g, x, gamma, _ = norm_input(be, dtype, c, dhw, view, seed)
    shape = (2, c, *dhw)
    dA = act(be, values(shape, g, dtype), dtype, *view, guard=True)
    add = act(be, values(shape, g, dtype), dtype, *addend, guard=True) if addend is not None else None
    xv, dAv, addv = widen(x), widen(dA), widen(add) if add is not None else None
    mean, rstd, scale, shift = stats_oracle(xv, groups, gamma, None)
    mr = dev(be, torch.stack((mean, rstd), -1).float())                    # what the kernel reads: the float64 statistics, rounded once
    sc, sh, gam = dev(be, scale.float()), dev(be, shift.float()), dev(be, gamma)
    dx_ref, dg_ref, db_ref = gn_bwd_oracle(xv, dAv, addv, groups, slope, gamma, sc.cpu(), sh.cpu())

    def outputs():
        return (out_act(be, shape, dtype, *dx_view), torch.full((c,), float("nan")).to(be.device) if "g" in params else None,
                torch.full((c,), float("nan")).to(be.device) if "b" in params else None)

    def judge(dx, dg, db, what):
        if dx is not None:
            bounded(A.store_err(widen(dx), dx_ref, dtype), what + " dx")
            outside_untouched(dx)
        if dg is not None:
            bounded(A.store_err(dg, dg_ref, F32), what + " dgamma")
        if db is not None:
            bounded(A.store_err(db, db_ref, F32), what + " dbeta")

    what = f"gn_act_bwd {dtype} C={c} G={groups} {dhw} slope={slope} addend={addend} params={params!r}"
    dx, dg, db = outputs()
    take(be)
    be.gn_act_bwd(x, dA, dx, groups, slope, gam, mr, sc, sh, dg, db, addend=add)
    if route == "plain":
        launched(be, launches)
        return judge(dx, dg, db, what)
    launched(be, launches[0])
    judge(dx, dg, db, what)
    xd = x.desc()
    nb = be.lib.mi355_gn_moments_blocks(ctypes.byref(xd))
    nb2 = nb - 2
    assert nb2 >= 2
    ws = be.ws(be.lib.mi355_gn_workspace(ctypes.byref(xd)))
    first_pass = ws[:2 * nb * c * 2].clone()                               # [n][B][C][2], at the head of the workspace (norm.hip)
    rec = torch.full((2, nb2, c, 2), float("nan")).to(be.device)
    _lib.check(be.lib.mi355_gn_records_reduce(first_pass.data_ptr(), 2, nb, c, 2, rec.data_ptr(), nb2, be.stream()), "gn_records_reduce")
    launched(be, launches[1])
    dx, dg, db = outputs()
    be.gn_act_bwd(x, dA, dx, groups, slope, gam, mr, sc, sh, dg, db, addend=add, partials=(rec, nb2))
    launched(be, launches[2])
    judge(dx, dg, db, what + " fused")
    _, dg, db = outputs()
    _lib.check(be.lib.mi355_gn_bwd_params(ctypes.byref(xd), groups, gam.data_ptr(), mr.data_ptr(), ops._p(dg), ops._p(db), rec.data_ptr(), nb2,
                                          ws.data_ptr(), ws.numel() * 4, be.stream()), "gn_bwd_params")
    launched(be, launches[3])
    judge(None, dg, db, what + " params")


# ---- projection ------------------------------------------------------------------------------------------------------------------------
def proj_case(be, dtype, cin, cout, dhw, launches, bias, prologue, with_dx, seed=8):
    """mi355_proj_fwd and mi355_proj_bwd on one input; `launches` = (forward's, backward's)."""
    g = torch.Generator().manual_seed(seed)
    n = 2
    x = act(be, values((n, cin, *dhw), g, dtype), dtype, cin + 4, 4)
    w = torch.randn(cout, cin, generator=g) * 0.2
    b = torch.randn(cout, generator=g) if bias else None
    sc = torch.rand(n, cin, generator=g) + 0.5 if prologue else None
    sh = torch.randn(n, cin, generator=g) * 0.3 if prologue else None
    slope = 0.01
    pk = dict(scale=dev(be, sc), shift=dev(be, sh), slope=slope) if prologue else {}
    dz = torch.randn(n, cout, *dhw, generator=g)
    t = widen(x)
    if prologue:
        u = t * sc.double()[:, :, None, None, None] + sh.double()[:, :, None, None, None]
        t = torch.maximum(u, u * float(torch.tensor(slope, dtype=F32)))
    what = f"proj {dtype} {cin}->{cout} {dhw} bias={bias} prologue={prologue} dx={with_dx}"
    logits = torch.full((n, cout, *dhw), float("nan")).to(be.device)
    take(be)
    be.proj_fwd(x, dev(be, w), dev(be, b), logits, **pk)
    launched(be, launches[0])
    ref = torch.einsum("ncdhw,kc->nkdhw", t, w.double())
    if bias:
        ref = ref + b.double()[None, :, None, None, None]
    bounded(A.store_err(logits, ref, F32), what + " logits")
    dx = out_act(be, (n, cin, *dhw), dtype, cin + 8, 8) if with_dx else None
    dw = torch.full((cout, cin), float("nan")).to(be.device)
    dbias = torch.full((cout,), float("nan")).to(be.device) if bias else None
    be.proj_bwd(x, dev(be, w), dev(be, dz), dx, dw, dbias, **pk)
    launched(be, launches[1])
    bounded(A.store_err(dw, torch.einsum("nkdhw,ncdhw->kc", dz.double(), t), F32), what + " dw")
    if bias:
        bounded(A.store_err(dbias, dz.double().sum((0, 2, 3, 4)), F32), what + " dbias")
    if with_dx:
        bounded(A.store_err(widen(dx), torch.einsum("nkdhw,kc->ncdhw", dz.double(), w.double()), dtype), what + " dx")
        outside_untouched(dx)
    outside_untouched(x)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
ADAM_COUNTS = (1, 3, 4, 5, 1023, 4099)
ADAM_STEPS = (1, 2, 1000, 10 ** 6)
ADAM_SCALES = (1.0, 2.0 ** -16, 3.0)
ADAM_DECAYS = (0.0, 0.01)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def ulp32(t):
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -126))) - 23.0)


def adam_case(be, count, step, wd, gs, seed=9):
    """One step from a given state. |g * gs| is log-uniform over 1e-15 .. 1e3 with exact zeros among them; exp_avg_sq is non-negative
    with zeros; exp_avg and the parameter carry the gradient's sign (module docstring). The arrays are exactly `count` long."""
    g_ = torch.Generator().manual_seed(seed + count + step % 997)
    mag = torch.pow(10.0, torch.rand(count, generator=g_, dtype=torch.float64) * 18.0 - 15.0)
    sign = torch.where(torch.rand(count, generator=g_) < 0.5, -1.0, 1.0).double()
    zero = torch.rand(count, generator=g_) < 0.1
    if count >= 4:
        sign[count - 1], mag[count - 1], zero[count - 1] = -1.0, 0.37, False      # the last element (the tail loop's where count % 4) moves
    grad = (sign * mag / gs).float()
    grad[zero] = 0.0
    m = (sign * torch.randn(count, generator=g_).abs().double() * mag).float()
    v = (torch.rand(count, generator=g_).double() * mag * mag).float()
    v[torch.rand(count, generator=g_) < 0.15] = 0.0
    p = (sign * (torch.randn(count, generator=g_).abs().double() + 0.1)).float()
    pd, gd, md, vd = (torch.empty(count, dtype=F32, device=be.device).copy_(t) for t in (p, grad, m, v))
    take(be)
    be.adam_step(pd, gd, md, vd, LR, B1, B2, EPS, wd, step, grad_scale=gs)
    launched(be, ["adam_kernel"])
    assert torch.equal(gd.cpu(), grad), "the gradient was written"
    p64, m64, v64 = p.double(), m.double(), v.double()
    g64 = grad.double() * gs
    pr, mr, vr = p64.clone(), m64.clone(), v64.clone()
    O.adam_step(pr, g64, mr, vr, LR, B1, B2, EPS, wd, step)
    gabs = g64.abs() + wd * p64.abs()
    what = f"adam count={count} step={step} wd={wd} gs={gs}"
    for name, got, ref, allow in (("m", md, mr, (K_ADAM_M + 1) * U * (B1 * m64.abs() + (1 - B1) * gabs)),
                                  ("v", vd, vr, (K_ADAM_V + 1) * U * (B2 * v64 + (1 - B2) * gabs * gabs)),
                                  ("p", pd, pr, 0.5 * ulp32(pr) + (K_ADAM_P + 1) * U * (pr - p64).abs())):
        err = (got.cpu().double() - ref).abs()
        bad = ~(err <= allow)
        assert not bool(bad.any()), (what, name, int(bad.sum()), torch.nonzero(bad).flatten()[:4].tolist(), float(err[bad].max()), float(allow[bad].min()))
    return float(((pd.cpu().double() - pr).abs() / (0.5 * ulp32(pr) + (K_ADAM_P + 1) * U * (pr - p64).abs())).max())


def adam_tail_case(be):
    """The count % 4 elements after the last whole float4 are the tail loop's: every element must have moved."""
    for count in (1, 3, 5, 4099):
        p, g, m, v = (torch.full((count,), x, device=be.device) for x in (1.0, 0.5, 0.0, 0.0))
        be.adam_step(p, g, m, v, LR, B1, B2, EPS, 0.0, 1)
        assert bool((p < 1.0).all() and (m > 0).all() and (v > 0).all()), count


# ---- exhaustive conversions ------------------------------------------------------------------------------------------------------------------
def all_patterns(dtype):
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def conversion_inputs(src, dst):
    """Every input the direction src -> dst is held on, as a 1-D tensor of `src` whose length is a multiple of 4."""
    if src != F32:
        return all_patterns(src)
    p = all_patterns(dst)
    finite = torch.isfinite(p.float())
    a = p.float()
    if dst == BF16:                                                    # the midpoint to the upper neighbour: the next 16 bits set
        mid = (a.view(torch.int32) + 0x8000).view(F32)
    else:                                                              # fp16: 11-bit significands, the mean of two neighbours is exact in fp32
        up = (p.view(torch.int16).to(torch.int32) + 1).to(torch.int16).view(F16).float()
        top = (p.view(torch.int16) & 0x7fff) == 0x7bff                 # above the largest finite value: the overflow threshold, 65520
        mid = torch.where(top, torch.copysign(torch.tensor(65520.0), a), (a + up) * 0.5)
    mid = torch.where(finite, mid, a)
    below, above = (mid.view(torch.int32) - 1).view(F32), (mid.view(torch.int32) + 1).view(F32)
    thr = torch.tensor([65520.0, -65520.0, 65504.0, -65504.0, 65536.0, 3.3895314e38, -3.3895314e38, 3.4028235e38])
    thr = torch.cat((thr, (thr.view(torch.int32) - 1).view(F32), (thr.view(torch.int32) + 1).view(F32)))
    sub = torch.tensor([1, 2, 0x3fffff, 0x400000, 0x7fffff, 0x800000, 0x32ffffff, 0x33000000, 0x33000001, 0x33800000], dtype=torch.int32)
    sub = torch.cat((sub, sub | -0x80000000)).view(F32)                # fp32 subnormals and the fp16 underflow boundary 2^-25, both signs
    spec = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])
    nans = torch.tensor([0x7f800001, 0x7fffffff, -1, -0x7fffff, 0x7fc00000, 0x7f80ffff], dtype=torch.int32).view(F32)
    t = torch.cat((a, mid, below, above, thr, sub, spec, nans))
    return torch.cat((t, torch.zeros(-t.numel() % 4)))


def conversion_case(be, src, dst):
    t = conversion_inputs(src, dst)
    x = ops.Act(t.view(1, 1, 1, -1, 4).to(be.device).contiguous(), 0, 4)
    y = ops.Act(torch.zeros(1, 1, 1, t.numel() // 4, 4, dtype=dst).to(be.device), 0, 4)
    take(be)
    be.cast(x, out=y)
    launched(be, ["(cast_kernel<TS, TD>)"])
    same_bits(y.buf.view(-1), t.to(dst), f"{src} -> {dst}, {t.numel()} values")


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, entry, dtype, launches, fn, *args, **kw):
        self.name, self.entry, self.dtype, self.launches, self.fn, self.args, self.kw = name, entry, dtype, launches, fn, args, kw

    def claims(self):
        """(entry point, kernel expression, storage type) triples of this row."""
        flat = [e for l in self.launches for e in (l if isinstance(l, (list, tuple)) else [l])]
        entries = self.entry if isinstance(self.entry, tuple) else (self.entry,) * len(flat)
        if isinstance(self.entry, tuple) and len(entries) != len(flat):        # one entry point per call: (entry, its launches) in turn
            entries = [en for en, l in zip(self.entry, self.launches) for _ in l]
        return {(en, e, self.dtype) for en, e in zip(entries, flat)}

    def run(self, be):
        self.fn(be, *self.args, launches=self.launches, **self.kw)

    def __repr__(self):
        return self.name


def tname(dt):
    return {F32: "f32", BF16: "bf16", F16: "f16"}[dt] if not isinstance(dt, tuple) else "-".join(tname(d) for d in dt)


UPF, UPB = "mi355_upsample2x_fwd", "mi355_upsample2x_bwd"
UF_ROWS4, UF_ROWS8 = "(upsample2x_fwd_rows_kernel<T, 4>)", "(upsample2x_fwd_rows_kernel<T, 8>)"
UF_GRID4, UF_GRID8 = "(upsample2x_fwd_kernel<T, 4>)", "(upsample2x_fwd_kernel<T, 8>)"
UB4, UB8 = "(upsample2x_bwd_kernel<T, 4>)", "(upsample2x_bwd_kernel<T, 8>)"
MOM4, MOM8, MOMFIN = "(gn_moments_kernel<T, 4>)", "(gn_moments_kernel<T, 8>)", "gn_moments_finalize_kernel"
PART4, PART8 = "(gn_bwd_partial_kernel<T, 4>)", "(gn_bwd_partial_kernel<T, 8>)"
APPLY4, APPLY8, APPLY_ROWS8 = "(gn_bwd_apply_kernel<T, 4>)", "(gn_bwd_apply_kernel<T, 8>)", "(gn_bwd_apply_rows_kernel<T, 8>)"
BFIN, BPAR = "gn_bwd_finalize_kernel", "gn_bwd_param_kernel"
ODD, EMPTY = (3, 5, 7), (1, 17, 17)      # V = 105: odd; V = 289: B = 18 blocks of 17 voxels, the last one empty


def build_rows():
    rows = []

    def add(name, entry, dtypes, launches, fn, *args, **kw):
        for dt in (dtypes if isinstance(dtypes, tuple) else (dtypes,)):
            rows.append(Row(f"{name}-{tname(dt)}", entry, dt, launches, (lambda be, *a, _f=fn, _dt=dt, **kk: _f(be, _dt, *a, **kk)), *args, **kw))

    # up-sampling forward: cat is a slice at c0 != 0 of a wider buffer throughout
    add("up_fwd-rows4-C8", UPF, F32, [UF_ROWS4], upsample_fwd_case, 8, "g1", cat_view=(16, 8))
    add("up_fwd-grid4-C12", UPF, F32, [UF_GRID4], upsample_fwd_case, 12, "g2", cat_view=(16, 4))                 # Q = 3
    add("up_fwd-rows4-C256-xloop", UPF, F32, [UF_ROWS4], upsample_fwd_case, 256, "xloop", cat_view=(260, 4))     # Q = 64, XPB = 4 < Wc = 7
    add("up_fwd-rows8-C16", UPF, (BF16,), [UF_ROWS8], upsample_fwd_case, 16, "g3", cat_view=(24, 8))
    add("up_fwd-rows8-C16", UPF, (F16,), [UF_ROWS8], upsample_fwd_case, 16, "g4", cat_view=(24, 8))
    add("up_fwd-grid8-C24", UPF, LP, [UF_GRID8], upsample_fwd_case, 24, "g1", cat_view=(32, 8))                  # Q = 3
    add("up_fwd-rows4-C8-at-c0-4", UPF, LP, [UF_ROWS4], upsample_fwd_case, 8, "g2", cat_view=(16, 4))            # 8- but not 16-byte aligned
    add("up_fwd-rows4-C4", UPF, LP, [UF_ROWS4], upsample_fwd_case, 4, "g4", cat_view=(8, 4))                     # c % 8 == 4, Q = 1
    add("up_fwd-grid4-C12", UPF, LP, [UF_GRID4], upsample_fwd_case, 12, "g3", cat_view=(16, 4))                  # c % 8 == 4, Q = 3
    # up-sampling backward: dcat is the slice
    add("up_bwd-4-C12", UPB, F32, [UB4], upsample_bwd_case, 12, "g1", dcat_view=(16, 4))
    add("up_bwd-4-C8", UPB, F32, [UB4], upsample_bwd_case, 8, "g4", dcat_view=(16, 8))
    add("up_bwd-4-C12", UPB, LP, [UB4], upsample_bwd_case, 12, "g2", dcat_view=(16, 4))
    add("up_bwd-4-C8-at-c0-4", UPB, LP, [UB4], upsample_bwd_case, 8, "g3", dcat_view=(16, 4))
    add("up_bwd-8-C16", UPB, LP, [UB8], upsample_bwd_case, 16, "g4", dcat_view=(24, 8))
    add("up_bwd-8-C24", UPB, LP, [UB8], upsample_bwd_case, 24, "g3", dcat_view=(32, 8))
    # add / chscale
    for alias in (False, True):
        add(f"add-alias{int(alias)}", "mi355_add", ALL, ["add_kernel<T>"], add_case, alias=alias)
        add(f"chscale-4-C12-alias{int(alias)}", "mi355_chscale", ALL, ["(chscale_kernel<T, 4>)"], chscale_case, 12, view=(16, 4), alias=alias)
    add("chscale-4-C8-at-c0-4", "mi355_chscale", LP, ["(chscale_kernel<T, 4>)"], chscale_case, 8, view=(16, 4))
    add("chscale-8-C16", "mi355_chscale", LP, ["(chscale_kernel<T, 8>)"], chscale_case, 16, view=(24, 8))
    add("chscale-8-C16-alias", "mi355_chscale", LP, ["(chscale_kernel<T, 8>)"], chscale_case, 16, alias=True)
    # cast: nine (source, destination) pairs of one expression; layout: C = 1, 3 and 4 into ld = 8
    for s in ALL:
        for d in ALL:
            rows.append(Row(f"cast-{tname(s)}-{tname(d)}", "mi355_cast", (s, d), ["(cast_kernel<TS, TD>)"],
                            (lambda be, launches, _s=s, _d=d: cast_case(be, _s, _d, launches))))
    for c in (1, 3, 4):
        add(f"layout-C{c}", ("mi355_ncdhw_to_ndhwc", "mi355_ndhwc_to_ncdhw"), ALL, ["ncdhw_to_ndhwc_kernel<T>", "ndhwc_to_ncdhw_kernel<T>"], layout_case, c)
    # norm statistics: groups 1, C and C / 4
    for entry, fn, fin, gr in (("mi355_gn_moments", moments_case, [], lambda *g: ()), ("mi355_gn_stats", stats_case, [MOMFIN], lambda *g: g)):
        tag = entry[9:]
        add(f"{tag}-4-C12", entry, F32, [MOM4] + fin, fn, 12, ODD, *gr(3), view=(16, 4))
        add(f"{tag}-4-C8-empty", entry, F32, [MOM4] + fin, fn, 8, EMPTY, *gr(1))
        add(f"{tag}-4-C12", entry, LP, [MOM4] + fin, fn, 12, ODD, *gr(12), view=(16, 4))
        add(f"{tag}-8-C16-empty", entry, LP, [MOM8] + fin, fn, 16, EMPTY, *gr(1), view=(24, 8))
        add(f"{tag}-8-C24", entry, LP, [MOM8] + fin, fn, 24, ODD, *gr(6))                                       # Q * R = 3 * 85 = 255 threads
    add("gn_finalize-folded-C12", ("mi355_gn_moments", "mi355_gn_records_reduce", "mi355_gn_finalize"), F32,
        [[MOM4], ["(gn_records_reduce_kernel<3>)"], [MOMFIN]], lambda be, dt, *a, launches, **k: stats_case(
            be, dt, *a, launches=[e for l in launches for e in l], **k), 12, ODD, 3, fold=4)
    # act(GroupNorm) backward
    GB = "mi355_gn_act_bwd"
    add("gn_bwd-4-C12", GB, F32, [PART4, BFIN, BPAR, APPLY4], gn_bwd_case, 12, ODD, 3, 0.01, addend=(16, 4), view=(16, 4), dx_view=(20, 8))
    add("gn_bwd-4-C8-empty", GB, F32, [PART4, BFIN, BPAR, APPLY4], gn_bwd_case, 8, EMPTY, 8, 0.0, params="b")
    add("gn_bwd-4-C12", GB, LP, [PART4, BFIN, BPAR, APPLY4], gn_bwd_case, 12, ODD, 12, 0.0, params="g", view=(16, 4))     # Q * R = 3 * 85
    add("gn_bwd-rows8-C16-empty", GB, LP, [PART8, BFIN, BPAR, APPLY_ROWS8], gn_bwd_case, 16, EMPTY, 1, 0.01, addend=(24, 8), params="b")  # pairs + tail
    add("gn_bwd-rows8-C64", GB, LP, [PART8, BFIN, BPAR, APPLY_ROWS8], gn_bwd_case, 64, ODD, 16, 0.0, view=(72, 8))           # VPB = 32: pairs + tail
    add("gn_bwd-8-C24", GB, LP, [PART8, BFIN, APPLY8], gn_bwd_case, 24, ODD, 6, 0.01, addend=(32, 8), params="", dx_view=(32, 8))   # Q * R = 255
    add("gn_bwd-8-C24-noaddend", GB, LP, [PART8, BFIN, BPAR, APPLY8], gn_bwd_case, 24, EMPTY, 24, 0.0)
    add("gn_bwd-addend-only-misaligned", GB, LP, [PART8, BFIN, BPAR, APPLY4], gn_bwd_case, 16, ODD, 4, 0.01, addend=(20, 0))   # addend_ld % 8 == 4
    FU = (GB, "mi355_gn_records_reduce", "mi355_gn_act_bwd_fused", "mi355_gn_bwd_params")
    RED2 = ["(gn_records_reduce_kernel<2>)"]
    add("gn_bwd-fused-C12", FU, F32, [[PART4, BFIN, BPAR, APPLY4], RED2, [BFIN, BPAR, APPLY4], [BFIN, BPAR]], gn_bwd_case, 12, ODD, 3, 0.01,
        addend=(12, 0), route="fused")
    add("gn_bwd-fused-C16", FU, LP, [[PART8, BFIN, BPAR, APPLY_ROWS8], RED2, [BFIN, BPAR, APPLY_ROWS8], [BFIN, BPAR]], gn_bwd_case, 16, ODD, 4, 0.0,
        route="fused")
    # projection: cout 1, 2, 3, 8 (both class parities, PROJ_MAX_COUT); cin 4 and 96 (PROJ_MAX_CIN: 8 * 96 + 8 = 776 reduce entries, all four
    # part[] slots); V = 1, 127, 128, 129; with and without bias, prologue, dx
    PJ = ("mi355_proj_fwd", "mi355_proj_bwd")
    PL = [["proj_fwd_kernel<T>"], ["proj_bwd_kernel<T>", "proj_reduce_kernel"]]
    add("proj-4-1-V1", PJ, ALL, PL, proj_case, 4, 1, (1, 1, 1), bias=False, prologue=False, with_dx=True)
    add("proj-96-8-V127", PJ, ALL, PL, proj_case, 96, 8, (1, 1, 127), bias=True, prologue=True, with_dx=False)
    add("proj-4-2-V128", PJ, ALL, PL, proj_case, 4, 2, (2, 8, 8), bias=True, prologue=False, with_dx=True)
    add("proj-96-3-V129", PJ, ALL, PL, proj_case, 96, 3, (1, 3, 43), bias=False, prologue=True, with_dx=True)
    rows.append(Row("adam", "mi355_adam_step", F32, ["adam_kernel"], lambda be, launches: adam_case(be, 5, 2, 0.01, 3.0)))
    return rows


ROWS = build_rows()
ROW_IDS = [r.name for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)

# LAUNCHes of the two sources whose entry points are outside this table (sliding-window inference: tests/test_inferer.py)
OUTSIDE_THE_TABLE = {"sw_accumulate_kernel", "sw_normalize_kernel", "sw_gather_kernel", "sw_accumulate_batch_kernel"}


def launch_expressions(source):
    """First argument of every LAUNCH( of a source file, as the emulator records it."""
    text = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", source)).read()
    return {re.sub(r"\s+", " ", m.group(1).strip()) for m in re.finditer(r"\bLAUNCH\(\s*(\((?:[^()]|\([^()]*\))*\)|[^,()]+)", text)}


def check_table_is_complete():
    claimed = {e for r in ROWS for _, e, _ in r.claims()}
    in_source = launch_expressions("pointwise.hip") | launch_expressions("norm.hip")
    assert len(in_source) > 25 and OUTSIDE_THE_TABLE <= in_source, in_source
    assert in_source - OUTSIDE_THE_TABLE <= claimed, sorted(in_source - OUTSIDE_THE_TABLE - claimed)
    assert claimed - in_source == {"adam_kernel"}, claimed - in_source
    triples = {t for r in ROWS for t in r.claims()}
    # every templated streaming form on every storage type it is compiled for
    for entry, exprs, dtypes in ((UPF, (UF_ROWS4, UF_GRID4), ALL), (UPF, (UF_ROWS8, UF_GRID8), LP), (UPB, (UB4,), ALL), (UPB, (UB8,), LP),
                                 ("mi355_add", ("add_kernel<T>",), ALL), ("mi355_chscale", ("(chscale_kernel<T, 4>)",), ALL),
                                 ("mi355_chscale", ("(chscale_kernel<T, 8>)",), LP), ("mi355_gn_moments", (MOM4,), ALL), ("mi355_gn_moments", (MOM8,), LP),
                                 ("mi355_gn_stats", (MOM4, MOMFIN), ALL), ("mi355_gn_stats", (MOM8,), LP), ("mi355_gn_act_bwd", (PART4, APPLY4, BFIN, BPAR), ALL),
                                 ("mi355_gn_act_bwd", (PART8, APPLY8, APPLY_ROWS8), LP), ("mi355_gn_act_bwd_fused", (BFIN, BPAR, APPLY4), (F32,)),
                                 ("mi355_gn_act_bwd_fused", (APPLY_ROWS8,), LP), ("mi355_gn_bwd_params", (BFIN, BPAR), ALL),
                                 ("mi355_proj_fwd", ("proj_fwd_kernel<T>",), ALL), ("mi355_proj_bwd", ("proj_bwd_kernel<T>", "proj_reduce_kernel"), ALL),
                                 ("mi355_ncdhw_to_ndhwc", ("ncdhw_to_ndhwc_kernel<T>",), ALL), ("mi355_ndhwc_to_ncdhw", ("ndhwc_to_ncdhw_kernel<T>",), ALL),
                                 ("mi355_cast", ("(cast_kernel<TS, TD>)",), tuple((s, d) for s in ALL for d in ALL)),
                                 ("mi355_adam_step", ("adam_kernel",), (F32,))):
        for e in exprs:
            for dt in dtypes:
                assert (entry, e, dt) in triples, (entry, e, dt)


def check_geometry_is_covered():
    """Over the up-sampling rows, each axis sees: a low-resolution size of 1, a crop, padding at the end only, padding on both sides; every
    forward row writes, and every backward row reads, a slice at c0 != 0 of a wider buffer."""
    seen = {ax: set() for ax in range(3)}
    for r in ROWS:
        if r.entry not in (UPF, UPB):
            continue
        view = r.kw.get("cat_view") or r.kw.get("dcat_view")
        assert view and view[0] > r.args[0] and view[1] != 0, r
        lo, cat = GEOMETRY[r.args[1]]
        for ax in range(3):
            seen[ax] |= {"one"} if lo[ax] == 1 else set()
            seen[ax].add({-1: "crop", 0: "exact", 1: "end", 2: "both"}[cat[ax] - 2 * lo[ax]])
    for ax in range(3):
        assert {"one", "crop", "end", "both"} <= seen[ax], (ax, seen[ax])
    assert all(max(cat) <= 10 for _, cat in GEOMETRY.values())
