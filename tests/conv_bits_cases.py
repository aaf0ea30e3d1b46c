"""TEST INFRASTRUCTURE: the bit-exact pin of the conv entry points (csrc/conv3d_*.hip), modelled on tests/volume_bits_cases.py.

Every group builds small inputs from seeded CPU generators, runs conv entry points through `Backend` and returns {case name: sha256 over
dtype, shape and raw bytes of every output}. tests/test_conv_bits.py compares the digests with tests/golden/conv_bits.json on the emulator
and on the HIP library; tests/golden/make_conv_bits.py wrote that file from the commit BEFORE the conv sources were moved onto
csrc/conv_internal.h. A digest that moves is a change of behaviour, never a number to record again.

The cases: the executed form of the small shapes of tests/route_cases.py, one per route, forward and weight gradient; the Winograd forward
kernels, whose host path that commit rewrote, at the smallest shape where the shared argument fill can go wrong -- 12 input channels (the
2-D form pads them to 16, the 3-D form does not), 10 output channels (the scalar store path), 3 x 9 x 17 voxels (ragged tiles on every
axis), two samples, y a channel window (c0 = 4, ld = 16) of a wider buffer -- plain, with residual + channel scale + moments, with a
normalised input, and as a dgrad with the norm-backward sums; the Winograd weight gradient and the fused first-layer backward."""
import hashlib
import json
import os

import torch

import route_cases as R
from op_cases import Act, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bits.json")
GROUPS = ("route_fwd", "route_wgrad", "wino_fwd", "wino_wgrad_c4_bwd")
# the routes of tests/route_cases.py that are the same kernel at a large volume are left to the launch-geometry pin
FWD_SKIPPED = ("lp_tile_wide", "mfma_cfg4_big", "mfma_cfg8")
STORAGE = {R.F32: torch.float32, R.BF16: torch.bfloat16}


def digest(*outs):
    h = hashlib.sha256()
    for t in outs:
        t = t.detach().cpu().contiguous()
        h.update(str(t.dtype).encode() + str(tuple(t.shape)).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _act(be, spec, g, ld=None, c0=0, zero=False):
    """(n, d, h, w, c, storage) -> an Act of seeded normal values (zero: of 7.0, an output to be overwritten) on the backend's device."""
    n, d, h, w, c, st = spec
    buf = torch.full((n, d, h, w, ld or c), 7.0)
    if not zero:
        buf[..., c0:c0 + c] = torch.randn(n, d, h, w, c, generator=g)
    return Act(buf.to(STORAGE[st]).to(be.device).contiguous(), c0, c)


def _affine(be, n, c, g):
    return (torch.rand(n, c, generator=g) + 0.5).to(be.device), (torch.randn(n, c, generator=g) * 0.3).to(be.device)


def _with_env(env, f):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return f()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def route_fwd(be):
    out = {}
    for i, (cid, (xs, ys, kd, stride, pad, im, prec, _, env)) in enumerate(R.FWD.items()):
        if cid in FWD_SKIPPED:
            continue
        g = torch.Generator().manual_seed(200 + i)
        x, y = _act(be, xs, g), _act(be, ys, g, zero=True)
        dgrad = im == "ZERO_INSERT"
        w = torch.randn(*((xs[4], ys[4]) if dgrad else (ys[4], xs[4])), kd, kd, kd, generator=g) * (xs[4] * kd ** 3) ** -0.5
        kw = {}
        if im == "AFFINE_ACT":
            sc, sh = _affine(be, xs[0], xs[4], g)
            kw = dict(slope=0.01, scale=sc, shift=sh)
        be.set_precision(prec)
        try:
            wp = be.pack_weight(w.contiguous().to(be.device), 1 if dgrad else 0)
            _with_env(env, lambda: be.conv_fwd(x, wp, y, kd, stride, pad, in_mode=getattr(ops, "IN_" + im), out_dhw=ys[1:4], **kw))
        finally:
            be.set_precision("fp32")
        out["fwd:" + cid] = digest(y.buf)
    return out


def route_wgrad(be):
    out = {}
    for i, (cid, (xs, dys, kd, stride, pad, im, prec, om)) in enumerate(R.WGRAD.items()):
        g = torch.Generator().manual_seed(300 + i)
        x, dy = _act(be, xs, g), _act(be, dys, g)
        kw = {}
        if im == "AFFINE_ACT":
            sc, sh = _affine(be, xs[0], xs[4], g)
            kw = dict(slope=0.01, scale=sc, shift=sh)
        dw = torch.full((8 * dys[4], xs[4]) if om == "D2S" else (dys[4], xs[4], kd, kd, kd), 3.0, device=be.device)
        be.set_precision(prec)
        try:
            be.conv_wgrad(x, dy, dw, kd, stride, pad, in_mode=getattr(ops, "IN_" + im), out_mode=getattr(ops, "OUT_" + om), **kw)
        finally:
            be.set_precision("fp32")
        out["wgrad:" + cid] = digest(dw)
    return out


WINO_SHAPE = dict(n=2, cin=12, cout=10, dhw=(3, 9, 17), c0=4, ld=16)


def wino_fwd(be):
    s = WINO_SHAPE
    n, cin, cout, (d, h, w) = s["n"], s["cin"], s["cout"], s["dhw"]
    out = {}
    for form in ("2d", "3d"):
        for run in ("plain", "residual chscale moments", "normalised input", "dgrad norm-backward sums"):
            g = torch.Generator().manual_seed(400)
            x = _act(be, (n, d, h, w, cin, R.F32), g)
            y = _act(be, (n, d, h, w, cout, R.F32), g, ld=s["ld"], c0=s["c0"], zero=True)
            wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (cin * 27) ** -0.5
            kw, extra = {}, []
            mode = 0
            if run == "residual chscale moments":
                kw = dict(residual=_act(be, (n, d, h, w, cout, R.F32), g, ld=20, c0=8),
                          chscale=((torch.rand(n, cout, generator=g) > 0.3).float() * 1.25).to(be.device), moments=True)
            elif run == "normalised input":
                sc, sh = _affine(be, n, cin, g)
                kw = dict(in_mode=ops.IN_AFFINE_ACT, slope=0.01, scale=sc, shift=sh)
            elif run == "dgrad norm-backward sums":
                # x is the gradient of a conv from `cout` to `cin` channels; y the gradient wrt act(norm(gx)), gx of y's shape
                wt, mode = wt.permute(1, 0, 2, 3, 4).contiguous(), 1
                gx = _act(be, (n, d, h, w, cout, R.F32), g, ld=20, c0=8)
                mr = torch.stack([torch.randn(n, 5, generator=g) * 0.1, torch.rand(n, 5, generator=g) + 0.5], -1).contiguous().to(be.device)
                sc, sh = _affine(be, n, cout, g)
                kw = dict(gnb=(gx, (mr, sc, sh), 5, 0.01))
            parts = be.conv_fwd_wino(x, be.wino_pack_weight(wt.to(be.device), mode, form), y, **kw)
            if y.mom is not None:
                extra.append(y.mom[0][0])
            if parts is not None:
                extra.append(parts[0])
            assert len(extra) == (run in ("residual chscale moments", "dgrad norm-backward sums")), (form, run)
            out[f"wino {form} {run}"] = digest(y.buf, *extra)
    return out


def wino_wgrad_c4_bwd(be):
    out = {}
    g = torch.Generator().manual_seed(500)
    x, dy = _act(be, (1, 4, 8, 16, 32, R.F32), g), _act(be, (1, 4, 8, 16, 32, R.F32), g)
    dw = torch.full((32, 32, 3, 3, 3), 3.0, device=be.device)
    old = be.wgrad_form
    be.wgrad_form, be.WINO_MIN_VOXELS = "wino", 0
    calls = []
    orig = be.lib.mi355_conv3d_wgrad_wino
    be.lib.mi355_conv3d_wgrad_wino = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        be.conv_wgrad(x, dy, dw, 3, 1, 1)
    finally:
        be.lib.mi355_conv3d_wgrad_wino = orig
        be.wgrad_form = old
        del be.WINO_MIN_VOXELS
    assert calls, "the Winograd weight gradient did not take its case"
    out["wgrad_wino 32->32"] = digest(dw)

    x, dy = _act(be, (1, 4, 8, 16, 4, R.F32), g), _act(be, (1, 4, 8, 16, 32, R.F32), g)
    gam, bet = (torch.rand(4, generator=g) + 0.5).to(be.device), (torch.randn(4, generator=g) * 0.3).to(be.device)
    mr, sc, sh = be.gn_stats(x, 4, 1e-5, gam, bet)
    assert be.c4_bwd_supported(x, dy, ops.IN_AFFINE_ACT, 0.01, sc, sh)
    wp = be.pack_weight((torch.randn(32, 4, 3, 3, 3, generator=g) * 0.1).to(be.device), 1)
    dw = torch.full((32, 4, 3, 3, 3), 7.0, device=be.device)
    dgam, dbet = torch.full((4,), 7.0, device=be.device), torch.full((4,), 7.0, device=be.device)
    be.c4_bwd(x, dy, wp, dw, 4, gam, mr, sc, sh, dgam, dbet, slope=0.01)
    out["c4_bwd 4->32"] = digest(dw, dgam, dbet)
    return out


_DIGESTS = {}


def digests(be, group):
    """{case name: sha256 hex} of one group of GROUPS on backend `be`; computed once per backend and shared."""
    key = (id(be), group)
    if key not in _DIGESTS:
        _DIGESTS[key] = globals()[group](be)
    return _DIGESTS[key]


def check(be, section, group):
    """The digests of `group` on `be` against the committed section ("emu" | "gfx950"), exactly. A case the section leaves out (one whose
    digest differed between two runs of the pinned commit itself: tests/golden/make_conv_bits.py) is computed and not compared."""
    doc = json.load(open(GOLDEN))
    want, unstable = doc[section], doc.get(section + "_unstable", {})
    got = digests(be, group)
    assert got, group
    missing = sorted(set(got) - set(want) - set(unstable))
    assert not missing, f"{GOLDEN} [{section}] has no digest for {missing}"
    moved = sorted(k for k in got if k in want and got[k] != want[k])
    assert not moved, f"{len(moved)} of {len(got)} outputs of {group} changed bits on {section}: {moved}"


def check_complete(be, section):
    """Every digest of the committed section is still produced by some group: a case dropped from a group does not vanish silently."""
    doc = json.load(open(GOLDEN))
    want = set(doc[section]) | set(doc.get(section + "_unstable", {}))
    got = [k for group in GROUPS for k in digests(be, group)]
    assert len(got) == len(set(got)), "two groups produce a case of the same name"
    assert set(got) == want, f"no longer produced: {sorted(want - set(got))}; not in the fixture: {sorted(set(got) - want)}"
