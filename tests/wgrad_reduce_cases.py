"""TEST INFRASTRUCTURE: cases of the split-K slab reduction behind every weight gradient (`wgrad_reduce_kernel`, csrc/conv3d_wgrad.hip),
shared by the emulator tests (tests/test_wgrad_reduce_emu.py) and their GPU twins (tests/test_wgrad_reduce_gpu.py).

The reduction is driven through `be.conv_wgrad`. Every case runs the same call twice -- with MI355_WGRAD_REDUCE_ROWS=0 (the scatter form:
one workgroup per (pair, tap) tile, dwords at a stride of 4 T bytes) and without it (the rows form: contiguous pieces of dw) -- and asks
for two things: the two dw are the same bits (the rows form keeps every element's summation order), and dw agrees with the fp64
evaluation of the same gradient to 1e-5 of max |dw| (the bound tests/test_launch_audit.py holds `conv_wgrad` launches to).
The volumes are the smallest whose plans give the slab counts named in CASES; the slab count a case ran with is read back from the
workspace the call asked for (every producer sizes it pairs x slabs x taps x 4 KiB) and asserted, and printed with `parts` and T.
"""
import ctypes
import importlib
import os

import torch
import torch.nn.functional as F

import act_storage_cases as S
import op_cases as C

ops = importlib.import_module("3dunetcnn_amd.ops")
SWITCH = "MI355_WGRAD_REDUCE_ROWS"
BOUND = 1e-5

# name: (n, cin, cout, dhw, kd, slabs, parts). 3x3x3 stride 1 below the Winograd threshold runs the plane ring: one slab per 4 x 8 column
# and sample while there are fewer than 512 / pairs of them, so the batch size sets the slab count of the 32 -> 32 cases.
#   slabs 1 / 5: the tail loop only; 29 / 33: the unrolled loop (8 slabs per wave and trip) with and without a tail; 61: two trips.
#   parts = 4: fewer than 256 (pair, tap) tiles, four workgroups per tile's worth of outputs; parts = 1: 128 -> 96 has 4 * 3 * 27 = 324.
#   ragged: 40 -> 72 fills the last channel tile partly in both directions (8 of 32 ci, 8 of 32 co).
#   k1: T = 1, the 1x1x1 weight gradient (whole rows per piece); its voxel tiles are split 4 ways per workgroup, 2 workgroups -> 8 slabs.
CASES = {
    "slabs1": (1, 32, 32, (2, 4, 8), 3, 1, 4),
    "slabs5": (5, 32, 32, (2, 4, 8), 3, 5, 4),
    "slabs29": (29, 32, 32, (2, 4, 8), 3, 29, 4),
    "slabs33": (33, 32, 32, (2, 4, 8), 3, 33, 4),
    "slabs61": (61, 32, 32, (1, 4, 8), 3, 61, 4),
    "parts1": (2, 128, 96, (2, 4, 8), 3, 2, 1),
    "ragged": (3, 40, 72, (2, 4, 8), 3, 3, 4),
    "k1": (2, 64, 32, (8, 16, 16), 1, 8, 4),
}


def _launched(be):
    """Kernel expressions launched since the last call (the emulator records them; None on the GPU)."""
    if not hasattr(be.lib, "emu_take_launches"):
        return None
    buf = ctypes.create_string_buffer(4096)
    be.lib.emu_take_launches(buf, len(buf))
    return [k for k in buf.value.decode().split("\n") if k]


def _both_forms(be, call, numel, lead=0, guard=0):
    """Runs call(dw) with the switch off and on; dw is a view `lead` floats into a flat buffer with `guard` more floats behind it.
    Returns (dw scatter form, dw rows form, slab-workspace bytes asked for) after checking the floats around dw were left alone."""
    out, asked = [], []
    ws = be.ws
    be.ws = lambda nbytes: (asked.append(nbytes), ws(nbytes))[1]
    saved = os.environ.get(SWITCH)
    try:
        for form in ("0", None):
            if form is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = form
            buf = torch.full((lead + numel + guard,), 3.0).to(be.device)
            _launched(be)
            call(buf[lead:lead + numel])
            names = _launched(be)
            if names is not None:       # the emulator names what ran: the producer, then the reduction in the form asked for
                assert names[-1] == ("wgrad_reduce_scatter_kernel" if form == "0" else "wgrad_reduce_kernel"), (form, names)
            host = buf.cpu()
            assert bool((host[:lead] == 3.0).all()) and bool((host[lead + numel:] == 3.0).all()), ("floats around dw were written", form)
            out.append(host[lead:lead + numel].clone())
    finally:
        del be.ws
        if saved is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = saved
    assert asked[0] == asked[1]
    return out[0], out[1], asked[0]


def _check(name, dw_scatter, dw_rows, dw64, nbytes, cin, cout, T, slabs, parts):
    pairs = -(-cin // 32) * -(-cout // 32)
    got_slabs, got_parts = nbytes // (pairs * T * 4096), (4 if pairs * T < 256 else 1)
    err = float((dw_rows.double() - dw64.reshape(-1)).abs().max() / dw64.abs().max())
    print(f"wgrad reduce {name}: splits {got_slabs} parts {got_parts} T {T} pairs {pairs} err vs fp64 {err:.2e}")
    assert nbytes == pairs * got_slabs * T * 4096 and (got_slabs, got_parts) == (slabs, parts), (name, got_slabs, got_parts)
    assert torch.equal(dw_scatter.view(torch.int32), dw_rows.view(torch.int32)), (name, "the two forms differ in bits")
    assert err <= BOUND, (name, err)
    return err


def case_fp32(be, name, lead=0, guard=0):
    n, cin, cout, dhw, kd, slabs, parts = CASES[name]
    g = torch.Generator().manual_seed(17)
    x, dy = torch.randn(n, cin, *dhw, generator=g), torch.randn(n, cout, *dhw, generator=g)
    w = torch.zeros(cout, cin, kd, kd, kd, dtype=torch.float64, requires_grad=True)
    (dw64,) = torch.autograd.grad(F.conv3d(x.double(), w, padding=kd // 2), w, dy.double())
    xa, dya = C.to_act(be, x), C.to_act(be, dy)
    a, b, nbytes = _both_forms(be, lambda dw: be.conv_wgrad(xa, dya, dw.view(cout, cin, kd, kd, kd), kd, 1), dw64.numel(), lead, guard)
    return _check(name, a, b, dw64, nbytes, cin, cout, kd ** 3, slabs, parts)


def case_unaligned(be):
    """dw one float past a 16-byte boundary (as a slice of the flat gradient buffer may be), guard floats on both sides: the ragged case,
    whose pieces end inside channel quads and whose last tiles are cut by both guards."""
    return case_fp32(be, "ragged", lead=5, guard=7)


def case_lp_tr(be):
    """16-bit storage: bf16 tensors through conv3d_wgrad_lp_tr (LDS transpose reads), 5 x 9 x 18 in 4 x 8 columns of up to 16 planes."""
    n, cin, cout, dhw = 1, 32, 32, (5, 9, 18)
    g = torch.Generator().manual_seed(3)
    x, dy = S.bf16_values((n, cin, *dhw), g), S.bf16_values((n, cout, *dhw), g)
    w = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    (dw64,) = torch.autograd.grad(F.conv3d(x.double(), w, padding=1), w, dy.double())
    be.set_precision("bf16")
    try:
        xa, dya = S.acts(be, x)[1], S.acts(be, dy)[1]
        a, b, nbytes = _both_forms(be, lambda dw: be.conv_wgrad(xa, dya, dw.view(cout, cin, 3, 3, 3), 3, 1), dw64.numel())
    finally:
        be.set_precision("fp32")
    slabs = nbytes // (27 * 4096)
    return _check("lp_tr", a, b, dw64, nbytes, cin, cout, 27, slabs, 4)
