"""TEST INFRASTRUCTURE: the refusal table of the conv entry points (csrc/conv3d_*.hip).

For every entry point of ENTRIES one valid base call at 1 x 4 x 8 x 16 voxels (8 -> 32 channels; 4 -> 32 for the first-layer entries), then
one fault of FAULTS at a time: a null or misaligned argument, a malformed view, a descriptor no kernel takes, a norm-backward descriptor
with a hole in it, a workspace 4 bytes short, the shapes the Winograd kernels refuse. `rows(be)` returns {"entry | fault": {"value": the
status or the query's answer, "name": the kernel a config query printed, "launched": the kernels the emulator recorded}}.

tests/golden/conv_refusals.json holds the table of the commit BEFORE the conv sources were moved onto csrc/conv_internal.h
(tests/golden/make_conv_refusals.py). tests/test_conv_refusals.py compares every row on the emulator (a child process under
MI355_EMU_NOEXEC=1: `python tests/refusal_cases.py` prints the table) and the statuses / values on the HIP library. A row that moves is a
change of behaviour in a shared check, never a number to record again.

Every buffer is far larger than the base call needs (activations of 1032 channels, two samples), so a call that an entry point accepts in
spite of a fault -- one that does not read the damaged field -- stays inside its allocations on a GPU."""
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_refusals.json")
N0, D0, H0, W0, COUT0 = 1, 4, 8, 16, 32
CMAX = 1032                                    # channels every activation buffer has room for (the x.c = 1028 row is a real tensor)
FIRST_LAYER = ("c4_bwd", "c4_bwd_supported")
ENTRIES = ("fwd", "stats_blocks", "fwd_config", "wino_fwd", "wino3d_fwd", "wino_supported", "wino3d_supported", "wgrad", "wgrad_workspace",
           "wgrad_config", "wgrad_wino", "wgrad_wino_workspace", "c4_bwd", "c4_bwd_supported")


_POOL = {}


class Call:
    """One call's arguments: views, descriptor, weights (the weight-gradient entries: dw; c4_bwd: the dgrad pack), workspace."""
    def __init__(self, lib, dev, entry, shape=None):
        L = importlib.import_module("3dunetcnn_amd._lib")
        self.L, self.entry, self.keep = L, entry, []
        N, D, H, W, cin, COUT = shape or (N0, D0, H0, W0, 4 if entry in FIRST_LAYER else 8, COUT0)

        def buf(elems):      # the k-th buffer of every call is one allocation per device: no row reads what another wrote
            key = (str(dev), len(self.keep))
            t = _POOL.get(key)
            if t is None or t.numel() < elems:
                t = _POOL[key] = torch.zeros(elems, dtype=torch.float32, device=dev)
            self.keep.append(t)
            return t.data_ptr()
        act = 2 * D0 * H0 * W0 * CMAX
        assert 2 * D * H * W * max(cin, COUT, 16) <= act
        self.x = L.MiAct(buf(act), N, D, H, W, cin, cin, L.ACT_F32)
        self.y = L.MiAct(buf(act), N, D, H, W, COUT, COUT, L.ACT_F32)
        self.w = buf(3 << 20)
        self.other, self.scale, self.shift = buf(act), buf(4096), buf(4096)      # residual / normalised tensor; norm prologue
        self.rec, self.mean_rstd, self.dw = buf(1 << 20), buf(4096), buf(1 << 20)
        d = self.d = L.MiConvDesc()
        d.kd, d.stride, d.pad, d.in_mode, d.act_slope = 3, 1, 1, L.IN_PLAIN, 0.0
        d.out_d, d.out_h, d.out_w = D, H, W
        d.out_mode, d.precision, d.wformat = L.OUT_PLAIN, L.PREC_F32, L.W_PACKED
        if entry in FIRST_LAYER:                # the descriptor of the forward conv behind the first norm (ops.Backend.c4_bwd)
            d.in_mode, d.in_scale, d.in_shift = L.IN_AFFINE_ACT, self.scale, self.shift
        self.null = set()
        self.keep = list(self.keep)
        query = {"wgrad": lib.mi355_conv3d_wgrad_workspace, "wgrad_wino": lib.mi355_conv3d_wgrad_wino_workspace,
                 "c4_bwd": lib.mi355_conv3d_c4_bwd_workspace}.get(entry)
        self.ws_bytes = query(ctypes.byref(self.x), ctypes.byref(self.y), ctypes.byref(d)) if query else 0
        self.ws = buf(max(self.ws_bytes // 4, 1) + 16)

    def norm_input(self, slope=0.0):
        self.d.in_mode, self.d.in_scale, self.d.in_shift, self.d.act_slope = self.L.IN_AFFINE_ACT, self.scale, self.shift, slope

    def gn_bwd(self, **broken):
        f = self.L.MiGnBwdFuse(self.other, self.y.ld, self.scale, self.shift, self.mean_rstd, 4, 0.0, self.rec)
        for k, v in broken.items():
            setattr(f, k, v)
        self.keep.append(f)
        self.d.gn_bwd = ctypes.pointer(f)

    def arg(self, name):
        return None if name in self.null else ctypes.byref(getattr(self, name))


def _set(obj, **kw):
    def f(c):
        for k, v in kw.items():
            setattr(getattr(c, obj), k, v)
    return f


def _null(name):
    return lambda c: c.null.add(name)


def _slope(v):
    return lambda c: c.norm_input(v)


def _both(*fs):
    def f(c):
        for g in fs:
            g(c)
    return f


def _residual_short(c):
    c.d.residual, c.d.residual_ld = c.other, 16


def _off_by_4(name):
    def f(c):
        if name == "x":
            c.x.p += 4
        else:
            c.w += 4
            c.dw += 4
    return f


def _short_ws(c):
    c.ws_bytes = max(c.ws_bytes - 4, 0)


FAULTS = {
    "none": lambda c: None,
    # arguments
    "null x": _null("x"), "null y": _null("y"), "null weights": _null("w"), "null descriptor": _null("d"),
    "null x.p": _set("x", p=None), "x.c = 6": _set("x", c=6), "x.ld < x.c": _set("x", ld=4), "x.ld % 4 != 0": _set("x", ld=10),
    "y.ld < y.c": _set("y", ld=16), "x.n != y.n": _set("y", n=2), "x off by 4 bytes": _off_by_4("x"),
    "weights off by 4 bytes": _off_by_4("w"), "dtype = 7": _set("x", dtype=7),
    # descriptor
    "in_mode = 1 without scale": _set("d", in_mode=1, in_scale=None, in_shift=None),
    "in_mode = 1, slope 1.5": _slope(1.5), "in_mode = 1, slope -0.1": _slope(-0.1), "in_mode = 1, slope NaN": _slope(float("nan")),
    "in_mode = 4": _set("d", in_mode=4), "out_mode = 2": _set("d", out_mode=2), "precision = 9": _set("d", precision=9),
    "kd = 5": _set("d", kd=5), "stride = 3": _set("d", stride=3), "residual_ld < y.c": _residual_short,
    "moments_out and gn_bwd": _both(lambda c: setattr(c.d, "moments_out", c.rec), lambda c: c.gn_bwd()),
    "gn_bwd with in_mode = 1": _both(lambda c: c.gn_bwd(), _slope(0.0)),
    "gn_bwd, null gx": lambda c: c.gn_bwd(gx=None), "gn_bwd, groups = 0": lambda c: c.gn_bwd(groups=0),
    "gn_bwd, y.c % groups != 0": lambda c: c.gn_bwd(groups=5), "gn_bwd, gx_ld < y.c": lambda c: c.gn_bwd(gx_ld=16),
    "off_z = 1 with moments_out": _both(_set("d", off_z=1), lambda c: setattr(c.d, "moments_out", c.rec)),
    "workspace 4 bytes short": _short_ws,
    # the Winograd kernels' own
    "out_d != y.d": _set("d", out_d=D0 - 1), "x and y extents differ": _set("x", h=H0 - 2),
    "bf16 tensors": _both(_set("x", dtype=1), _set("y", dtype=1)),
    "x.c = 1028": _set("x", c=1028, ld=1028),
}


def run(lib, c, stream, name_buf):
    """The entry point's answer: (status or value, the name a config query printed or None)."""
    x, y, d = c.arg("x"), c.arg("y"), c.arg("d")
    w = None if "w" in c.null else c.w
    dw = None if "w" in c.null else c.dw
    e = c.entry
    if e == "fwd":
        return lib.mi355_conv3d_fwd(x, w, y, d, stream), None
    if e == "stats_blocks":
        return lib.mi355_conv3d_stats_blocks(x, y, d), None
    if e in ("fwd_config", "wgrad_config"):
        name_buf.value = b""
        rc = (lib.mi355_conv3d_fwd_config if e == "fwd_config" else lib.mi355_conv3d_wgrad_config)(x, y, d, name_buf, 96)
        return rc, name_buf.value.decode()
    if e == "wino_fwd":
        return lib.mi355_conv3d_wino_fwd(x, w, y, d, stream), None
    if e == "wino3d_fwd":
        return lib.mi355_conv3d_wino3d_fwd(x, w, y, d, stream), None
    if e == "wino_supported":
        return lib.mi355_conv3d_wino_supported(x, y, d), None
    if e == "wino3d_supported":
        return lib.mi355_conv3d_wino3d_supported(x, y, d), None
    if e == "wgrad":
        return lib.mi355_conv3d_wgrad(x, y, dw, d, c.ws, c.ws_bytes, stream), None
    if e == "wgrad_workspace":
        return lib.mi355_conv3d_wgrad_workspace(x, y, d), None
    if e == "wgrad_wino":
        return lib.mi355_conv3d_wgrad_wino(x, y, dw, d, c.ws, c.ws_bytes, stream), None
    if e == "wgrad_wino_workspace":
        return lib.mi355_conv3d_wgrad_wino_workspace(x, y, d), None
    if e == "c4_bwd":
        return lib.mi355_conv3d_c4_bwd(x, y, w, dw, d, c.mean_rstd, 4, c.rec, c.ws, c.ws_bytes, stream), None
    if e == "c4_bwd_supported":
        return lib.mi355_conv3d_c4_bwd_supported(x, y, d), None
    raise KeyError(e)


def gpu_rows(want):
    """The rows of the committed table `want` that run on a GPU: every row that launched nothing, every base call, and the 1028-channel
    tensor (a real one). A row that launched in spite of its fault -- the entry point does not read the damaged field -- stays with the
    emulator, which records the launch without running a kernel on a damaged argument."""
    return {k for k, r in want.items() if not r["launched"] or k.endswith(("| none", "| x.c = 1028"))}


def rows(be, take=None, only=None):
    """The table on backend `be` (only: these rows). take: None, or a function returning the kernels launched since its last call (the
    emulator)."""
    lib = be.lib
    stream = be.stream() if be.device.type == "cuda" else None
    name_buf = ctypes.create_string_buffer(96)
    out = {}
    for entry in ENTRIES:
        for fault, apply in FAULTS.items():
            if only is not None and f"{entry} | {fault}" not in only:
                continue
            c = Call(lib, be.device, entry)
            apply(c)
            if take:
                take()
            value, name = run(lib, c, stream, name_buf)
            r = {"value": value}
            if name is not None:
                r["name"] = name
            if take:
                r["launched"] = take()
            out[f"{entry} | {fault}"] = r
    if be.device.type == "cuda":
        torch.cuda.synchronize()
    return out


def check_values(got, want):
    """The statuses / values (and config names) of `got` against the committed table, exactly; every committed row still produced."""
    assert got and set(got) == set(want), f"rows that left: {sorted(set(want) - set(got))}; rows not in the fixture: {sorted(set(got) - set(want))}"
    moved = {k: (got[k]["value"], want[k]["value"]) for k in want if got[k]["value"] != want[k]["value"] or got[k].get("name") != want[k].get("name")}
    assert not moved, f"{len(moved)} of {len(want)} rows answer differently (now, pinned): {moved}"


def main():
    import route_cases as R
    assert os.environ.get("MI355_EMU_NOEXEC") == "1", "the refusal table only records launches: run with MI355_EMU_NOEXEC=1"
    _, be = R._backend()
    buf = ctypes.create_string_buffer(4096)

    def take():
        be.lib.emu_take_launches(buf, len(buf))
        return [k for k in buf.value.decode().split("\n") if k]
    print(json.dumps(rows(be, take)))


if __name__ == "__main__":
    main()
