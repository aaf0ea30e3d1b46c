"""TEST INFRASTRUCTURE: the launch geometry of the conv entry points on the CPU emulator under MI355_EMU_NOEXEC=1 (launches are recorded,
not run). Run as a child process by tests/test_conv_launch_geometry.py:

    MI355_EMU_NOEXEC=1 python tests/launch_geometry_cases.py   -> one JSON object {case id: [[kernel expression, "gx gy gz bx by bz lds"], ...]}

The cases: every launch of tests/route_cases.py (plain and with the moments epilogue), the fuse forms of both Winograd forward kernels at
the shape of tests/conv_bits_cases.py (12 input channels: the two kernels pad them differently, which their LDS sizes show), the Winograd
weight gradient and the fused first-layer backward. tests/golden/conv_launch_geometry.json holds the answers of the commit BEFORE the conv
sources were moved onto csrc/conv_internal.h (tests/golden/make_conv_launch_geometry.py)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_launch_geometry.json")
WINO_FUSE_FORMS = ("plain", "moments", "normalised input", "normalised input, moments", "norm-backward sums")


def collect():
    import refusal_cases as F
    import route_cases as R
    res = {}
    for cid, r in R.collect().items():
        res[cid] = list(zip(r["launched"], r["geometry"]))
        if "moments_launched" in r:
            res[cid + " moments"] = list(zip(r["moments_launched"], r["moments_geometry"]))
    _, be = R._backend()
    lib = be.lib
    buf = ctypes.create_string_buffer(4096)

    def take():
        out = []
        for f in (lib.emu_take_launches, lib.emu_take_geometry):
            f(buf, len(buf))
            out.append([k for k in buf.value.decode().split("\n") if k])
        return list(zip(*out))

    def launch(cid, c):
        take()
        value, _ = F.run(lib, c, None, None)
        assert value == 0, (cid, value)
        res[cid] = take()
        assert res[cid], cid

    for entry in ("wino_fwd", "wino3d_fwd"):
        for form in WINO_FUSE_FORMS:
            c = F.Call(lib, be.device, entry, shape=(2, 3, 9, 17, 12, 10))
            c.y.ld = 16
            if form.startswith("normalised input"):
                c.norm_input(0.01)
            if form.endswith("moments"):
                c.d.moments_out = c.rec
            if form == "norm-backward sums":
                c.gn_bwd(groups=5, gx_ld=16)
            launch(f"{entry} {form}", c)
    launch("wgrad_wino 32->32", F.Call(lib, be.device, "wgrad_wino", shape=(1, 4, 8, 16, 32, 32)))
    launch("c4_bwd 4->32", F.Call(lib, be.device, "c4_bwd", shape=(1, 4, 8, 16, 4, 32)))
    return res


if __name__ == "__main__":
    assert os.environ.get("MI355_EMU_NOEXEC") == "1", "launch geometry is recorded, not run: MI355_EMU_NOEXEC=1"
    print(json.dumps(collect()))
