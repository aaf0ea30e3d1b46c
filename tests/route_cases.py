"""Routing cases of the conv entry points on the CPU emulator with MI355_EMU_NOEXEC=1 (launches are recorded, not run: the shapes
that select the large-volume routes cost nothing). Run as a child process by tests/test_routing_emu.py:

    MI355_EMU_NOEXEC=1 python tests/route_cases.py   -> one JSON object {case id: result}

For every case: the kernel the config query names, the kernels the launch recorded (tools/emu: emu_take_launches) with their grid, block
and dynamic LDS bytes (emu_take_geometry), the launch's status, and what the workspace / statistics-block query answered together with
the status of a launch that relies on that answer."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, BF16 = "fp32", "bf16"

# forward: id -> (x (n, d, h, w, c, storage), y (n, d, h, w, c, storage), kd, stride, pad, in_mode, precision, wformat, env)
FWD = {
    "c4": ((1, 8, 8, 8, 4, F32), (1, 8, 8, 8, 32, F32), 3, 1, 1, "PLAIN", "fp32", "OIDHW4", {}),
    "c4_bf16": ((1, 8, 8, 8, 4, F32), (1, 8, 8, 8, 32, BF16), 3, 1, 1, "AFFINE_ACT", "bf16", "OIDHW4", {}),
    "narrow": ((1, 4, 8, 8, 32, F32), (1, 4, 8, 8, 4, F32), 3, 1, 1, "PLAIN", "fp32", "PACKED", {}),
    "lp_tile": ((1, 4, 8, 16, 32, BF16), (1, 4, 8, 16, 64, BF16), 3, 1, 1, "AFFINE_ACT", "bf16", "PACKED", {"MI355_BF16_FORM": "tile"}),
    "lp_tile_wide": ((2, 32, 32, 64, 32, BF16), (2, 32, 32, 64, 128, BF16), 3, 1, 1, "PLAIN", "bf16", "PACKED", {"MI355_BF16_FORM": "tile"}),
    "lp_zring": ((1, 5, 8, 16, 32, BF16), (1, 5, 8, 16, 32, BF16), 3, 1, 1, "AFFINE_ACT", "bf16", "PACKED", {"MI355_BF16_FORM": "zring1"}),
    "lp_zring2": ((1, 9, 8, 16, 64, BF16), (1, 9, 8, 16, 64, BF16), 3, 1, 1, "AFFINE_ACT", "bf16", "PACKED", {"MI355_BF16_FORM": "zring"}),
    "s2c32_fwd": ((1, 9, 10, 12, 32, F32), (1, 5, 5, 6, 32, F32), 3, 2, 1, "PLAIN", "fp32", "PACKED", {}),
    "s2c32_dgrad": ((1, 4, 4, 5, 32, F32), (1, 8, 7, 9, 32, F32), 3, 1, 1, "ZERO_INSERT", "fp32", "PACKED", {}),
    "k1_stream": ((1, 4, 8, 8, 32, BF16), (1, 4, 8, 8, 64, BF16), 1, 1, 0, "PLAIN", "bf16", "PACKED", {}),
    "mfma_cfg0": ((1, 4, 8, 8, 16, F32), (1, 4, 8, 8, 64, F32), 1, 1, 0, "PLAIN", "fp32", "PACKED", {}),
    "mfma_cfg1": ((1, 4, 8, 8, 16, F32), (1, 4, 8, 8, 32, F32), 1, 1, 0, "AFFINE_ACT", "fp32", "PACKED", {}),
    "mfma_cfg2": ((1, 8, 8, 8, 32, F32), (1, 4, 4, 4, 64, F32), 3, 2, 1, "PLAIN", "fp32", "PACKED", {}),
    "mfma_cfg3": ((1, 8, 8, 8, 16, F32), (1, 4, 4, 4, 32, F32), 3, 2, 1, "AFFINE_ACT", "fp32", "PACKED", {}),
    "mfma_cfg4": ((1, 4, 4, 4, 16, F32), (1, 8, 8, 8, 64, F32), 3, 1, 1, "ZERO_INSERT", "fp32", "PACKED", {}),
    "mfma_cfg5": ((1, 4, 4, 4, 64, F32), (1, 8, 8, 8, 32, F32), 3, 1, 1, "ZERO_INSERT", "fp32", "PACKED", {}),
    "mfma_cfg4_big": ((2, 32, 64, 32, 64, F32), (2, 32, 64, 32, 64, F32), 3, 1, 1, "AFFINE_ACT", "fp32", "PACKED", {}),
    "mfma_cfg6": ((1, 8, 8, 8, 64, F32), (1, 8, 8, 8, 64, F32), 3, 1, 1, "AFFINE_ACT", "fp32", "PACKED", {}),
    "mfma_cfg7": ((1, 8, 8, 8, 16, F32), (1, 8, 8, 8, 32, F32), 3, 1, 1, "PLAIN", "fp32", "PACKED", {}),
    "mfma_cfg8": ((1, 32, 32, 32, 32, F32), (1, 32, 32, 32, 64, F32), 3, 1, 1, "PLAIN", "fp32", "PACKED", {}),
}
# weight gradient: id -> (x, dy, kd, stride, pad, in_mode, precision, out_mode)
WGRAD = {
    "c4": ((1, 8, 8, 8, 4, F32), (1, 8, 8, 8, 32, BF16), 3, 1, 1, "AFFINE_ACT", "bf16", "PLAIN"),
    "lp_tr": ((1, 8, 8, 16, 32, BF16), (1, 8, 8, 16, 64, BF16), 3, 1, 1, "AFFINE_ACT", "bf16", "PLAIN"),
    "k1_f32": ((1, 4, 8, 8, 32, F32), (1, 4, 8, 8, 64, F32), 1, 1, 0, "PLAIN", "fp32", "PLAIN"),
    "k1_bf16": ((1, 4, 8, 8, 64, BF16), (1, 4, 8, 8, 32, BF16), 1, 1, 0, "PLAIN", "bf16", "PLAIN"),
    "k3_bf16": ((1, 4, 8, 16, 32, F32), (1, 4, 8, 16, 32, F32), 3, 1, 1, "AFFINE_ACT", "bf16", "PLAIN"),
    "s2c32": ((1, 9, 8, 12, 32, F32), (1, 5, 4, 6, 32, F32), 3, 2, 1, "PLAIN", "fp32", "PLAIN"),
    "ring": ((1, 6, 8, 8, 16, F32), (1, 6, 8, 8, 16, F32), 3, 1, 1, "AFFINE_ACT", "fp32", "PLAIN"),
    "mfma_k1": ((1, 4, 8, 8, 16, F32), (1, 4, 8, 8, 24, F32), 1, 1, 0, "AFFINE_ACT", "fp32", "PLAIN"),
    "mfma_s2": ((1, 8, 8, 8, 16, F32), (1, 4, 4, 4, 32, F32), 3, 2, 1, "PLAIN", "fp32", "PLAIN"),
    "mfma_d2s": ((1, 4, 4, 4, 16, F32), (1, 8, 8, 8, 8, F32), 1, 1, 0, "PLAIN", "fp32", "D2S"),
}


def _backend():
    so = os.path.join(ROOT, "tools", "emu", "libmi355unet3d_emu.so")
    subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lib_mod = importlib.import_module("3dunetcnn_amd._lib")
    ops = importlib.import_module("3dunetcnn_amd.ops")
    cdll = ctypes.CDLL(so)
    for take in (cdll.emu_take_launches, cdll.emu_take_geometry):
        take.restype, take.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]
    return ops, ops.Backend(lib=lib_mod.bind(cdll), device="cpu")


def collect():
    """{case id: result} of every case of FWD and WGRAD."""
    import torch
    assert os.environ.get("MI355_EMU_NOEXEC") == "1", "route cases only record launches: run with MI355_EMU_NOEXEC=1"
    ops, be = _backend()
    lib = be.lib
    buf = ctypes.create_string_buffer(4096)

    def take():
        lib.emu_take_launches(buf, len(buf))
        return [k for k in buf.value.decode().split("\n") if k]

    def geometry():
        lib.emu_take_geometry(buf, len(buf))
        return [k for k in buf.value.decode().split("\n") if k]

    def act(spec):
        n, d, h, w, c, st = spec
        return be.empty_act(n, d, h, w, c, dtype=torch.float32 if st == F32 else torch.bfloat16)

    def desc(kd, stride, pad, in_mode, precision, out_mode, out_dhw, keep):
        be.set_precision(precision)
        scale = shift = None
        if in_mode == "AFFINE_ACT":
            scale, shift = torch.ones(64, 256), torch.zeros(64, 256)
        return be._desc(kd, stride, pad, getattr(ops, "IN_" + in_mode), 0.0, scale, shift, None, None, None, (0, 0, 0), out_dhw, keep,
                        None, getattr(ops, "OUT_" + out_mode))

    w = torch.zeros(1 << 20)               # any weights: nothing runs
    res = {}
    for cid, (xs, ys, kd, stride, pad, im, prec, wf, env) in FWD.items():
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            x, y, keep = act(xs), act(ys), []
            d = desc(kd, stride, pad, im, prec, "PLAIN", ys[1:4], keep)
            d.wformat = getattr(ops, "W_" + wf)
            xd, yd = x.desc(), y.desc()
            r = {"config_rc": lib.mi355_conv3d_fwd_config(ctypes.byref(xd), ctypes.byref(yd), ctypes.byref(d), buf, 96)}
            r["config"] = buf.value.decode()
            take(), geometry()
            r["rc"] = lib.mi355_conv3d_fwd(ctypes.byref(xd), w.data_ptr(), ctypes.byref(yd), ctypes.byref(d), None)
            r["launched"], r["geometry"] = take(), geometry()
            # the statistics query, and a launch with the moments epilogue it allows or refuses
            r["stats_blocks"] = lib.mi355_conv3d_stats_blocks(ctypes.byref(xd), ctypes.byref(yd), ctypes.byref(d))
            rec = torch.zeros(max(r["stats_blocks"], 1) * ys[0] * ys[4] * 3)
            d.moments_out = rec.data_ptr()
            r["config_moments_rc"] = lib.mi355_conv3d_fwd_config(ctypes.byref(xd), ctypes.byref(yd), ctypes.byref(d), buf, 96)
            r["config_moments"] = buf.value.decode()
            r["moments_rc"] = lib.mi355_conv3d_fwd(ctypes.byref(xd), w.data_ptr(), ctypes.byref(yd), ctypes.byref(d), None)
            r["moments_launched"], r["moments_geometry"] = take(), geometry()
            res["fwd:" + cid] = r
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    for cid, (xs, dys, kd, stride, pad, im, prec, om) in WGRAD.items():
        x, dy, keep = act(xs), act(dys), []
        d = desc(kd, stride, pad, im, prec, om, xs[1:4] if om == "D2S" else dys[1:4], keep)
        xd, dyd = x.desc(), dy.desc()
        r = {"config_rc": lib.mi355_conv3d_wgrad_config(ctypes.byref(xd), ctypes.byref(dyd), ctypes.byref(d), buf, 96)}
        r["config"] = buf.value.decode()
        r["workspace"] = nbytes = lib.mi355_conv3d_wgrad_workspace(ctypes.byref(xd), ctypes.byref(dyd), ctypes.byref(d))
        ws, dw = torch.zeros(max(nbytes // 4, 1)), torch.zeros(1 << 20)
        take(), geometry()
        r["rc"] = lib.mi355_conv3d_wgrad(ctypes.byref(xd), ctypes.byref(dyd), dw.data_ptr(), ctypes.byref(d), ws.data_ptr(), nbytes, None)
        r["launched"], r["geometry"] = take(), geometry()
        r["short_ws_rc"] = lib.mi355_conv3d_wgrad(ctypes.byref(xd), ctypes.byref(dyd), dw.data_ptr(), ctypes.byref(d), ws.data_ptr(),
                                                  nbytes - 1, None)
        r["short_ws_launched"] = take()
        res["wgrad:" + cid] = r
    be.set_precision("fp32")
    return res


def main():
    print(json.dumps(collect()))


if __name__ == "__main__":
    main()
