"""Every route of mi355_conv3d_fwd and mi355_conv3d_wgrad on the CPU emulator (launches recorded, not run: tests/route_cases.py): the kernel
the config query names is the kernel the entry point launches, and the statistics-block / workspace queries agree with what the launch
accepts."""
import json
import os
import subprocess
import sys

import pytest

import route_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUPPORTED, EWORKSPACE = -2, -4


@pytest.fixture(scope="module")
def routes(emu_backend):         # (emu_backend: the emulator library is built)
    env = dict(os.environ, MI355_EMU_NOEXEC="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "route_cases.py")], env=env, capture_output=True, text=True,
                         timeout=600, check=True).stdout
    return json.loads(out)


def base(kernel):
    """'(conv3d_mfma<KD, STRIDE, ...>)' (a LAUNCH expression) or 'conv3d_mfma<3, 1, ...>' (a config query) -> 'conv3d_mfma'"""
    return kernel.strip("() ").split("<")[0]


def mfma_flags(kernel):
    """(in_mode, tl, fullj) of a conv3d_mfma name or LAUNCH expression (the launch writes tl = true as 'KD == 3')."""
    args = [a.strip() for a in kernel.strip("() ").split("<", 1)[1].rstrip(">").split(",")]
    return args[11], "true" if args[12] in ("true", "KD == 3") else args[12], args[13]


FWD_KERNEL = {"c4": "conv3d_c4_fwd", "c4_bf16": "conv3d_c4_fwd_bf16", "narrow": "conv3d_c4_dgrad", "lp_tile": "conv3d_k3_bf16",
              "lp_tile_wide": "conv3d_k3_bf16", "lp_zring": "conv3d_k3_lp_zring", "lp_zring2": "conv3d_k3_lp_zring2",
              "s2c32_fwd": "conv3d_s2c32_fwd", "s2c32_dgrad": "conv3d_s2c32_dgrad", "k1_stream": "conv3d_k1_stream_bf16"}
# template arguments (KD .. NT) of the generic kernel's configuration rows (csrc/conv3d_fwd.hip: kMfmaCfg)
MFMA_ARGS = {0: "1, 1, 1, 1, 256, 32, 4, 4, 1, 2, 2", 1: "1, 1, 1, 1, 256, 32, 4, 4, 1, 2, 1", 2: "3, 2, 4, 4, 8, 8, 0, 4, 1, 1, 2",
             3: "3, 2, 4, 4, 8, 8, 0, 4, 1, 1, 1", 4: "3, 1, 4, 8, 8, 16, 4, 4, 1, 2, 2", 5: "3, 1, 4, 8, 8, 16, 4, 4, 1, 2, 1",
             6: "3, 1, 2, 4, 8, 32, 4, 2, 2, 1, 1", 7: "3, 1, 4, 4, 8, 32, 4, 4, 1, 1, 1", 8: "3, 1, 4, 4, 8, 16, 4, 2, 2, 2, 1"}


@pytest.mark.parametrize("case", sorted(R.FWD))
def test_fwd_route(routes, case):
    r = routes["fwd:" + case]
    assert r["config_rc"] == 0 and r["rc"] == 0, r
    assert r["launched"] and base(r["launched"][0]) == base(r["config"]), r
    if case.startswith("mfma_cfg"):
        cfg = int(case[len("mfma_cfg")])
        assert r["config"].startswith(f"conv3d_mfma<{MFMA_ARGS[cfg]}, "), r["config"]
        assert mfma_flags(r["config"]) == mfma_flags(r["launched"][0]), r
    else:
        assert base(r["config"]) == FWD_KERNEL[case]
    # statistics: a call the query gives records to launches with the moments epilogue (on the kernel the config query then names);
    # a call it gives none refuses the epilogue
    if r["stats_blocks"] > 0:
        assert r["moments_rc"] == 0 and base(r["moments_launched"][0]) == base(r["config_moments"]), r
        if r["config_moments"].startswith("conv3d_mfma<"):
            assert mfma_flags(r["config_moments"]) == mfma_flags(r["moments_launched"][0]), r
    else:
        assert r["moments_rc"] == EUNSUPPORTED and not r["moments_launched"], r


WGRAD_KERNEL = {"c4": "conv3d_c4_wgrad", "lp_tr": "conv3d_wgrad_lp_tr", "k1_f32": "conv3d_wgrad_k1_stream", "k1_bf16": "conv3d_wgrad_k1_stream",
                "k3_bf16": "conv3d_wgrad_k3_bf16", "s2c32": "conv3d_s2c32_wgrad", "ring": "conv3d_wgrad_ring",
                "mfma_k1": "conv3d_wgrad_mfma<1, 1>", "mfma_s2": "conv3d_wgrad_mfma<3, 2>", "mfma_d2s": "conv3d_wgrad_mfma<1, 1>"}


@pytest.mark.parametrize("case", sorted(R.WGRAD))
def test_wgrad_route(routes, case):
    r = routes["wgrad:" + case]
    assert r["config_rc"] == 0 and r["config"] == WGRAD_KERNEL[case], r
    # the workspace the query asks for is what the launch needs: enough, and one byte less is refused before anything launches
    assert r["workspace"] > 0 and r["rc"] == 0, r
    assert r["launched"] and base(r["launched"][0]) == base(r["config"]), r
    assert r["short_ws_rc"] == EWORKSPACE and not r["short_ws_launched"], r


def test_wgrad_refused_call_has_no_workspace_and_no_name(emu_backend):
    """Mixed storage types on the 3x3x3 stride-2 form: the launch refuses them, so the queries answer 0 / unsupported (the workspace
    query used to answer a size for them)."""
    import ctypes
    import importlib
    import torch
    ops = importlib.import_module("3dunetcnn_amd.ops")
    be = emu_backend
    x, dy = be.empty_act(1, 8, 8, 8, 16), be.empty_act(1, 4, 4, 4, 32, dtype=torch.bfloat16)
    d = be._desc(3, 2, 1, ops.IN_PLAIN, 0.0, None, None, None, None, None, (0, 0, 0), (4, 4, 4), [])
    xd, dyd = x.desc(), dy.desc()
    name = ctypes.create_string_buffer(96)
    assert be.lib.mi355_conv3d_wgrad_workspace(ctypes.byref(xd), ctypes.byref(dyd), ctypes.byref(d)) == 0
    assert be.lib.mi355_conv3d_wgrad_config(ctypes.byref(xd), ctypes.byref(dyd), ctypes.byref(d), name, 96) == EUNSUPPORTED
