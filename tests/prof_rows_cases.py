"""The profile rows (Backend.prof) of one training step per routing, shared by tests/test_prof_rows.py (CPU emulator, stub events),
tests/test_prof_rows_gpu.py (HIP library, real events) and tests/golden/make_prof_rows.py, which writes the expectation
tests/golden/prof_rows.json. bench.py builds its roofline block, its per-instantiation rows and the PMC look-up from these rows; they
are host arithmetic over shapes plus the kernel names the library's plans answer, so one fixture serves both libraries.

A case = one forward + Dice loss + backward of a committed golden bundle (20 x 16 x 24 volumes) under a routing, or one direct
Backend.c4_bwd call (no bundle is wide enough to reach the fused first-layer backward). Of a row (family, flops, bytes, e0, e1,
variant, fused bytes) everything but the two events is compared, exactly: strings and Python floats."""
import importlib
import json
import os

import torch

import op_cases as C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "prof_rows.json")
COMPARED = (0, 1, 2, 5, 6)            # family, flops, bytes, variant, fused bytes

WINO = dict(winograd=True, wgrad_form="wino", WINO_MIN_VOXELS=0)       # the bundles are 20 x 16 x 24: route every level
# name -> (bundle, network: None = HipUNet3D | (autocast_dtype, activation_storage) = HipAutocastUNet, backend attributes)
CASES = {
    "wino2d": ("unet3d_small.pt", None, dict(WINO, wino_form="2d")),               # Winograd forward, dgrad and weight-gradient rows
    "wino3d": ("unet3d_small.pt", None, dict(WINO, wino_form="3d")),
    "direct": ("unet3d_small.pt", None, dict(winograd=False, wgrad_form="direct")),   # conv3d_mfma<...>, conv3d_wgrad_ring, first layer, stride 2, 1x1x1
    "bf16": ("unet3d_small_autocast.pt", ("bf16", "bf16"), {}),                    # conv3d_k3_bf16<...> variants, element-size bytes
    # zero-insert flops / 8, windowed out_dhw, bias; the product routing (the 20 x 16 x 24 level is above the Winograd threshold)
    "transposed": ("unet3d_small_transposed.pt", None, dict(winograd=True, wino_form="auto", wgrad_form="wino")),
    "c4_bwd": (None, None, {}),
}
C4_BWD_CASE = dict(n=1, dhw=(2, 3, 5), xld=8, dyld=64)      # the smallest first-layer case of tests/test_ops_emu.py


class StubEvent:
    """Stands in for torch.cuda.Event where there is no device: accepts enable_timing, records nothing."""
    def __init__(self, enable_timing=False):
        self.enable_timing = enable_timing

    def record(self, stream=None):
        pass


def run_case(be, name):
    """The rows `be` records for case `name`; the backend's attributes are restored."""
    bundle, net, attrs = CASES[name]
    unet = importlib.import_module("3dunetcnn_amd.unet")
    losses = importlib.import_module("3dunetcnn_amd.losses")
    saved = {k: getattr(be, k) for k in attrs if k != "WINO_MIN_VOXELS"}
    saved.update(precision=be.precision, act_dtype=be.act_dtype)
    for k, v in attrs.items():
        setattr(be, k, v)
    be.prof = rows = []
    try:
        if bundle is None:
            C.case_c4_bwd(be, **C4_BWD_CASE)
            return rows
        g = torch.load(os.path.join(GOLD, bundle))
        if "bundle" in g:                                    # the autocast record names the bundle it was generated from
            g = torch.load(os.path.join(GOLD, g["bundle"]))
        m = unet.HipUNet3D(**g["kwargs"]) if net is None else unet.HipAutocastUNet(autocast_dtype=net[0], activation_storage=net[1], **g["kwargs"])
        m = m.to(be.device).eval()
        m._be = be
        m.load_state_dict(g["state_dict"])
        crit = losses.HipDiceLoss(sigmoid=True)
        crit._be = be
        crit(m(g["x"].to(be.device)), g["y"].to(be.device)).backward()
        return rows
    finally:
        be.prof = None
        if "WINO_MIN_VOXELS" in attrs:
            del be.WINO_MIN_VOXELS
        for k, v in saved.items():
            setattr(be, k, v)


def compared(rows):
    return [[r[i] for i in COMPARED] for r in rows]


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def assert_rows_match(rows, want):
    """Exact equality, type included (a float that became an int would still compare equal)."""
    got = compared(rows)
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert [(type(v), v) for v in a] == [(type(v), v) for v in b], (i, a, b)
