"""Writes tests/golden/normalize_reference.pt: small inputs and what the REFERENCE's own normalisers return for them.

    python tests/golden/make_normalize_reference.py            (needs the reference checkout: oracle/reference_shim.REFERENCE_ROOT)

The reference's unet3d/utils/normalize.py and unet3d/utils/threshold.py are loaded from their files, untouched, behind an empty stub of
`monai` (not installed; only histogram_normalize and nothing in threshold.py would use it). Nothing of them is copied: the fixture holds
data only -- inputs, outputs, and the parameters of the calls.

  percentile_window, percentile_threshold   on the FLOAT64 copies of the fp32 inputs: on float32 input numpy 2.x evaluates the rank
                                            position in float32, tens of fp32 ulps from the double rule this project follows
  foreground_zero_mean_normalize_image_data the single-channel branch, on the float64 copy
  static_windows, radiology_style_windowing on the fp32 input (every step is one fp32 operation: the bits are the expectation); the
                                            windows are integers, so level -/+ width / 2 is exact in fp32
zero_one_window and zero_floor_normalize_image_data are absent: as written they call torch.percentile, which does not exist.
"""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import reference_shim  # noqa: E402

WINDOW_PERCENTILES = [(5, 95), (1, 99)]
THRESHOLD_FRACTIONS = [0.9, 0.5]
WINDOWS = [(40, 80), (50, 350), (-600, 1500)]
RADIOLOGY_WINDOW = (40, 400)


def load(name):
    for n in ("monai", "monai.transforms", "monai.transforms.intensity", "monai.transforms.intensity.array", "monai.inferers"):
        if n not in sys.modules:
            sys.modules[n] = types.ModuleType(n)
    sys.modules["monai.transforms.intensity.array"].HistogramNormalize = None
    path = os.path.join(reference_shim.REFERENCE_ROOT, "unet3d", "utils", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    normalize, threshold = load("normalize"), load("threshold")
    g = torch.Generator().manual_seed(20)
    a = (torch.randn(3, 5, 6, 7, generator=g) * torch.tensor([100.0, 1.0, 1e-3]).view(3, 1, 1, 1) + torch.tensor([0.0, 1000.0, -5.0]).view(3, 1, 1, 1))
    b = torch.where(torch.rand(1, 9, 10, 11, generator=g) < 0.55, torch.zeros(()), torch.randn(1, 9, 10, 11, generator=g) * 50 + 300)
    ct = torch.randn(1, 9, 10, 11, generator=g) * 400
    out = {"a": a.float().contiguous(), "b": b.float().contiguous(), "ct": ct.float().contiguous(),
           "window_percentiles": WINDOW_PERCENTILES, "threshold_fractions": THRESHOLD_FRACTIONS, "windows": WINDOWS,
           "radiology_window": RADIOLOGY_WINDOW}
    for name in ("a", "b"):
        x64 = out[name].double()
        for lo, hi in WINDOW_PERCENTILES:
            out[f"percentile_window_{name}_{lo}_{hi}"] = normalize.percentile_window(x64, lo, hi)
        for fraction in THRESHOLD_FRACTIONS:
            out[f"percentile_threshold_{name}_{fraction}"] = threshold.percentile_threshold(x64, fraction)
    out["foreground_zero_mean_b"] = normalize.foreground_zero_mean_normalize_image_data(out["b"].double())
    out["static_windows_ct"] = normalize.static_windows(out["ct"], WINDOWS)
    out["radiology_ct"] = normalize.radiology_style_windowing(out["ct"][0], *RADIOLOGY_WINDOW)
    for k, v in out.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.contiguous().clone()
    path = os.path.join(HERE, "normalize_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")
    for fn in ("zero_one_window", "zero_floor_normalize_image_data"):
        try:
            getattr(normalize, fn)(out["a"])
        except AttributeError as e:
            print(f"{fn}: {e}")


if __name__ == "__main__":
    main()
