"""Writes tests/golden/permutation_reference.json: the REFERENCE's 48 permutation keys and what its own permute_data returns.

    python tests/golden/make_permutation_reference.py          (needs the reference checkout: oracle/reference_shim.REFERENCE_ROOT)

The reference's unet3d/utils/augment.py is loaded from its file, untouched, as a module of a stub package: its sibling modules (affine,
image, resample, nilearn_custom_utils, utils) and monai / scipy.ndimage are empty stand-ins that only carry the names it imports -- the
permutation functions use none of them. Nothing of it is copied: the fixture holds data only.

  keys      generate_permutation_keys(), sorted
  cases     for each of them and for EXTRA_KEYS (the old 2-tuple rotation, the transpose flag): the key, the shape and the 120 values of
            permute_data(arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5), key), and whether reverse_permute_data gave the input back
"""
import importlib.util
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import reference_shim  # noqa: E402

SHAPE = (2, 3, 4, 5)
EXTRA_KEYS = [((1, 3), 1, 0, 1, 1), ((0, 1), 0, 1, 0, 1), ((2, 0), 0, 0, 0, 0), ((1, 2, 3), 1, 1, 0, 1)]
STUBS = {"monai": (), "monai.transforms": ("GaussianSmooth",), "scipy": (), "scipy.ndimage": (), "scipy.ndimage.interpolation": ("map_coordinates",),
         "scipy.ndimage.filters": ("gaussian_filter",),
         "refpkg": (), "refpkg.affine": ("get_extent_from_image", "get_spacing_from_affine", "assert_affine_is_diagonal"),
         "refpkg.image": ("get_image",), "refpkg.resample": ("resample", "resample_to_img"), "refpkg.nilearn_custom_utils": (),
         "refpkg.nilearn_custom_utils.nilearn_utils": ("get_background_values",), "refpkg.utils": ("copy_image",)}


def load_augment():
    saved = {n: sys.modules.get(n) for n in STUBS}
    for name, attrs in STUBS.items():
        mod = types.ModuleType(name)
        mod.__path__ = []
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    try:
        path = os.path.join(reference_shim.REFERENCE_ROOT, "unet3d", "utils", "augment.py")
        spec = importlib.util.spec_from_file_location("refpkg.augment", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod


def plain(key):
    return [[int(r) for r in key[0]]] + [int(v) for v in key[1:]]


def main():
    augment = load_augment()
    keys = sorted(augment.generate_permutation_keys())
    x = torch.arange(SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3]).reshape(SHAPE)
    cases = []
    for key in keys + EXTRA_KEYS:
        y = augment.permute_data(x, key)
        back = augment.reverse_permute_data(y, key)
        cases.append({"key": plain(key), "shape": list(y.shape), "values": [int(v) for v in y.reshape(-1).tolist()],
                      "reverse_gives_input": bool(torch.equal(back, x))})
    out = {"shape": list(SHAPE), "keys": [plain(k) for k in keys], "cases": cases}
    path = os.path.join(HERE, "permutation_reference.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    distinct = {tuple(c["values"]) + tuple(c["shape"]) for c in cases[:len(keys)]}
    print(path, os.path.getsize(path), "bytes;", len(keys), "keys,", len(distinct), "distinct results,",
          sum(1 for k in keys if tuple(k[0]) == (0, 0, 0)), "pure flips, all reversed:", all(c["reverse_gives_input"] for c in cases))


if __name__ == "__main__":
    main()
