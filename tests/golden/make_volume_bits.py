"""Writes one section of tests/golden/volume_bits.json: the sha256 digests of tests/volume_bits_cases.py.

    python tests/golden/make_volume_bits.py emu      [--out FILE]    # the CPU emulator build of this tree's kernel sources
    python tests/golden/make_volume_bits.py gfx950   [--out FILE]    # the HIP library of this tree, on an MI355X

Run from a checkout of the commit whose behaviour is to be pinned (for the committed file: the parent of the commit that introduced
csrc/volume_common.h, with this script and tests/volume_bits_cases.py copied in), with the library built. The other section of an existing
file is kept. The file is never rewritten from a tree whose kernels are under test: see tests/volume_bits_cases.py.
"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def backend(section):
    ops = importlib.import_module("3dunetcnn_amd.ops")
    if section == "gfx950":
        import torch
        assert torch.cuda.is_available(), "the gfx950 section needs an MI355X"
        return ops.default_backend()
    subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)
    lib_mod = importlib.import_module("3dunetcnn_amd._lib")
    return ops.Backend(lib=lib_mod.bind(ctypes.CDLL(os.path.join(ROOT, "tools", "emu", "libmi355unet3d_emu.so"))), device="cpu")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("section", choices=("emu", "gfx950"))
    ap.add_argument("--out", default=os.path.join(HERE, "volume_bits.json"))
    a = ap.parse_args()
    import volume_bits_cases as B
    be = backend(a.section)
    got = {}
    for group in B.GROUPS:
        d = B.digests(be, group)
        assert not set(d) & set(got), group
        got.update(d)
        print(f"{a.section}: {group}: {len(d)} digests", flush=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc[a.section] = got
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(got)} digests to {a.out} [{a.section}]")


if __name__ == "__main__":
    main()
