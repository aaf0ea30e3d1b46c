"""Writes one section of tests/golden/conv_bits.json: the sha256 digests of tests/conv_bits_cases.py.

    python tests/golden/make_conv_bits.py emu      [--out FILE]    # the CPU emulator build of this tree's kernel sources
    python tests/golden/make_conv_bits.py gfx950   [--out FILE]    # the HIP library of this tree, on an MI355X: two runs, two processes

Run from a checkout of the commit whose behaviour is to be pinned (for the committed file: the parent of the commit that introduced
csrc/conv_internal.h, with this script and tests/conv_bits_cases.py copied in), with the library built. The other section of an existing
file is kept. The gfx950 section is written from two runs in fresh processes: a case whose digests differ between them (a kernel that
accumulates in an order the hardware schedules) is not a pin; it goes to `gfx950_unstable` with both digests and the tests do not compare
it. The emu section leaves nothing out. The file is never rewritten from a tree whose kernels are under test.
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


def one_run(section):
    import conv_bits_cases as B
    be = backend(section)
    got = {}
    for group in B.GROUPS:
        d = B.digests(be, group)
        assert not set(d) & set(got), group
        got.update(d)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("section", choices=("emu", "gfx950"))
    ap.add_argument("--out", default=os.path.join(HERE, "conv_bits.json"))
    ap.add_argument("--print-digests", action="store_true", help="one run in this process, digests as JSON on stdout (the child of a gfx950 run)")
    a = ap.parse_args()
    if a.print_digests:
        print(json.dumps(one_run(a.section)))
        return
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.section == "emu":
        doc["emu"] = one_run("emu")
    else:
        runs = [json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "gfx950", "--print-digests"], capture_output=True,
                                          text=True, check=True, timeout=240).stdout.strip().splitlines()[-1]) for _ in range(2)]
        assert set(runs[0]) == set(runs[1])
        doc["gfx950"] = {k: v for k, v in runs[0].items() if runs[1][k] == v}
        doc["gfx950_unstable"] = {k: [runs[0][k], runs[1][k]] for k in runs[0] if runs[1][k] != runs[0][k]}
        for k, v in doc["gfx950_unstable"].items():
            print(f"gfx950: {k} differs between two runs of this tree: {v[0]} / {v[1]}")
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(doc[a.section])} digests to {a.out} [{a.section}]")


if __name__ == "__main__":
    main()
