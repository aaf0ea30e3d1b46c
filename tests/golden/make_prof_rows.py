"""Writes tests/golden/prof_rows.json: the profile rows (family, flops, bytes, variant, fused bytes) that Backend.prof records for the
cases of tests/prof_rows_cases.py, run on the CPU emulator build of the kernel sources with a stub in place of torch.cuda.Event.

    python tests/golden/make_prof_rows.py

The fixture pins what the host code computes today: regenerate it only with a change that MEANS to change a row, from the commit before
that change, and say so in the commit message. It holds data only."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import prof_rows_cases as P  # noqa: E402


def main():
    os.environ.pop("MI355_PROF_SHAPES", None)
    subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)
    lib = importlib.import_module("3dunetcnn_amd._lib").bind(ctypes.CDLL(os.path.join(ROOT, "tools", "emu", "libmi355unet3d_emu.so")))
    be = importlib.import_module("3dunetcnn_amd.ops").Backend(lib=lib, device="cpu")
    torch.cuda.Event = P.StubEvent
    out = {name: P.compared(P.run_case(be, name)) for name in P.CASES}
    with open(P.FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]" for name, rows in out.items()) + "\n}\n")
    assert P.load_fixture() == out
    for name, rows in out.items():
        print(name, len(rows), "rows,", len({r[0] for r in rows}), "families")
    print(P.FIXTURE, os.path.getsize(P.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
