"""Writes tests/golden/conv_refusals.json (the table of tests/refusal_cases.py) or, with `geometry`, tests/golden/conv_launch_geometry.json
(tests/launch_geometry_cases.py): what the CPU emulator build of this tree's conv sources answers and launches under MI355_EMU_NOEXEC=1.

    python tests/golden/make_conv_refusals.py [refusals | geometry] [--out FILE]

Run from a checkout of the commit whose behaviour is to be pinned (for the committed files: the parent of the commit that introduced
csrc/conv_internal.h, with this script, the two case modules, tests/route_cases.py and the launch-geometry record of tools/emu copied in --
test infrastructure only, no source of that commit changed). Never rewritten from a tree whose sources are under test.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
PINS = {"refusals": ("refusal_cases.py", "conv_refusals.json"), "geometry": ("launch_geometry_cases.py", "conv_launch_geometry.json")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pin", nargs="?", default="refusals", choices=sorted(PINS))
    ap.add_argument("--out")
    a = ap.parse_args()
    script, name = PINS[a.pin]
    out = subprocess.run([sys.executable, os.path.join(TESTS, script)], env=dict(os.environ, MI355_EMU_NOEXEC="1"), capture_output=True,
                         text=True, check=True).stdout
    doc = json.loads(out)
    path = a.out or os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(doc)} rows to {path}")


if __name__ == "__main__":
    main()
