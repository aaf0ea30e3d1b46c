"""Every conv launch of tests/launch_geometry_cases.py has the kernel, grid, block and dynamic LDS bytes that
tests/golden/conv_launch_geometry.json pinned from the commit before the conv sources were moved onto csrc/conv_internal.h."""
import json
import os
import subprocess
import sys

import launch_geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_geometry(emu_backend):         # (emu_backend: the emulator library is built)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_geometry_cases.py")], env=dict(os.environ, MI355_EMU_NOEXEC="1"),
                         capture_output=True, text=True, timeout=600, check=True).stdout
    got, want = {k: [list(l) for l in v] for k, v in json.loads(out).items()}, json.load(open(G.GOLDEN))
    assert set(got) == set(want), f"cases that left: {sorted(set(want) - set(got))}; not in the fixture: {sorted(set(got) - set(want))}"
    moved = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not moved, f"{len(moved)} of {len(want)} cases launch differently (now, pinned): {moved}"
