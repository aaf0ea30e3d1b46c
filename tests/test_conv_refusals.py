"""The refusal table of the conv entry points (tests/refusal_cases.py) is the one tests/golden/conv_refusals.json pinned from the commit
before the conv sources were moved onto csrc/conv_internal.h: on the emulator every status, value, printed kernel name and recorded launch;
on an MI355X the status, value and name of every row that launched nothing there (refusal_cases.gpu_rows; a refused call launches nothing:
the twin runs in well under a second)."""
import json
import os
import subprocess
import sys

import pytest

import refusal_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusal_table_on_the_emulator(emu_backend):         # (emu_backend: the emulator library is built)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "refusal_cases.py")], env=dict(os.environ, MI355_EMU_NOEXEC="1"),
                         capture_output=True, text=True, timeout=600, check=True).stdout
    got, want = json.loads(out), json.load(open(F.GOLDEN))
    F.check_values(got, want)
    moved = {k: (got[k]["launched"], want[k]["launched"]) for k in want if got[k]["launched"] != want[k]["launched"]}
    assert not moved, f"{len(moved)} rows launch differently (now, pinned): {moved}"


@pytest.mark.gpu
def test_refusal_table_on_the_gpu(hip_backend):
    want = json.load(open(F.GOLDEN))
    only = F.gpu_rows(want)
    assert len(only) > 400
    F.check_values(F.rows(hip_backend, only=only), {k: want[k] for k in only})
