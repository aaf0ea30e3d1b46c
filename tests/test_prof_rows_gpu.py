"""GPU twin of tests/test_prof_rows.py: the same rows from the HIP library with real events. The rows come from host code, so the
emulator-sized bundles are all it needs."""
import math

import pytest
import torch

import prof_rows_cases as P


@pytest.mark.gpu
def test_prof_rows_match_the_fixture_with_real_events(hip_backend, monkeypatch):
    monkeypatch.delenv("MI355_PROF_SHAPES", raising=False)
    fx = P.load_fixture()
    for name in ("wino2d", "bf16"):
        rows = P.run_case(hip_backend, name)
        P.assert_rows_match(rows, fx[name])
        torch.cuda.synchronize()
        for r in rows:
            ms = r[3].elapsed_time(r[4])
            assert math.isfinite(ms) and ms >= 0, (name, r[0], ms)
