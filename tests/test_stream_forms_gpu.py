"""Every kernel form of the streaming ops on an MI355X: the views of the form table of tests/stream_form_cases.py (the kernel choice is host
code that depends on the view only; tests/test_stream_forms_emu.py pins it) with their values against float64, the exhaustive storage
conversions -- what says the gfx950 conversion instructions and their C++ twins in tools/emu agree -- and single Adam steps. The criteria
and their derivation are in that module's docstring."""
import pytest

import stream_form_cases as S


@pytest.mark.gpu
@pytest.mark.parametrize("row", S.ROWS, ids=S.ROW_IDS)
def test_form(hip_backend, row):
    """The row's view on the device: the values meet the row's criterion."""
    row.run(hip_backend)


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", [(S.BF16, S.F32), (S.F16, S.F32), (S.F32, S.BF16), (S.F32, S.F16), (S.BF16, S.F16), (S.F16, S.BF16)],
                         ids=lambda d: S.tname(d))
def test_conversion_exhaustive(hip_backend, src, dst):
    S.conversion_case(hip_backend, src, dst)


@pytest.mark.gpu
@pytest.mark.parametrize("count", S.ADAM_COUNTS)
def test_adam_single_step(hip_backend, count):
    worst = 0.0
    for step in S.ADAM_STEPS:
        for wd in S.ADAM_DECAYS:
            for gs in S.ADAM_SCALES:
                worst = max(worst, S.adam_case(hip_backend, count, step, wd, gs))
    print(f"adam count={count}: worst parameter error / allowance {worst:.3f}")


@pytest.mark.gpu
def test_adam_tail_is_written(hip_backend):
    S.adam_tail_case(hip_backend)
