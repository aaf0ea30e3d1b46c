"""Every kernel form of the streaming ops on the CPU emulator of the same kernel sources: the form table of tests/stream_form_cases.py
(which kernel each view launches, read from the emulator's launch record, and its values against float64), the exhaustive storage
conversions, and single Adam steps. The criteria, their derivation and what each row reaches are in that module's docstring."""
import pytest

import stream_form_cases as S


def test_table_is_complete():
    S.check_table_is_complete()


def test_geometry_is_covered():
    S.check_geometry_is_covered()


@pytest.mark.parametrize("row", S.ROWS, ids=S.ROW_IDS)
def test_form(emu_backend, row):
    """The row's view launches exactly the row's kernel expressions, and the values meet the row's criterion."""
    row.run(emu_backend)


@pytest.mark.parametrize("src,dst", [(S.BF16, S.F32), (S.F16, S.F32), (S.F32, S.BF16), (S.F32, S.F16), (S.BF16, S.F16), (S.F16, S.BF16)],
                         ids=lambda d: S.tname(d))
def test_conversion_exhaustive(emu_backend, src, dst):
    S.conversion_case(emu_backend, src, dst)


@pytest.mark.parametrize("count", S.ADAM_COUNTS)
def test_adam_single_step(emu_backend, count):
    worst = 0.0
    for step in S.ADAM_STEPS:
        for wd in S.ADAM_DECAYS:
            for gs in S.ADAM_SCALES:
                worst = max(worst, S.adam_case(emu_backend, count, step, wd, gs))
    print(f"adam count={count}: worst parameter error / allowance {worst:.3f}")


def test_adam_tail_is_written(emu_backend):
    S.adam_tail_case(emu_backend)
