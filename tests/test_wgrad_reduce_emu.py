"""The slab reduction of the weight gradients in its two forms on the CPU emulator (cases: tests/wgrad_reduce_cases.py)."""
import pytest

import wgrad_reduce_cases as W


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_wgrad_reduce_forms_agree_emulator(emu_backend, name):
    W.case_fp32(emu_backend, name)


def test_wgrad_reduce_unaligned_dw_emulator(emu_backend):
    W.case_unaligned(emu_backend)


def test_wgrad_reduce_lp_tr_emulator(emu_backend):
    W.case_lp_tr(emu_backend)
