"""The slab reduction of the weight gradients in its two forms on the MI355X (cases: tests/wgrad_reduce_cases.py)."""
import pytest

import wgrad_reduce_cases as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_wgrad_reduce_forms_agree_gpu(hip_backend, name):
    W.case_fp32(hip_backend, name)


def test_wgrad_reduce_unaligned_dw_gpu(hip_backend):
    W.case_unaligned(hip_backend)


def test_wgrad_reduce_lp_tr_gpu(hip_backend):
    W.case_lp_tr(hip_backend)
