"""GPU twins of tests/test_dynunet_storage.py: the 16-bit-storage convolution forms of HipDynUNet on the MI355X (the HIP library through the
C ABI). The cases and their criterion: tests/dynunet_storage_cases.py."""
import pytest
import torch

import dynunet_storage_cases as DC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision,storage", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
@pytest.mark.parametrize("cid", sorted(DC.CASES))
def test_conv_forms_round_once_on_store(hip_backend, cid, precision, storage):
    DC.run(hip_backend, cid, precision, storage)
