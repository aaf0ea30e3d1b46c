"""16-bit activation storage in HipDynUNet / HipDynUNetDS on the CPU emulator of the same kernel sources: the convolution forms only this
model family sends to the library (tests/dynunet_storage_cases.py), and the training step of the small deep-supervision network with
activations and their gradients stored as bf16 / fp16 next to the same step with fp32 tensors. GPU twins: tests/test_dynunet_storage_gpu.py
and tests/test_deep_supervision_gpu.py::test_bf16_activation_storage_tracks_the_fp32_storage_run."""
import pytest
import torch

import deep_supervision_cases as DS
import dynunet_storage_cases as DC
from oracle import unet3d_ref as R

dyn, losses = DS.dyn, DS.losses
SMALL, DHW = [8, 12, 16], (8, 12, 8)


@pytest.mark.parametrize("precision,storage", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
@pytest.mark.parametrize("cid", sorted(DC.CASES))
def test_conv_forms_round_once_on_store(emu_backend, cid, precision, storage):
    DC.run(emu_backend, cid, precision, storage)


def _step(be, precision, storage, side_stream=True):
    torch.manual_seed(5)
    m = dyn.HipDynUNetDS(**DS.kw(SMALL, 1)).train()
    crit = losses.HipDeepSupervisionLoss(losses.HipDiceLoss(sigmoid=True))
    DS.bind(be, m, crit)
    m.conv_precision, m.act_storage, m.backward_side_stream = precision, storage, side_stream
    x, y = R.synthetic_case(2, 4, DHW, 3)
    with DS.audited_heads(be) as seen:           # the head's dw, dbias and dx against float64 from the tensors this run hands it
        loss, grads = DS.train_step(m, crit, x, y)
    assert seen == [(storage or torch.float32, SMALL[1], 2)], seen
    assert be.act_dtype == torch.float32 and be.precision == 0          # the backend is left in its own mode
    return float(loss), grads


@pytest.mark.parametrize("precision,storage", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_16bit_storage_step_tracks_the_fp32_storage_step(emu_backend, precision, storage):
    """Losses within 2e-3 of each other (the bound tests/test_act_storage_gpu.py holds the losses of a network's 16-bit runs to), every
    gradient finite, and the storage type does change the arithmetic (the stored run is not the fp32-tensor run). The gradients' distance
    is printed as a record."""
    lop, gop = _step(emu_backend, precision, None)
    lst, gst = _step(emu_backend, precision, storage)
    print("record", dict(operands=lop, storage=lst))
    for k in gop:
        assert bool(torch.isfinite(gst[k]).all()), k
        print("record", k, float((gst[k] - gop[k]).abs().max()) / float(gop[k].abs().max()))
    assert lop != lst and abs(lop - lst) < 2e-3, (lop, lst)


def test_16bit_storage_without_the_side_stream(emu_backend):
    a = _step(emu_backend, "bf16", torch.bfloat16, side_stream=True)
    b = _step(emu_backend, "bf16", torch.bfloat16, side_stream=False)
    assert a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
