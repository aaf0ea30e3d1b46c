"""GPU twins of tests/test_deep_supervision.py: the two head kernels on the MI355X against float64, HipDynUNetDS against the plain-torch
restatement at the BraTS head widths, a training step replayed as one HIP graph. Cases and criteria: tests/deep_supervision_cases.py."""
import importlib

import pytest
import torch

import deep_supervision_cases as DS
import scratch_guard as G
from oracle import unet3d_ref as R

pytestmark = pytest.mark.gpu
dyn, losses, optim = DS.dyn, DS.losses, DS.optim
graph = importlib.import_module("3dunetcnn_amd.graph")


@pytest.mark.parametrize("cid", sorted(DS.CASES))
def test_head_ops_against_float64(hip_backend, cid):
    DS.head_case(hip_backend, *DS.CASES[cid])


@pytest.mark.parametrize("rid", sorted(DS.REFUSALS))
def test_head_ops_refuse(hip_backend, rid):
    assert DS.refusal(hip_backend, *DS.REFUSALS[rid]) == (DS.EINVAL, DS.EINVAL)


def test_head_ops_on_hostile_memory(hip_backend):
    for cid in ("bf16-c100-k3-f2", "f32-c320-k3-f16"):
        assert G.hold(hip_backend, lambda: DS.head_case(hip_backend, *DS.CASES[cid]), (G.QNAN, G.ONES)).results > 0


def test_head_ops_abi_contract(hip_backend):
    DS.abi_contract(hip_backend)


def _step_case(be):
    torch.manual_seed(7)
    m = dyn.HipDynUNetDS(**DS.kw([8, 12, 16], 1)).cuda().train()
    crit = losses.HipDeepSupervisionLoss(losses.HipDiceLoss(sigmoid=True))
    DS.bind(be, m, crit)
    x, y = (t.cuda() for t in R.synthetic_case(1, 4, (4, 8, 4), 3))
    out = m(x)
    loss = crit(out, y)
    loss.backward()
    return [out.detach(), loss.detach().reshape(1)] + [p.grad for p in m.parameters()]


def test_training_step_on_hostile_memory(hip_backend):
    assert G.hold(hip_backend, lambda: _step_case(hip_backend), (G.QNAN, G.ONES)).results > 0


# Recorded on MI355X (`pytest -s` prints the dictionaries; no assertion on n_loose / max_err_vs_fp32, they describe the conditioning of the
# problem as in tests/test_dynunet.py):
#   narrow       ([16, 32, 48, 64] 32^3 batch 2 K = 2): logits 3.5e-6, loss 7e-8, grad 0.008, n_loose 0, max_err_vs_fp32 1.6e-4
#   brats-widths ([64, 96, 128, 192] 32^3 batch 1 K = 2): logits 2.8e-6, loss 0,   grad 0.090, n_loose 0, max_err_vs_fp32 4.1e-4
NETWORK = {"narrow": ([16, 32, 48, 64], (32, 32, 32), 2, 2), "brats-widths": ([64, 96, 128, 192], (32, 32, 32), 1, 2)}


@pytest.mark.parametrize("name", sorted(NETWORK))
def test_network_fwd_bwd(name):
    """Heads on 96 and 128 channels ("brats-widths") are the widths of the BraTS configuration's first two supervised levels."""
    filters, dhw, n, K = NETWORK[name]
    torch.manual_seed(1234)
    m = dyn.HipDynUNetDS(**DS.kw(filters, K)).cuda().train()
    e = DS.pair(m, None, dhw, n, "cuda")
    print("record", name, {k: e[k] for k in ("n_loose", "max_err_vs_fp32")}, e)
    assert e["logits"] < DS.TOL and e["loss"] < DS.TOL and e["grad"] <= 1.0, e


def test_bf16_activation_storage_tracks_the_fp32_storage_run(hip_backend):
    """The "narrow" case with 16-bit operands, activations stored as bf16 next to the same step with fp32 tensors: losses within 2e-3 of
    each other (the bound tests/test_act_storage_gpu.py holds a network's storage runs to). The convolution forms the model needs for this
    are held to their own criterion in tests/test_dynunet_storage_gpu.py, and both heads' backward launches of both runs to the op-level
    one on the tensors the network hands them (DS.audited_heads): dw, dbias and the sum left in the level's gradient."""
    x, y = (t.cuda() for t in R.synthetic_case(2, 4, (32, 32, 32), 3))
    got = {}
    for storage in (None, torch.bfloat16):
        torch.manual_seed(1234)
        m = dyn.HipDynUNetDS(**DS.kw([16, 32, 48, 64], 2)).cuda().train()
        m.conv_precision, m.act_storage = "bf16", storage
        crit = losses.HipDeepSupervisionLoss(losses.HipDiceLoss(sigmoid=True))
        DS.bind(hip_backend, m, crit)
        with DS.audited_heads(hip_backend) as seen:
            loss, grads = DS.train_step(m, crit, x, y)
        assert sorted(seen) == [(storage or torch.float32, 32, 2), (storage or torch.float32, 48, 4)], seen
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        got[storage] = float(loss)
    print("record", got)
    assert abs(got[None] - got[torch.bfloat16]) < 2e-3, got


def _build():
    torch.manual_seed(3)
    m = dyn.HipDynUNetDS(**DS.kw([16, 32, 48], 1)).cuda().train()
    return m, losses.HipDeepSupervisionLoss(losses.HipDiceLoss(sigmoid=True)), optim.HipAdam(m.parameters(), lr=1e-3)


def test_graphed_step_equals_eager_step(hip_backend):
    """Two replays of the captured step (forward with its head, the deep-supervision loss, backward) equal two eager steps, bit for bit."""
    batches = [tuple(t.cuda() for t in R.synthetic_case(1, 4, (16, 16, 16), 3, seed=s)) for s in range(2)]
    m0, crit0, opt0 = _build()
    want = [float(DS.train_step(m0, crit0, x, y, opt0)[0]) for x, y in batches]
    m1, crit1, opt1 = _build()
    step = graph.HipGraphedTrainStep(m1, crit1, opt1, *batches[0])
    got = [float(step(x, y).item()) for x, y in batches]
    assert got == want, (got, want)
    assert tuple(step.logits.shape) == (1, 2, 3, 16, 16, 16)
    for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert torch.equal(a, b), k
