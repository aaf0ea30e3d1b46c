"""GPU twins of tests/test_res_block.py: the residual-block kernels on the MI355X against float64, HipDynUNet / HipDynUNetDS with
res_block=True against the plain-torch restatement, training steps against torch's Adam, a step replayed as one HIP graph and bf16
activation storage. Cases and criteria: tests/res_block_cases.py."""
import importlib

import pytest
import torch

import deep_supervision_cases as DS
import res_block_cases as RB
import scratch_guard as G
from oracle import torch_ops as O, unet3d_ref as R

pytestmark = pytest.mark.gpu
dyn, losses, optim = RB.dyn, RB.losses, RB.optim
graph = importlib.import_module("3dunetcnn_amd.graph")


@pytest.mark.parametrize("cid", sorted(RB.JOIN))
def test_join_against_float64(hip_backend, cid):
    RB.join_case(hip_backend, *RB.JOIN[cid])


@pytest.mark.parametrize("cid", sorted(RB.SHORTCUT))
def test_shortcut_conv_against_float64(hip_backend, cid):
    RB.shortcut_case(hip_backend, *RB.SHORTCUT[cid])


def test_ops_refuse(hip_backend):
    RB.refusals(hip_backend)


def test_ops_on_hostile_memory(hip_backend):
    for case in (lambda: RB.join_case(hip_backend, *RB.JOIN["bf16-c100-v33"]), lambda: RB.shortcut_case(hip_backend, *RB.SHORTCUT["f32-12-16-v1"])):
        assert G.hold(hip_backend, case, (G.QNAN, G.ONES)).results > 0


def test_training_step_on_hostile_memory(hip_backend):
    assert G.hold(hip_backend, lambda: RB.step_case(hip_backend, "cuda"), (G.QNAN, G.ONES)).results > 0


# Recorded on MI355X (`pytest -s` prints the dictionaries; no assertion on n_loose / max_err_vs_fp32, they describe the conditioning of the
# problem as in tests/test_dynunet.py):
#   three        ([32, 64, 96] (16, 24, 32) batch 2):        logits 1.7e-6, loss 0,    grad 0.0008, n_loose 1, max_err_vs_fp32 1.7e-3
#   brats-widths ([64, 96, 128, 192] 32^3 batch 1):          logits 1.9e-6, loss 7e-8, grad 0.030,  n_loose 8, max_err_vs_fp32 7.8e-3
#   heads        ([16, 32, 48, 64] 32^3 batch 2, K = 2):     logits 1.6e-6, loss 0,    grad 0.018,  n_loose 1, max_err_vs_fp32 2.0e-3
#   bf16 storage ([16, 32, 48, 64] 32^3 batch 2):            loss 0.9130553 with fp32 tensors, 0.9130418 with bf16-stored activations
NETWORK = {"three": ([32, 64, 96], (16, 24, 32), 2, 0), "brats-widths": ([64, 96, 128, 192], (32, 32, 32), 1, 0),
           "heads": ([16, 32, 48, 64], (32, 32, 32), 2, 2)}


@pytest.mark.parametrize("name", sorted(NETWORK))
def test_network_fwd_bwd(name):
    filters, dhw, n, K = NETWORK[name]
    torch.manual_seed(1234)
    m = (dyn.HipDynUNetDS(**RB.kw(filters, K)).cuda().train() if K else dyn.HipDynUNet(**RB.kw(filters)).cuda().eval())
    e = RB.pair(m, None, dhw, n, "cuda")
    print("record", name, {k: e[k] for k in ("n_loose", "max_err_vs_fp32")}, e)
    assert e["logits"] < RB.TOL and e["loss"] < RB.TOL and e["grad"] <= 1.0, e


def test_training_steps_track_the_oracle():
    """Three Adam steps: the loss of every step within 1e-3 of the torch restatement's under torch.optim.Adam."""
    torch.manual_seed(3)
    m = dyn.HipDynUNet(**RB.kw([16, 32, 48])).cuda().train()
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    x, y = R.synthetic_case(2, 4, (16, 16, 16), 3)
    opt_ref = torch.optim.Adam(list(sd.values()), lr=1e-3)
    opt = optim.HipAdam(m.parameters(), lr=1e-3)
    crit = losses.HipDiceLoss(sigmoid=True)
    xg, yg = x.cuda(), y.cuda()
    for _ in range(3):
        opt_ref.zero_grad()
        l0 = O.dice_loss(RB.res_dynunet_forward(sd, x, 3), y)
        l0.backward()
        opt_ref.step()
        opt.zero_grad()
        l1 = crit(m(xg), yg)
        l1.backward()
        opt.step()
        assert abs(float(l1.detach()) - float(l0.detach())) / abs(float(l0.detach())) < RB.TOL, (float(l1.detach()), float(l0.detach()))


def _build():
    torch.manual_seed(3)
    m = dyn.HipDynUNet(**RB.kw([16, 32, 48])).cuda().train()
    return m, losses.HipDiceLoss(sigmoid=True), optim.HipAdam(m.parameters(), lr=1e-3)


def test_graphed_step_equals_eager_step(hip_backend):
    """Two replays of the captured step equal two eager steps, bit for bit."""
    batches = [tuple(t.cuda() for t in R.synthetic_case(1, 4, (16, 16, 16), 3, seed=s)) for s in range(2)]
    m0, crit0, opt0 = _build()
    want = [float(DS.train_step(m0, crit0, x, y, opt0)[0]) for x, y in batches]
    m1, crit1, opt1 = _build()
    step = graph.HipGraphedTrainStep(m1, crit1, opt1, *batches[0])
    got = [float(step(x, y).item()) for x, y in batches]
    assert got == want, (got, want)
    for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert torch.equal(a, b), k


def test_bf16_activation_storage_tracks_the_fp32_storage_run(hip_backend):
    """16-bit operands, activations stored as bf16 next to the same step with fp32 tensors: losses within 2e-3 of each other (the bound
    tests/test_act_storage_gpu.py holds a network's storage runs to), every gradient finite."""
    x, y = (t.cuda() for t in R.synthetic_case(2, 4, (32, 32, 32), 3))
    got = {}
    for storage in (None, torch.bfloat16):
        torch.manual_seed(1234)
        m = dyn.HipDynUNet(**RB.kw([16, 32, 48, 64])).cuda().train()
        m.conv_precision, m.act_storage = "bf16", storage
        crit = losses.HipDiceLoss(sigmoid=True)
        DS.bind(hip_backend, m, crit)
        loss, grads = DS.train_step(m, crit, x, y)
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        got[storage] = float(loss)
    print("record", got)
    assert abs(got[None] - got[torch.bfloat16]) < 2e-3, got
