"""HipFocalLoss / HipDiceFocalLoss / HipTverskyLoss on the HIP library: the tables of tests/focal_cases.py (what tests/test_focal_losses.py
runs on the emulator) at tests/test_losses.py's GPU shape, one case per loss past the focal kernel's grid cap, the hostile-memory rows
and one graphed training step."""
import importlib

import pytest
import torch

import focal_cases as FC
import scratch_guard as G
from oracle import unet3d_ref as R          # synthetic inputs only

losses = FC.losses
graph = importlib.import_module("3dunetcnn_amd.graph")
unet = importlib.import_module("3dunetcnn_amd.unet")
optim = importlib.import_module("3dunetcnn_amd.optim")
pytestmark = pytest.mark.gpu
DHW = (40, 48, 36)                  # ragged 256-thread tails, 16 Dice partial blocks
# focal_kernel keeps ce_kernel's grid cap (1024 blocks x 256 threads = 262 144 voxels of the batch per trip): N * V = 2 * 188 160 = 376 320
# gives its grid-stride loop a second, ragged trip
DHW_PAST_CAP = (48, 56, 70)


@pytest.mark.parametrize("name,mk,ref,c", FC.CASES, ids=FC.IDS)
def test_parity_gpu(hip_backend, name, mk, ref, c):
    FC.check(mk(), ref, None, "cuda", 2, c, DHW, name)


def test_tversky_none_gpu(hip_backend):
    FC.check_none(FC.NONE_KW, None, "cuda", 2, 3, DHW)
    FC.check_none(dict(FC.NONE_KW, batch=True, include_background=False), None, "cuda", 2, 3, DHW)


@pytest.mark.parametrize("name", ["focal_g1.5_alpha", "dicefocal", "tversky_03_07"])
def test_past_the_grid_cap_and_same_bits_twice(hip_backend, name):
    _, mk, ref, c = FC.case(name)
    assert c == 3 and 2 * DHW_PAST_CAP[0] * DHW_PAST_CAP[1] * DHW_PAST_CAP[2] > 1024 * 256
    first = FC.check(mk(), ref, None, "cuda", 2, c, DHW_PAST_CAP, name)
    again = FC.check(mk(), ref, None, "cuda", 2, c, DHW_PAST_CAP, name)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


ROWS = FC.rows((24, 20, 28))        # more than one block in every pass, ragged tails


@pytest.mark.parametrize("rid", sorted(ROWS))
def test_on_hostile_memory_gpu(hip_backend, rid):
    case, fills = ROWS[rid]
    assert G.hold(hip_backend, lambda: case(hip_backend), fills).results > 0


def _build():
    torch.manual_seed(3)
    return unet.HipUNet3D(n_features=4, n_outputs=3, base_width=16, encoder_blocks=[1, 2, 2]).cuda().eval()


def test_graphed_step_equals_eager_step(hip_backend):
    """tests/test_graph.py's test of the same name (its network, shapes and single-stream capture) with HipDiceFocalLoss(sigmoid=True):
    two graphed steps equal two eager steps, losses and weights bit for bit."""
    batches = [tuple(t.cuda() for t in R.synthetic_case(2, 4, (32, 32, 32), 3, seed=s)) for s in range(2)]
    m0 = _build()
    crit0, opt0 = losses.HipDiceFocalLoss(sigmoid=True), optim.HipAdam(m0.parameters(), lr=1e-3)
    want = []
    for x, y in batches:
        opt0.zero_grad(set_to_none=True)
        loss = crit0(m0(x), y)
        loss.backward()
        opt0.step()
        want.append(float(loss.detach()))
    m1 = _build()
    crit1, opt1 = losses.HipDiceFocalLoss(sigmoid=True), optim.HipAdam(m1.parameters(), lr=1e-3)
    step = graph.HipGraphedTrainStep(m1, crit1, opt1, *batches[0])
    got = []
    for x, y in batches:
        opt1.zero_grad(set_to_none=True)
        got.append(float(step(x, y).item()))
    assert got == want, (got, want)
    for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert torch.equal(a, b), k
