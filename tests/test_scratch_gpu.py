"""Every op on poisoned, exact-size, guarded scratch, records and outputs -- on a real MI355X through libmi355unet3d.so. The rows and what
is asserted per row are those of tests/test_scratch_emu.py (tests/scratch_cases.py, tests/scratch_guard.py); on top of them each route
gets the smallest existing shape that reaches its multi-chunk / multi-workgroup path (scratch_cases.GPU_ROWS) and the product
network (HipUNet3D in its default configuration at 30 x 31 x 29, and at 32^3 batch 2 in bf16 with 16-bit storage). Measured on an MI355X: 183 rows in 11-25 s (15-42 s with
start-up; two runs), against 8.5 min for the whole GPU suite. Run with -x: after a violated guard the run should end rather than continue on possibly corrupted memory.
"""
import pytest

import scratch_cases as SC
import scratch_guard as G

pytestmark = pytest.mark.gpu

OP_ROWS = {**SC.ROWS, **SC.GPU_ROWS}
NET_ROWS = {**SC.NETWORK_ROWS, **SC.GPU_NETWORK_ROWS}


@pytest.mark.parametrize("rid", sorted(OP_ROWS))
def test_op_on_hostile_memory(hip_backend, rid):
    case, cfg, fills = OP_ROWS[rid]
    with G.configured(hip_backend, **cfg) as be:
        assert G.hold(be, lambda: case(be), fills).results > 0


@pytest.mark.parametrize("rid", sorted(NET_ROWS))
def test_network_on_hostile_memory(hip_backend, rid):
    case, cfg, fills = NET_ROWS[rid]
    with G.configured(hip_backend, **cfg) as be:
        held = G.hold(be, lambda: case(be), fills)
    assert held.results > 10 and held.allocations > 50, held      # logits, loss, every gradient; every activation, record and gradient buffer
