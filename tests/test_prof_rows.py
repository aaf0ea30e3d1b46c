"""The profile rows of Backend.conv_fwd / conv_fwd_wino / conv_wgrad / c4_bwd on the CPU emulator, against tests/golden/prof_rows.json
(tests/prof_rows_cases.py states the cases; tests/golden/make_prof_rows.py wrote the fixture). The rows need torch.cuda.Event, so a
stub takes its place here; the GPU twin (tests/test_prof_rows_gpu.py) records real events against the same fixture."""
import pytest
import torch

import prof_rows_cases as P


@pytest.fixture
def rows_of(emu_backend, monkeypatch):
    monkeypatch.setattr(torch.cuda, "Event", P.StubEvent)
    monkeypatch.delenv("MI355_PROF_SHAPES", raising=False)
    return lambda name: P.run_case(emu_backend, name)


@pytest.mark.parametrize("name", list(P.CASES))
def test_prof_rows_match_the_fixture(rows_of, name):
    rows = rows_of(name)
    P.assert_rows_match(rows, P.load_fixture()[name])
    assert rows and all(len(r) == 7 and type(r[3]) is P.StubEvent and type(r[4]) is P.StubEvent and r[3] is not r[4] for r in rows)
    families = [r[0] for r in rows]
    if name == "wino2d":
        assert {"conv3d_wino2d", "conv3d_wgrad_wino_ring (+reduce)"} <= set(families) and "conv3d_wino3d" not in families
    elif name == "wino3d":
        assert "conv3d_wino3d" in families            # mi355_conv3d_wino3d_supported accepts at least one layer of the bundle
    elif name == "direct":
        assert not any("wino" in f for f in families) and all(r[5] is None for r in rows)
    elif name == "bf16":
        assert "conv3d_wgrad_k3_bf16<...> (+reduce)" in families
        assert any(r[0] == "conv3d_k3_bf16<...>" and r[5].startswith(("conv3d_k3_bf16<", "conv3d_k3_lp_zring")) for r in rows)
    elif name == "c4_bwd":
        # the two passes the fused kernel replaces: twice the forward's figures (n = 1, 2 x 3 x 5 voxels, 4 -> 32 channels)
        assert P.compared(rows) == [["conv3d_c4_bwd (+reduce)", 2 * 2.0 * 30 * 4 * 32 * 27, 2 * 4.0 * (30 * (4 + 32) + 27 * 4 * 32), None, 0.0]]


def test_no_bundle_reaches_the_fused_first_layer_backward():
    """... which is why the c4_bwd case calls Backend.c4_bwd directly (32 output channels of the first block are needed)."""
    fx = P.load_fixture()
    assert all(row[0] != "conv3d_c4_bwd (+reduce)" for name, rows in fx.items() if name != "c4_bwd" for row in rows)
