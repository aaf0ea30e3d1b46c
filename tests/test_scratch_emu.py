"""Every op on poisoned, exact-size, guarded scratch, records and outputs -- on the CPU emulator (tests/scratch_guard.py is the harness,
tests/scratch_cases.py the rows and the entry-point coverage table; tests/test_scratch_gpu.py runs the same rows on the HIP library).

Invariant held: results do not depend on the prior contents of scratch, records or outputs, and no op writes outside what its size
query promised. Per row: two clean runs agree bit for bit; a run per poison pattern with every workspace cut to exactly the queried
size, every `empty` tensor of the package and every pre-made output filled with the pattern, all inside 64 KiB guard bands, passes the
case's own assertion, gives bit-identical results, and leaves every guard byte untouched.

The first tests are the harness's self-test: three fake ops written here (no kernel, no library call) -- one reads its workspace
without writing it, one writes one element past its output, one is correct -- must be told apart.

Cost (measured, 8 pytest-xdist workers): the op rows of this file alone 4 min 12 s; its self-tests, plane-ring, Winograd weight-gradient
and network rows (37 tests) alone 2 min 33 s. The network rows use a reduced UNet3D (scratch_cases.UNET_REDUCED says why).
"""
import os
import re
import sys

import pytest
import torch

import scratch_cases as SC
import scratch_guard as G

ops = SC.C.ops
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- self-test of the harness: pure Python, a Backend around no library ------------------------------------------------------------------
@pytest.fixture
def fake_backend():
    return ops.Backend(lib=object(), device="cpu")


def _op_correct(be, x):
    """partials into the workspace, folded into an `empty` output: the pattern of the library's two-launch reductions."""
    ws = be.ws(4 * x.shape[0])
    ws[:x.shape[0]] = x.sum(dim=1)
    out = torch.empty(1)                       # (this module's `torch` global is the harness's proxy inside `guarded`)
    out[0] = ws[:x.shape[0]].sum()
    return out


def _op_reads_unwritten_slot(be, x):
    ws = be.ws(4 * x.shape[0])
    ws[:x.shape[0] - 1] = x[:-1].sum(dim=1)    # the last "workgroup" returns early
    out = torch.empty(1)
    out[0] = ws[:x.shape[0]].sum()
    return out


def _op_writes_past_its_output(be, x):
    out = torch.empty(x.shape[0])
    out.copy_(x.sum(dim=1))
    beyond = torch.as_strided(out, (x.shape[0] + 1,), (1,))     # one element more than was asked for
    beyond[x.shape[0]] = 1.0
    return out


def _self(be, op):
    x = torch.arange(12.0).reshape(3, 4)
    return G.hold(be, lambda: op(be, x), fills=(G.QNAN, G.ONES), modules=(sys.modules[__name__],))


def test_harness_passes_a_correct_op(fake_backend):
    assert _self(fake_backend, _op_correct) == (1, 2)            # one result compared; the workspace and the output were guarded
    # every patch is undone; the only workspace left is the clean runs' own
    assert "ws" not in fake_backend.__dict__ and torch is sys.modules["torch"] and SC.C.OUT_FILL is None
    assert [w.numel() for w in fake_backend._ws_by_stream.values()] == [1 << 18]


def test_harness_sees_a_slot_that_was_read_but_not_written(fake_backend):
    # clean: the unwritten slot of Backend.ws's >= 1 MiB torch.empty buffer holds whatever it holds, the same in both clean runs (one
    # buffer, reused) -- the op "works", twice. All the test needs is that this is not the poison's bits, which a NaN sum guarantees
    with pytest.raises(G.PoisonDiffers, match="differ from the clean run"):
        _self(fake_backend, _op_reads_unwritten_slot)
    assert "ws" not in fake_backend.__dict__ and torch is sys.modules["torch"] and SC.C.OUT_FILL is None


def test_harness_sees_a_write_past_an_output(fake_backend):
    with pytest.raises(G.GuardViolated, match=r"\(3,\) torch.float32 allocated at tests/test_scratch_emu.py:\d+ _op_writes_past_its_output.*"
                                              r"4 guard bytes after the payload were written, first / last byte offset 0 / 3"):
        with G.guarded(fake_backend, G.QNAN, modules=(sys.modules[__name__],)):
            _op_writes_past_its_output(fake_backend, torch.ones(3, 4))
    assert torch is sys.modules["torch"]


def test_harness_reports_the_overrun_when_the_case_fails_first(fake_backend):
    with pytest.raises(G.GuardViolated, match="and the case then failed") as ei:
        with G.guarded(fake_backend, G.QNAN, modules=(sys.modules[__name__],)):
            _op_writes_past_its_output(fake_backend, torch.ones(3, 4))
            assert False, "the case's own assertion"
    assert isinstance(ei.value.__cause__, AssertionError) and "own assertion" in str(ei.value.__cause__)
    with pytest.raises(ZeroDivisionError):                     # without an overrun the case's failure is the failure
        with G.guarded(fake_backend, G.QNAN, modules=(sys.modules[__name__],)):
            1 / 0
    assert torch is sys.modules["torch"] and "ws" not in fake_backend.__dict__


def test_harness_allocations_are_exact_aligned_and_poisoned(fake_backend):
    with G.guarded(fake_backend, G.ONES, modules=(sys.modules[__name__],)) as g:
        ws = fake_backend.ws(10)
        a = torch.empty(3, 5, dtype=torch.bfloat16)
        b = torch.empty_like(torch.zeros(7, dtype=torch.uint8))
        i = torch.empty((2, 3), dtype=torch.int32)
        assert ws.shape == (3,) and ws.dtype == torch.float32 and a.shape == (3, 5) and b.shape == (7,) and i.shape == (2, 3)
        assert all(t.data_ptr() % G.ALIGN == 0 and t.is_contiguous() for t in (ws, a, b, i))
        assert bool(torch.isnan(ws).all()) and bool(torch.isnan(a).all()) and bool((b == 255).all()) and bool((i == -1).all())
        assert all(al.off >= G.GUARD and al.raw.numel() - al.off - al.nbytes >= G.GUARD for al in g.allocs) and G.GUARD >= 64 << 10
    with G.guarded(fake_backend, G.QNAN, modules=(sys.modules[__name__],)):
        h, f, w = torch.empty(4, dtype=torch.float16), torch.empty(4), torch.empty(4, dtype=torch.bfloat16)
        assert h.view(torch.int16).tolist() == [0x7e00] * 4 and f.view(torch.int32).tolist() == [0x7fc00000] * 4 and w.view(torch.int16).tolist() == [0x7fc0] * 4


# ---- the coverage table against the header -------------------------------------------------------------------------------------------------
def test_every_size_query_has_a_row():
    header = open(os.path.join(ROOT, "include", "mi355_unet3d.h")).read()
    queries = set(re.findall(r"\b(mi355_\w+(?:_workspace|_blocks))\s*\(", header))
    assert len(queries) >= 14, queries
    rows = set(SC.ROWS) | set(SC.GPU_ROWS) | set(SC.NETWORK_ROWS) | set(SC.GPU_NETWORK_ROWS)
    assert not queries - set(SC.COVERAGE), f"size queries of the header without a row in scratch_cases.COVERAGE: {sorted(queries - set(SC.COVERAGE))}"
    declared = set(re.findall(r"\b(mi355_\w+)\s*\(", header))
    assert not set(SC.COVERAGE) - declared, sorted(set(SC.COVERAGE) - declared)
    for entry, ids in SC.COVERAGE.items():
        assert ids and not set(ids) - rows, (entry, sorted(set(ids) - rows))


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", sorted(SC.ROWS))
def test_op_on_hostile_memory(emu_backend, rid):
    case, cfg, fills = SC.ROWS[rid]
    with G.configured(emu_backend, **cfg) as be:
        assert G.hold(be, lambda: case(be), fills).results > 0


@pytest.mark.parametrize("rid", sorted(SC.NETWORK_ROWS))
def test_network_on_hostile_memory(emu_backend, rid):
    case, cfg, fills = SC.NETWORK_ROWS[rid]
    with G.configured(emu_backend, **cfg) as be:
        held = G.hold(be, lambda: case(be), fills)
    assert held.results > 10 and held.allocations > 50, held      # logits, loss, every gradient; every activation, record and gradient buffer
