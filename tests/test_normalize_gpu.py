"""The cases of tests/test_normalize.py through the HIP library on an MI355X, against the same oracles and bounds
(tests/normalize_cases.py), plus one 3 x 48 x 56 x 70 volume so that every launch has many workgroups in flight and the histogram
atomics arrive from all XCDs. Hostile memory as on the emulator: poisoned, guarded scratch and outputs, identical bits. The reference
is met through the committed fixture only."""
import importlib

import numpy as np
import pytest
import torch

import normalize_cases as K
import test_normalize as T

normalize = importlib.import_module("3dunetcnn_amd.normalize")
prepost = importlib.import_module("3dunetcnn_amd.prepost")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", K.VALUE_SETS)
def test_percentiles_of_small_volumes(hip_backend, kind):
    for c in K.CHANNELS:
        for v in K.SMALL_SIZES:
            x = K.values(kind, c, v)
            for qs in K.Q_SETS:
                K.check_percentiles(hip_backend, x, qs, what=f"{kind} c={c} v={v} q={qs}")


@pytest.mark.parametrize("kind", K.VALUE_SETS)
def test_percentiles_with_several_workgroups(hip_backend, kind):
    x = K.values(kind, 3, K.LARGE_SIZE)
    for qs in K.Q_SETS:
        K.check_percentiles(hip_backend, x, qs, what=f"{kind} v={K.LARGE_SIZE} q={qs}")


@pytest.mark.parametrize("v", (3, 257, 4099, K.LARGE_SIZE))
def test_percentiles_above_a_device_threshold(hip_backend, v):
    for kind in ("gauss100", "zeros60", "one_nan"):
        x = K.values(kind, 3, v)
        s = np.sort(x.numpy()[~np.isnan(x.numpy())].reshape(-1))
        for above in ([s[-1]] * 3, [s[-2], s[-1], s[-3]], [s[-3], s[-2], K.NAN], [s[s.size // 3], 0.0, -np.inf], [K.NAN] * 3):
            for qs in ((0, 50, 99, 100), (0.9 * 100,)):
                K.check_percentiles(hip_backend, x, qs, above=above, what=f"{kind} v={v} above={above}")


@pytest.mark.parametrize("v", (1, 3, 255, 257, 4099, K.LARGE_SIZE))
def test_windows_are_the_torch_expressions(hip_backend, v):
    T.test_windows_are_the_torch_expressions(hip_backend, v)


@pytest.mark.parametrize("kind", ("gauss100", "offset1000", "tiny_minus5", "zeros60", "duplicates"))
def test_zscore_select_within_its_bound(hip_backend, kind):
    T.test_zscore_select_within_its_bound(hip_backend, kind)
    x = K.values(kind, 3, K.LARGE_SIZE)
    K.check_zscore(hip_backend, x, K.SELECT_ALL, 0.0, True, 1, False, what=f"{kind} large")
    K.check_zscore(hip_backend, x, K.SELECT_NONZERO, 0.0, True, 0, True, what=f"{kind} large, nonzero")
    K.check_zscore(hip_backend, x, K.SELECT_ABS_ABOVE, 1.5, False, 1, False, what=f"{kind} large, above")


def test_zscore_select_edge_cases(hip_backend):
    T.test_zscore_select_edge_cases(hip_backend)


@pytest.mark.parametrize("kind", ("gauss100", "zeros60", "offset1000"))
def test_composed_functions_against_their_restatements(hip_backend, kind):
    T.test_composed_functions_against_their_restatements(hip_backend, kind)


def test_what_the_functions_mean(hip_backend):
    T.test_what_the_functions_mean(hip_backend)
    x = T.volume("zeros60", 2, (5, 6, 7)).cuda()               # the default backend, from the tensor's device
    got = normalize.zero_one_window(x)
    assert got.is_cuda and torch.equal(got, normalize.zero_one_window(x, _backend=hip_backend))


def test_reference_fixture(hip_backend):
    K.check_against_reference(hip_backend, normalize)


def test_volume_with_many_workgroups_per_launch(hip_backend):
    be = hip_backend
    c, dhw = K.MANY_WG_SHAPE[0], K.MANY_WG_SHAPE[1:]
    mr = T.volume("zeros60", c, dhw, seed=9)
    first = K.check_percentiles(be, K.flat(mr), (1, 50, 0.9 * 100, 99), what="many workgroups, zeros60")
    K.check_percentiles(be, K.flat(mr), (99,), above=first[0][:, 0].cpu(), what="many workgroups, above the floor")
    K.check_percentiles(be, K.flat(T.volume("mixed", c, dhw, seed=9)), (0.1, 33.3, 99.9, 100), what="many workgroups, mixed")
    K.check_zscore(be, K.flat(T.volume("offset1000", c, dhw, seed=9)), K.SELECT_ALL, 0.0, True, 1, False, what="many workgroups, offset1000")
    K.check_zscore(be, K.flat(mr), K.SELECT_NONZERO, 0.0, True, 0, True, what="many workgroups, nonzero")
    a = K.check_zero_one_window(be, normalize, mr)
    K.check_zero_floor(be, normalize, mr)
    K.check_percentile_threshold(be, normalize, mr, 0.9)
    again = normalize.zero_one_window(mr.cuda())                # identical bits on a second call
    assert torch.equal(again.view(torch.int32), a.view(torch.int32))
    second = be.percentiles(K.flat(mr).cuda(), [1, 50, 0.9 * 100, 99], want_ranks=True)
    for g, h in zip(first, second):
        assert torch.equal(g.view(torch.int32), h.view(torch.int32))


@pytest.mark.parametrize("name", sorted(T.HOSTILE))
def test_op_on_hostile_memory(hip_backend, name):
    T.hold_op(hip_backend, name)
