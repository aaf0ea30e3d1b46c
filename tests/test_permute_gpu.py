"""The cases of tests/test_permute.py through the HIP library on an MI355X, against the same restatements, oracle and bound
(tests/permute_cases.py), plus one 2 x 3 x 33 x 70 x 130 batch so that every launch has many workgroups in flight. Hostile memory as on
the emulator: poisoned, exact-size, guarded outputs, identical bits. The reference is met through the committed fixture only."""
import importlib

import pytest
import torch

import permute_cases as K
import test_permute as T

permute = importlib.import_module("3dunetcnn_amd.permute")
pytestmark = pytest.mark.gpu


def test_reference_fixture(hip_backend):
    T.check_reference_fixture(hip_backend)


@pytest.mark.parametrize("elem", (1, 2, 4))
def test_all_keys_on_a_small_batch(hip_backend, elem):
    T.test_all_keys_on_a_small_batch(hip_backend, elem)


@pytest.mark.parametrize("elem", (1, 2, 4))
@pytest.mark.parametrize("shape", K.TILE_SHAPES)
def test_all_keys_across_the_tile(hip_backend, shape, elem):
    T.test_all_keys_across_the_tile(hip_backend, shape, elem)


@pytest.mark.parametrize("elem", (1, 2, 4))
def test_extents_of_one_and_around_the_tile(hip_backend, elem):
    T.test_extents_of_one_and_around_the_tile(hip_backend, elem)


def test_public_forms(hip_backend):
    T.check_public_forms(hip_backend)
    x = K.volume((3, 4, 5, 6), 4).cuda()                           # the default backend, from the tensor's device
    key = ((1, 0, 2), 0, 1, 0, 1)
    got = permute.permute_data(x, key)
    assert got.is_cuda and torch.equal(got, permute.permute_data(x, key, _backend=hip_backend))


def test_per_sample_keys(hip_backend):
    T.check_per_sample_keys(hip_backend)


def test_fold_is_the_inverse_permutation(hip_backend):
    T.check_fold_is_the_inverse_permutation(hip_backend)


@pytest.mark.parametrize("activation", ("sigmoid", "softmax"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_fold_within_its_bound(hip_backend, activation, dtype):
    """The bound is K.fold_bound, derived at the top of permute_cases.py: 1e-6 + (K + 1) * 2^-24."""
    K.check_fold(hip_backend, T.FOLD_SHAPE, K.FLIP_KEYS, activation, dtype, say="MI355X")
    K.check_fold(hip_backend, K.SMALL_SHAPE, K.KEYS48, activation, dtype, seed=1, say="MI355X")
    K.check_fold(hip_backend, T.FOLD_TILE_SHAPE, K.KEYS48[1::6], activation, dtype, seed=2, say="MI355X")
    if dtype == torch.bfloat16:
        K.check_fold(hip_backend, T.FOLD_SHAPE, K.FLIP_KEYS, activation, torch.float16, seed=3, say="MI355X")


def test_ensemble(hip_backend):
    T.check_ensemble(hip_backend)


def test_ensemble_as_the_inferers_network(hip_backend):
    T.check_ensemble_as_the_inferers_network(hip_backend)


def test_abi_rejects_bad_arguments(hip_backend):
    T.check_abi_rejects_bad_arguments(hip_backend)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", T.HOSTILE)
def test_op_on_hostile_memory(hip_backend, name):
    T.hold_op(hip_backend, name)


@pytest.mark.parametrize("elem", (1, 2, 4))
def test_batch_with_many_workgroups_per_launch(hip_backend, elem):
    """All 48 keys, compared on the device against the torch chain; a second call gives the same bits."""
    be = hip_backend
    x = K.volume(K.MANY_WG_SHAPE, elem, seed=5).cuda()
    for key in K.KEYS48:
        y = permute.permute_data(x, key, _backend=be)
        assert torch.equal(y, K.restate(x, key)), key
        assert torch.equal(permute.permute_data(x, key, _backend=be), y), key
        assert torch.equal(permute.reverse_permute_data(y, key, _backend=be), x), key


def test_fold_with_many_workgroups_per_launch(hip_backend):
    be = hip_backend
    shape = (2, 3, 33, 70, 132)
    first = K.check_fold(be, shape, K.KEYS48[::7], "softmax", torch.float32, seed=6, say="MI355X, many workgroups")
    again = K.check_fold(be, shape, K.KEYS48[::7], "softmax", torch.float32, seed=6)
    assert torch.equal(first, again)
    K.check_fold(be, shape, K.FLIP_KEYS, "sigmoid", torch.bfloat16, seed=7, say="MI355X, many workgroups")
