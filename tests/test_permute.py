"""Volume permutations and the permutation-ensemble fold (csrc/permute.hip, 3dunetcnn_amd/permute.py) on the CPU emulator of the same
kernel sources: every key bit for bit against the torch chain it abbreviates (tests/permute_cases.py), the reference's own results
through the committed fixture, the fold against a float64 oracle within a derived bound, hostile memory, bad arguments, launch counts."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import permute_cases as K
import scratch_guard as G

permute = importlib.import_module("3dunetcnn_amd.permute")
inferer = importlib.import_module("3dunetcnn_amd.inferer")
_lib = importlib.import_module("3dunetcnn_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW = {"mi355_permute3d", "mi355_unpermute_accumulate"}
T = K.T


# ---- the keys and the reference --------------------------------------------------------------------------------------------------------
def test_key_set_is_the_references():
    fx = K.fixture()
    assert {K.as_key(k) for k in fx["keys"]} == permute.generate_permutation_keys() and len(fx["keys"]) == 48
    assert len({permute.key_code(k) for k in K.KEYS48}) == 48 and len(K.FLIP_KEYS) == 8
    assert all(c["reverse_gives_input"] for c in fx["cases"])
    assert [K.as_key(c["key"]) for c in fx["cases"][48:]][:2] == [((1, 3), 1, 0, 1, 1), ((0, 1), 0, 1, 0, 1)]
    for key in K.ALL_KEYS:
        rot = key[0] if len(key[0]) == 3 else (0,) + tuple(key[0])
        assert permute.reverse_permutation_key(key) == (tuple(-r for r in rot),) + tuple(key[1:])
    g = torch.Generator().manual_seed(5)
    drawn = {permute.random_permutation_key(g) for _ in range(400)}
    assert drawn <= permute.generate_permutation_keys() and len(drawn) > 40
    assert permute.random_permutation_key() in permute.generate_permutation_keys()


def test_restatement_is_pinned_to_the_reference_fixture():
    fx = K.fixture()
    x = torch.arange(120).reshape(fx["shape"])
    for case in fx["cases"]:
        y = K.restate(x, K.as_key(case["key"]))
        assert list(y.shape) == case["shape"] and y.reshape(-1).tolist() == case["values"], case["key"]
        assert torch.equal(K.restate_reverse(y, K.as_key(case["key"])), x)


def check_reference_fixture(be):
    fx = K.fixture()
    for dtype in (torch.int32, torch.int16, torch.uint8):
        x = torch.arange(120).reshape(fx["shape"]).to(dtype)
        for case in fx["cases"]:
            key = K.as_key(case["key"])
            y = permute.permute_data(x.to(be.device), key, _backend=be)
            assert list(y.shape) == case["shape"] and y.dtype == dtype and y.cpu().reshape(-1).tolist() == case["values"], (dtype, key)
            K.same(permute.reverse_permute_data(y, key, _backend=be), x, f"reverse {key}")


def test_reference_fixture(emu_backend):
    check_reference_fixture(emu_backend)


# ---- every key, both routes, three element sizes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", (1, 2, 4))
def test_all_keys_on_a_small_batch(emu_backend, elem):
    K.check_keys(emu_backend, K.SMALL_SHAPE, elem, K.ALL_KEYS)
    K.check_keys(emu_backend, K.SMALL_SHAPE, elem, K.ALL_KEYS, odd_offset=True, seed=1)
    K.check_keys(emu_backend, K.VEC_SHAPE, elem, K.ALL_KEYS, seed=2)                      # rows of whole 16-byte groups, both directions
    K.check_keys(emu_backend, K.VEC_SHAPE, elem, K.ALL_KEYS, odd_offset=True, seed=3)     # ... and the fall-back from them


@pytest.mark.parametrize("elem", (1, 2, 4))
@pytest.mark.parametrize("shape", K.TILE_SHAPES)
def test_all_keys_across_the_tile(emu_backend, shape, elem):
    K.check_keys(emu_backend, shape, elem, K.ALL_KEYS, odd_offset=True)


@pytest.mark.parametrize("elem", (1, 2, 4))
def test_extents_of_one_and_around_the_tile(emu_backend, elem):
    for shape in K.EDGE_SHAPES:
        K.check_keys(emu_backend, shape, elem, K.KEYS48[::5] + K.OLD_FORM_KEYS[:1] + K.TRANSPOSED_KEYS[:1], odd_offset=elem == 2)
    for shape in K.EDGE_SHAPES[:4]:
        K.check_keys(emu_backend, shape, elem, K.ALL_KEYS)


def check_public_forms(be):
    host = K.volume((3, 4, 5, 6), 4)
    x = host.to(be.device)
    key = ((1, 0, 2), 0, 1, 0, 1)
    K.same(permute.permute_data(x, key, _backend=be), K.restate(host, key), "[C, D, H, W]")
    half = host.to(torch.bfloat16)
    K.same(permute.permute_data(half.to(be.device), key, _backend=be), K.restate(half, key), "bf16")
    view = host.transpose(2, 3)                                   # not dense: the module makes it so
    K.same(permute.permute_data(view.to(be.device), key, _backend=be), K.restate(view.contiguous(), key), "a strided input")
    for t in (host.double(), host.long()):
        with pytest.raises(NotImplementedError):
            permute.permute_data(t.to(be.device), key, _backend=be)
    with pytest.raises(ValueError):
        permute.permute_data(x[0], key, _backend=be)
    with pytest.raises(RuntimeError, match="MI355X"):
        permute.permute_data(host, key)
    g = torch.Generator().manual_seed(11)
    label = K.volume((2, 4, 5, 6), 1, seed=4)
    xp, yp = permute.random_permutation_x_y(x, label.to(be.device), generator=g, _backend=be)
    drawn = permute.random_permutation_key(torch.Generator().manual_seed(11))
    K.same(xp, K.restate(host, drawn), "x of random_permutation_x_y")
    K.same(yp, K.restate(label, drawn), "y of random_permutation_x_y")
    last = host.movedim(0, -1).contiguous()
    xl, _ = permute.random_permutation_x_y(last.to(be.device), last.to(be.device), channel_axis=3, generator=torch.Generator().manual_seed(11),
                                           _backend=be)
    K.same(xl.contiguous(), K.restate(host, drawn).movedim(0, -1).contiguous(), "channels last")


def test_public_forms(emu_backend):
    check_public_forms(emu_backend)


# ---- one key per sample --------------------------------------------------------------------------------------------------------------------
def check_per_sample_keys(be):
    keys = [((0, 0, 0), 0, 0, 1, 0), ((1, 0, 0), 0, 0, 0, 0), ((0, 1, 1), 1, 0, 0, 0), ((0, 0, 1), 0, 1, 0, 0)]      # both routes in one launch
    assert len({permute.key_code(k) for k in keys}) == 4 and {(permute.key_code(k) >> 4) & 3 for k in keys} > {2}
    for elem in (1, 2, 4):
        host = K.volume((4, 2, 6, 6, 6), elem, seed=elem)
        got = permute.permute_batch(host.to(be.device), keys, _backend=be)
        K.same(got, torch.stack([K.restate(host[i], keys[i]) for i in range(4)]), f"per-sample keys, elem={elem}")
    host = K.volume((4, 2, 6, 6, 6), 4)
    K.same(permute.permute_batch(host.to(be.device), keys[:1] * 4, _backend=be), K.restate(host, keys[0]), "the same key four times")
    flat = K.volume((2, 2, 4, 6, 6), 4)                            # D differs from H = W: keys that only mix H and W still agree
    hw = [((1, 0, 0), 0, 0, 0, 0), ((0, 0, 0), 0, 1, 1, 1)]
    K.same(permute.permute_batch(flat.to(be.device), hw, _backend=be), torch.stack([K.restate(flat[i], hw[i]) for i in range(2)]), "H-W keys")
    with pytest.raises(ValueError, match="different shapes"):
        permute.permute_batch(flat.to(be.device), [keys[0], keys[2]], _backend=be)
    with pytest.raises(ValueError):
        permute.permute_batch(flat.to(be.device), keys[:1], _backend=be)
    n = _lib.PERMUTE_MAX_BATCH + 3                                 # above the cap: split into two launches
    many = K.volume((n, 1, 2, 2, 2), 2, seed=8)
    mk = [K.KEYS48[(7 * i) % 48] for i in range(n)]
    on_emulator = be.device.type == "cpu"
    if on_emulator:
        _take(be)
    got = permute.permute_batch(many.to(be.device), mk, _backend=be)
    if on_emulator:
        assert len(_take(be)) == 2
    K.same(got, torch.stack([K.restate(many[i], mk[i]) for i in range(n)]), "above the cap")


def test_per_sample_keys(emu_backend):
    check_per_sample_keys(emu_backend)


# ---- the fold ------------------------------------------------------------------------------------------------------------------------------
FOLD_SHAPE = (2, 3, 5, 6, 8)                  # W a multiple of 4: four voxels per thread on the row route
FOLD_TILE_SHAPE = (1, 3, 2, T + 1, T + 3)     # crosses the tile both ways; W odd


def check_fold_is_the_inverse_permutation(be):
    for shape, keys in ((K.SMALL_SHAPE, K.ALL_KEYS), (FOLD_SHAPE, K.ALL_KEYS), (FOLD_TILE_SHAPE, K.KEYS48[::4] + K.TRANSPOSED_KEYS)):
        host = K.volume(shape, 4, seed=6)
        host.view(-1)[::7] *= -0.0                                  # signed zeros survive a bit copy
        for key in keys:
            src = K.restate(host, key)
            code = permute.key_code(key)
            poisoned = torch.full(shape, float("nan")).to(be.device)
            acc = be.unpermute_accumulate(src.to(be.device), [code], poisoned, None, 1.0, init=True)
            assert acc is poisoned
            K.same(acc, host, f"init onto NaN {shape} {key}")
            base = K.volume(shape, 4, seed=9)
            acc = be.unpermute_accumulate(src.to(be.device), [code], base.clone().to(be.device), None, 1.0, init=False)
            K.same(acc, base + host, f"init=0 adds {shape} {key}")   # fma(1, x, a) and a + x: the one rounding of the exact sum
            acc = be.unpermute_accumulate(src.to(be.device), [code], base.clone().to(be.device), None, -0.5, init=False)
            K.same(acc, base + host * -0.5, f"weight -0.5 {shape} {key}")      # (a product by a power of two is exact)
        for dtype in (torch.bfloat16, torch.float16):
            src = K.restate(host, keys[5]).to(dtype)
            acc = be.unpermute_accumulate(src.to(be.device), [permute.key_code(keys[5])], None, None, 1.0)
            K.same(acc, K.restate_reverse(src, keys[5]).float(), f"{dtype} source")
    keys = [((0, 0, 0), 0, 0, 1, 0), ((1, 0, 0), 0, 0, 0, 0), ((0, 1, 1), 1, 0, 0, 0), ((0, 0, 1), 0, 1, 0, 0)]
    host = K.volume((4, 2, 6, 6, 6), 4, seed=3)                      # one key per sample
    src = torch.stack([K.restate(host[i], keys[i]) for i in range(4)])
    acc = be.unpermute_accumulate(src.to(be.device), [permute.key_code(k) for k in keys], None, None, 1.0)
    K.same(acc, host, "per-sample codes")


def test_fold_is_the_inverse_permutation(emu_backend):
    check_fold_is_the_inverse_permutation(emu_backend)


@pytest.mark.parametrize("activation", ("sigmoid", "softmax"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_fold_within_its_bound(emu_backend, activation, dtype):
    """Against the float64 oracle mean_k reverse(act(src_k)); the bound is K.fold_bound (derived at the top of permute_cases.py):
    1e-6 + (K + 1) * 2^-24."""
    K.check_fold(emu_backend, FOLD_SHAPE, K.FLIP_KEYS, activation, dtype, say="emulator")
    K.check_fold(emu_backend, K.SMALL_SHAPE, K.KEYS48, activation, dtype, seed=1, say="emulator")
    K.check_fold(emu_backend, FOLD_TILE_SHAPE, K.KEYS48[1::6], activation, dtype, seed=2, say="emulator")
    if dtype == torch.bfloat16:
        K.check_fold(emu_backend, FOLD_SHAPE, K.FLIP_KEYS, activation, torch.float16, seed=3, say="emulator")


# ---- the ensemble --------------------------------------------------------------------------------------------------------------------------
def check_ensemble(be):
    host = K.logits((2, 3, 5, 6, 8), seed=4)                       # not a cube
    x = host.to(be.device)
    for keys, names in (("flips", K.FLIP_KEYS), ("all", K.KEYS48), (K.OLD_FORM_KEYS + K.TRANSPOSED_KEYS, K.OLD_FORM_KEYS + K.TRANSPOSED_KEYS)):
        for activation in ("sigmoid", "softmax", None):
            ens = permute.PermutationEnsemble(K.predictor, keys, activation, _backend=be)
            assert ens.keys == [tuple(k) for k in names]
            got = ens(x)
            want, peak = K.ensemble_oracle(host, names, activation)
            # no activation: nothing is approximated (no 1e-6) and the K + 1 roundings are half ulps of numbers below the largest |prediction|
            bound = K.fold_bound(len(names)) if activation else (len(names) + 1) * 2.0 ** -24 * peak
            err = float((got.cpu().double() - want).abs().max())
            assert got.dtype == torch.float32 and got.shape == host.shape and err <= bound, (keys, activation, err, bound)
    # a wrong inverse cannot hide: the predictor is symmetric under no key
    for key in K.KEYS48[1:]:
        assert not torch.equal(K.restate_reverse(K.predictor(K.restate(host, key))[0], key), K.predictor(host)[0]), key
    with pytest.raises(ValueError):
        permute.PermutationEnsemble(K.predictor, "rotations", _backend=be)
    with pytest.raises(ValueError):
        permute.PermutationEnsemble(K.predictor, "flips", "tanh", _backend=be)
    with pytest.raises(RuntimeError, match="MI355X"):
        permute.PermutationEnsemble(K.predictor)(host)


def test_ensemble(emu_backend):
    check_ensemble(emu_backend)


def check_ensemble_as_the_inferers_network(be):
    host = K.logits((1, 3, 6, 6, 6), seed=7)
    inf = inferer.HipSlidingWindowInferer(roi_size=(4, 4, 4), sw_batch_size=2, overlap=0.25)
    inf._be = be
    got = inf(host.to(be.device), permute.PermutationEnsemble(K.predictor, "flips", "sigmoid", _backend=be))
    want = inf(host.to(be.device), lambda win: K.ensemble_oracle(win.cpu(), K.FLIP_KEYS, "sigmoid")[0].float().to(be.device))
    # the inferer's result is a convex combination of window predictions (weights / their sum): it carries the fold's bound, plus the
    # rounding of the oracle to fp32 (2^-25) and the inferer's own arithmetic on either side: at most 8 windows cover a voxel, so at most
    # 8 products, 8 additions and one division, each within 2^-24 of a value <= 1 -- 17 * 2^-24 per side
    assert got.shape == host.shape and float((got - want).abs().max()) <= K.fold_bound(8) + 2.0 ** -25 + 34 * 2.0 ** -24


def test_ensemble_as_the_inferers_network(emu_backend):
    check_ensemble_as_the_inferers_network(emu_backend)


def _take(be):
    fn = be.lib.emu_take_launches
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(65536)
    fn(buf, 65536)
    return buf.value.decode().split()


def test_launch_counts(emu_backend):
    """One launch per permutation whatever the key; K + K for an ensemble of K keys whatever the data."""
    be = emu_backend
    x = K.volume(K.SMALL_SHAPE, 4)
    for key in K.ALL_KEYS:
        _take(be)
        y = permute.permute_data(x, key, _backend=be)
        permute.reverse_permute_data(y, key, _backend=be)
        assert len(_take(be)) == 2, key
    for keys, count in (("flips", 8), ("all", 48)):
        runs = []
        for data in (torch.zeros(1, 3, 3, 4, 5), K.logits((1, 3, 3, 4, 5)), torch.full((1, 3, 3, 4, 5), float("nan"))):
            _take(be)
            permute.PermutationEnsemble(K.predictor, keys, "softmax", _backend=be)(data)
            runs.append(_take(be))
        assert runs[0] == runs[1] == runs[2] and len(runs[0]) == 2 * count, (keys, runs[0])
        assert sum("unpermute_accumulate" in name for name in runs[0]) == count


# ---- hostile memory ------------------------------------------------------------------------------------------------------------------------
def _hostile(be, name):
    rows, tile = ((0, 0, 0), 1, 0, 1, 0), ((1, 0, 2), 0, 1, 0, 0)
    shape = (2, 3, 3, T + 1, 24)
    if name.startswith("permute"):
        x = K.volume(shape, int(name[-1]), seed=2).to(be.device)
        return [permute.permute_data(x, key, _backend=be) for key in (rows, tile)] + [permute.permute_batch(x, [rows, rows], _backend=be)]
    activation, dtype = {"fold_none": (None, torch.float32), "fold_sigmoid": ("sigmoid", torch.bfloat16), "fold_softmax": ("softmax", torch.float32)}[name]
    x = K.logits(shape, seed=3)
    return [be.unpermute_accumulate(K.restate(x, key).to(dtype).to(be.device), [permute.key_code(key)], None, activation, 0.5)
            for key in (rows, tile)] + [permute.PermutationEnsemble(K.predictor, [rows, tile], activation, _backend=be)(x.to(be.device))]


HOSTILE = ("permute1", "permute2", "permute4", "fold_none", "fold_sigmoid", "fold_softmax")


def hold_op(be, name):
    """scratch_guard.hold: clean twice (same bits), then with every `empty` tensor of ops.py pre-filled with QNAN and with ONES inside
    guard bands: same bits again, every guard byte untouched. The outputs are exact-size: a write past the end lands in a guard."""
    held = G.hold(be, lambda: _hostile(be, name), fills=(G.QNAN, G.ONES), modules=(permute,))
    assert held.results == 3 and held.allocations >= 3, held
    return held


@pytest.mark.parametrize("name", HOSTILE)
def test_op_on_hostile_memory(emu_backend, name):
    hold_op(emu_backend, name)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def check_abi_rejects_bad_arguments(be):
    lib = be.lib
    n, c, d, h, w = 2, 3, 4, 5, 6
    x = torch.zeros(n, c, d, h, w).to(be.device)
    y, acc = torch.zeros_like(x), torch.zeros_like(x)
    big = torch.zeros(_lib.PERMUTE_MAX_BATCH + 1, 1, 2, 2, 2).to(be.device)
    xp, yp, ap, bp = x.data_ptr(), y.data_ptr(), acc.data_ptr(), big.data_ptr()

    def codes(*vals):
        return (ctypes.c_int32 * len(vals))(*vals)

    ident, swap_dh, swap_hw = 0 | 1 << 2 | 2 << 4, 1 | 0 << 2 | 2 << 4, 0 | 2 << 2 | 1 << 4
    one = codes(ident)
    assert lib.mi355_permute3d(xp, yp, n, c, d, h, w, 4, one, 1, 0) == 0
    assert lib.mi355_permute3d(xp, yp, n, c, d, h, w, 4, codes(ident, ident | 1 << 8), 2, 0) == 0
    assert lib.mi355_permute3d(bp, yp, 1, 1, 2, 2, 2, 4, one, 1, 0) == 0
    many = codes(*[ident] * (_lib.PERMUTE_MAX_BATCH + 1))
    bad_permute = [
        (None, yp, n, c, d, h, w, 4, one, 1), (xp, None, n, c, d, h, w, 4, one, 1), (xp, yp, n, c, d, h, w, 4, None, 1),      # null pointers
        (xp, yp, 0, c, d, h, w, 4, one, 1), (xp, yp, n, 0, d, h, w, 4, one, 1), (xp, yp, n, c, 0, h, w, 4, one, 1),           # extents
        (xp, yp, n, c, d, -1, w, 4, one, 1), (xp, yp, n, c, d, h, 0, 4, one, 1), (xp, yp, -2, c, d, h, w, 4, one, 1),
        (xp, xp, n, c, d, h, w, 4, one, 1),                                                                                   # src == dst
        (xp, yp, n, c, d, h, w, 0, one, 1), (xp, yp, n, c, d, h, w, 3, one, 1), (xp, yp, n, c, d, h, w, 8, one, 1),           # elem_bytes
        (xp, yp, n, c, d, h, w, 4, codes(0), 1), (xp, yp, n, c, d, h, w, 4, codes(0 | 1 << 2 | 1 << 4), 1),                   # no permutation
        (xp, yp, n, c, d, h, w, 4, codes(3 | 1 << 2 | 2 << 4), 1), (xp, yp, n, c, d, h, w, 4, codes(ident | 1 << 9), 1),
        (xp, yp, n, c, d, h, w, 4, codes(-1), 1),
        (xp, yp, n, c, d, h, w, 4, codes(ident, ident, ident), 3), (xp, yp, n, c, d, h, w, 4, one, 0),                        # n_codes
        (xp, yp, 3, c, d, h, w, 4, codes(ident, ident), 2),
        (bp, yp, _lib.PERMUTE_MAX_BATCH + 1, 1, 2, 2, 2, 4, many, _lib.PERMUTE_MAX_BATCH + 1),                                # above the cap
        (xp, yp, n, c, d, h, w, 4, codes(ident, swap_dh), 2), (xp, yp, n, c, d, h, w, 4, codes(swap_hw, ident), 2),           # different extents
    ]
    for args in bad_permute:
        assert lib.mi355_permute3d(*args, 0) == EINVAL, args
    nan = float("nan")
    assert lib.mi355_unpermute_accumulate(xp, 0, ap, n, c, d, h, w, one, 1, 2, 0.5, 1, 0) == 0
    assert lib.mi355_unpermute_accumulate(xp, 1, ap, n, c, d, h, w, codes(ident, ident | 1 << 6), 2, 1, 0.5, 0, 0) == 0
    bad_fold = [
        (None, 0, ap, n, c, d, h, w, one, 1, 0, 1.0, 1), (xp, 0, None, n, c, d, h, w, one, 1, 0, 1.0, 1), (xp, 0, ap, n, c, d, h, w, None, 1, 0, 1.0, 1),
        (xp, 0, ap, 0, c, d, h, w, one, 1, 0, 1.0, 1), (xp, 0, ap, n, 0, d, h, w, one, 1, 0, 1.0, 1), (xp, 0, ap, n, c, 0, h, w, one, 1, 0, 1.0, 1),
        (xp, 0, ap, n, c, d, 0, w, one, 1, 0, 1.0, 1), (xp, 0, ap, n, c, d, h, -3, one, 1, 0, 1.0, 1),
        (xp, 0, xp, n, c, d, h, w, one, 1, 0, 1.0, 1),                                                                        # src == acc
        (xp, 3, ap, n, c, d, h, w, one, 1, 0, 1.0, 1), (xp, -1, ap, n, c, d, h, w, one, 1, 0, 1.0, 1),                        # src_elem
        (xp, 0, ap, n, c, d, h, w, codes(2 | 2 << 2 | 2 << 4), 1, 0, 1.0, 1), (xp, 0, ap, n, c, d, h, w, codes(ident | 1 << 10), 1, 0, 1.0, 1),
        (xp, 0, ap, n, c, d, h, w, codes(ident, ident, ident), 3, 0, 1.0, 1), (xp, 0, ap, n, c, d, h, w, one, 0, 0, 1.0, 1),
        (bp, 0, ap, _lib.PERMUTE_MAX_BATCH + 1, 1, 2, 2, 2, many, _lib.PERMUTE_MAX_BATCH + 1, 0, 1.0, 1),
        (xp, 0, ap, n, c, d, h, w, codes(ident, swap_dh), 2, 0, 1.0, 1),
        (xp, 0, ap, 1, 17, 1, 2, 2, one, 1, 2, 1.0, 1),                                                                       # c > 16 with softmax
        (xp, 0, ap, n, c, d, h, w, one, 1, 3, 1.0, 1), (xp, 0, ap, n, c, d, h, w, one, 1, -1, 1.0, 1),                        # activation
        (xp, 0, ap, n, c, d, h, w, one, 1, 0, nan, 1),                                                                        # NaN weight
    ]
    for args in bad_fold:
        assert lib.mi355_unpermute_accumulate(*args, 0) == EINVAL, args
    assert lib.mi355_unpermute_accumulate(xp, 0, ap, 1, 17, 1, 2, 2, one, 1, 1, 1.0, 1, 0) == 0      # 17 channels are fine without softmax
    # the Python layer raises
    with pytest.raises(RuntimeError, match="permute3d"):
        be.permute3d(x, [ident, swap_dh])
    with pytest.raises(RuntimeError, match="unpermute_accumulate"):
        be.unpermute_accumulate(x, [ident], None, None, nan)
    with pytest.raises(RuntimeError, match="unpermute_accumulate"):
        be.unpermute_accumulate(torch.zeros(1, 17, 1, 2, 2).to(be.device), [ident], None, "softmax", 1.0)
    with pytest.raises(AssertionError):
        be.permute3d(x, [ident] * 3)


def test_abi_rejects_bad_arguments(emu_backend):
    _take(emu_backend)
    check_abi_rejects_bad_arguments(emu_backend)
    assert len(_take(emu_backend)) == 6                          # only the six calls that were meant to succeed launched anything


def test_header_and_signatures(emu_backend):
    hdr = open(os.path.join(ROOT, "include", "mi355_unet3d.h")).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(_lib.SIGNATURES)
    for name in NEW:
        assert hasattr(emu_backend.lib, name)
    section = hdr[hdr.index("csrc/permute.hip"):]
    assert not re.search(r"_(workspace|blocks)\s*\(", section)
    for macro, value in (("PERMUTE_MAX_BATCH", _lib.PERMUTE_MAX_BATCH), ("PERMUTE_TILE", _lib.PERMUTE_TILE), ("ACT_NONE", _lib.ACT_NONE),
                         ("ACT_SIGMOID", _lib.ACT_SIGMOID), ("ACT_SOFTMAX", _lib.ACT_SOFTMAX)):
        assert int(re.search(rf"#define MI355_{macro} (\d+)", hdr).group(1)) == value, macro
    assert section.count("One launch") == 2
    for formula in ("s0 | s1 << 2 | s2 << 4 | f0 << 6 | f1 << 7 | f2 << 8", "out_extent[a] = E[s_a]", "u[s_a] = f_a ? out_extent[a] - 1 - v_a : v_a",
                    "(init ? 0 : acc[n, c, u]) + weight * p[n, c, v]"):
        assert formula in section, formula


def test_sources_never_wait_for_the_host_and_use_no_atomics():
    src = open(os.path.join(ROOT, "3dunetcnn_amd", "csrc", "permute.hip")).read()
    for word in ("hipMalloc", "hipMemcpy", "Synchronize", "hipFree", "atomicAdd", "atomicCAS", "atomicMax", "atomicMin", "cooperative"):
        assert word not in src, word
    mod = open(os.path.join(ROOT, "3dunetcnn_amd", "permute.py")).read()
    for word in (".item()", ".tolist()", ".cpu()", "synchronize", ".numpy()"):
        assert word not in mod, word
