"""On-device volume permutations -- the 48 rotations and reflections of a volume -- and permutation-ensemble inference, with the names and
signatures of the reference's unet3d/utils/augment.py (generate_permutation_keys, permute_data, reverse_permute_data,
reverse_permutation_key, random_permutation_key, random_permutation_x_y). Everything runs in the two kernels of csrc/permute.hip; there is
no CPU fallback.

A KEY is the reference's tuple ((rotate_x, rotate_y, rotate_z), flip_x, flip_y, flip_z, transpose) over data [C, X, Y, Z]: quarter turns
about x (in the plane of dims 2, 3), y (dims 1, 3) and z (dims 1, 2) as torch.rot90 counts them, then the flips of dims 1, 2, 3, then the
swap of dims 2 and 3. The old form with a 2-tuple rotation means (0, rotate_y, rotate_z). The host folds a key into ONE signed axis
permutation, the code of include/mi355_unet3d.h (s0 | s1 << 2 | s2 << 4 | f0 << 6 | f1 << 7 | f2 << 8), so any key is one launch where
the chain of torch.rot90 / flip / transpose is up to seven passes.

  permute_data / reverse_permute_data     [C, D, H, W] or [N, C, D, H, W], elements of 1, 2 or 4 bytes, any extents; a bit copy
  permute_batch                           one key per sample of [N, C, D, H, W] (the keys must agree on the output extents)
  PermutationEnsemble                     mean over keys of reverse(activation(predictor(permute(x)))): per key one permute launch, the
                                          predictor, and one launch that undoes the permutation, applies the activation and folds the
                                          result into the fp32 mean
"""
import functools
import random

import torch

from . import _lib
from . import ops as _ops

_IDENTITY = ((0, 1, 2), (0, 0, 0))         # (source axis of each output axis, whether it runs backwards)


def _be(t, be=None):
    if be is not None:
        return be
    if t.device.type != "cuda":
        raise RuntimeError("3dunetcnn_amd.permute runs on an MI355X only (no CPU fallback)")
    return _ops.default_backend(t.device)


def _then(first, step):
    """The signed permutation `first` followed by `step`: output axis a of the result reads, through step, axis step.s[a] of first's output."""
    (s, f), (s2, f2) = first, step
    return tuple(s[s2[a]] for a in range(3)), tuple(f2[a] ^ f[s2[a]] for a in range(3))


def _flip(axis):
    return (0, 1, 2), tuple(int(a == axis) for a in range(3))


def _swap(p, q):
    s = [0, 1, 2]
    s[p], s[q] = q, p
    return tuple(s), (0, 0, 0)


def _quarter_turns(perm, k, p, q):
    """torch.rot90(k, dims=(p, q)) over spatial axes: one quarter turn is the swap of p and q followed by the flip of p."""
    for _ in range(int(k) % 4):
        perm = _then(_then(perm, _swap(p, q)), _flip(p))
    return perm


def _split(key):
    rotation, flip_x, flip_y, flip_z, transpose = key
    rotation = tuple(int(r) for r in rotation)
    if len(rotation) == 2:
        rotation = (0,) + rotation
    if len(rotation) != 3:
        raise ValueError(f"a key's rotation has 2 or 3 entries, not {len(rotation)}")
    return rotation, (bool(flip_x), bool(flip_y), bool(flip_z)), bool(transpose)


def _key_perm(key):
    (rx, ry, rz), flips, transpose = _split(key)
    perm = _quarter_turns(_IDENTITY, rx, 1, 2)
    perm = _quarter_turns(perm, ry, 0, 2)
    perm = _quarter_turns(perm, rz, 0, 1)
    for axis in range(3):
        if flips[axis]:
            perm = _then(perm, _flip(axis))
    if transpose:
        perm = _then(perm, _swap(1, 2))
    return perm


def _code(perm):
    s, f = perm
    return s[0] | s[1] << 2 | s[2] << 4 | f[0] << 6 | f[1] << 7 | f[2] << 8


def _inverse(perm):
    s, f = perm
    inv_s, inv_f = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        inv_s[s[a]], inv_f[s[a]] = a, f[a]
    return tuple(inv_s), tuple(inv_f)


def key_code(key):
    """The code (include/mi355_unet3d.h) of what permute_data does with `key`."""
    return _code(_key_perm(key))


def reverse_key_code(key):
    """The code of what reverse_permute_data does with `key`: the inverse of key_code(key)."""
    return _code(_inverse(_key_perm(key)))


@functools.lru_cache(maxsize=None)
def _sorted_keys():
    seen, keys = set(), []
    for rx in range(4):
        for ry in range(4):
            for rz in range(4):
                for fx in (0, 1):
                    for fy in (0, 1):
                        for fz in (0, 1):
                            key = ((rx, ry, rz), fx, fy, fz, 0)
                            code = key_code(key)
                            if code not in seen:
                                seen.add(code)
                                keys.append(key)
    assert len(keys) == 48
    return tuple(sorted(keys))


def generate_permutation_keys():
    """The set of 48 keys ((rotate_x, rotate_y, rotate_z), flip_x, flip_y, flip_z, 0), one per rotation / reflection of a volume: of
    the keys that give the same transform, the first in the order of the rotations, then the flips, each counted up from 0."""
    return set(_sorted_keys())


def random_permutation_key(generator=None):
    """One of the 48 keys, uniformly: drawn from `generator` (a CPU torch.Generator) or, without one, from Python's `random`."""
    keys = _sorted_keys()
    if generator is None:
        return random.choice(keys)
    return keys[int(torch.randint(len(keys), (1,), generator=generator))]


def reverse_permutation_key(key):
    """The key with every rotation count negated (a 2-tuple rotation becomes (0, -ry, -rz)); reverse_permute_data undoes the steps of
    `key` in the opposite order with these counts."""
    return tuple(-r for r in _split(key)[0]), key[1], key[2], key[3], key[4]


def _as_batch(data):
    if data.dim() not in (4, 5):
        raise ValueError(f"[C, D, H, W] or [N, C, D, H, W], not {tuple(data.shape)}")
    if data.element_size() not in (1, 2, 4):
        raise NotImplementedError(f"{data.dtype}: elements of 1, 2 or 4 bytes")
    x = data.detach()
    return (x if x.dim() == 5 else x[None]).contiguous()


def _run(data, code, _backend):
    be = _be(data, _backend)
    out = be.permute3d(_as_batch(data), [code])
    return out if data.dim() == 5 else out[0]


def permute_data(data, key, _backend=None):
    """data [C, D, H, W] or [N, C, D, H, W] permuted by `key`: a new tensor, one launch."""
    return _run(data, key_code(key), _backend)


def reverse_permute_data(data, key, _backend=None):
    """Undoes permute_data(., key): a new tensor, one launch."""
    return _run(data, reverse_key_code(key), _backend)


def _extents(code, dhw):
    return tuple(int(dhw[(code >> (2 * a)) & 3]) for a in range(3))


def permute_batch(x, keys, _backend=None):
    """x [N, C, D, H, W] with one key per sample; the keys must give every sample the same shape (any keys on a cube). One launch per
    _lib.PERMUTE_MAX_BATCH samples."""
    be = _be(x, _backend)
    keys = list(keys)
    if x.dim() != 5 or len(keys) != x.shape[0]:
        raise ValueError(f"{len(keys)} keys for a batch of shape {tuple(x.shape)}")
    codes = [key_code(k) for k in keys]
    shapes = {_extents(c, x.shape[2:]) for c in codes}
    if len(shapes) > 1:
        raise ValueError(f"the keys give samples of different shapes: {sorted(shapes)}")
    xb = _as_batch(x)
    cap = _lib.PERMUTE_MAX_BATCH
    outs = [be.permute3d(xb[i:i + cap], codes[i:i + cap]) for i in range(0, len(codes), cap)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def random_permutation_x_y(x_data, y_data, channel_axis=0, generator=None, _backend=None):
    """x_data and y_data ([C, D, H, W] with the channels at channel_axis) permuted by one random key."""
    key = random_permutation_key(generator)
    if channel_axis != 0:
        return [torch.moveaxis(permute_data(torch.moveaxis(data, channel_axis, 0), key, _backend), 0, channel_axis)
                for data in (x_data, y_data)]
    return permute_data(x_data, key, _backend), permute_data(y_data, key, _backend)


class PermutationEnsemble:
    """predictor -> a callable with the predictor's signature that returns the fp32 mean over `keys` of
    reverse_permute(activation(predictor(permute(x)))) in the extents of x [N, C, D, H, W].

    keys: "flips" (the 8 keys without rotation: the mirror ensemble), "all" (the 48) or an iterable of keys. activation: None | "sigmoid" |
    "softmax", applied to each prediction before the mean. A predictor that returns a tuple contributes its element 0. Usable as the
    `network` of HipSlidingWindowInferer. Per key: one permute launch, the predictor, one fold launch -- no pass for the activation, the
    sum or the division."""

    def __init__(self, predictor, keys="flips", activation=None, _backend=None):
        if isinstance(keys, str):
            if keys not in ("flips", "all"):
                raise ValueError(f"keys={keys!r}: 'flips', 'all' or an iterable of keys")
            keys = [k for k in _sorted_keys() if keys == "all" or k[0] == (0, 0, 0)]
        self.keys = [tuple(k) for k in keys]
        if not self.keys:
            raise ValueError("no keys")
        if activation not in (None, "none", "sigmoid", "softmax"):
            raise ValueError(f"activation={activation!r}: None, 'sigmoid' or 'softmax'")
        self.predictor, self.activation, self._backend = predictor, activation, _backend
        self.codes = [key_code(k) for k in self.keys]

    def __call__(self, x, *args, **kwargs):
        be = _be(x, self._backend)
        if x.dim() != 5:
            raise ValueError(f"[N, C, D, H, W], not {tuple(x.shape)}")
        xb = _as_batch(x)
        weight = 1.0 / len(self.codes)
        acc = None
        for code in self.codes:
            y = self.predictor(be.permute3d(xb, [code]), *args, **kwargs)
            if isinstance(y, (tuple, list)):
                y = y[0]
            if y.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                y = y.float()
            acc = be.unpermute_accumulate(y.detach().contiguous(), [code], acc, self.activation, weight, init=acc is None)
        return acc
