"""TEST INFRASTRUCTURE: hostile memory for the ops under test (tests/test_scratch_emu.py, tests/test_scratch_gpu.py).

The op tests vary shapes, types and routes; this module varies THE MEMORY the kernels are handed. Under `guarded(be, fill)`:

* `be.ws(nbytes)` returns a 1-D float32 view of exactly ceil(nbytes / 4) elements (ops.py passes `ws.numel() * 4` on, so the library's
  MI355_EWORKSPACE check runs at the boundary of what its own size query answered) instead of the >= 1 MiB grow-only buffer;
* `torch.empty` / `torch.empty_like` as called by the package's modules (PACKAGE_MODULES: their `torch` global is a thin proxy for the
  duration of the context, everything else delegated) return a view of exactly the requested shape -- records, `empty_act`, logits,
  gradients, packs, label maps. The test's own code and the oracle keep the real torch;
* every such view lies inside a larger buffer the harness owns: GUARD bytes (64 KiB) of GUARD_BYTE on each side, the payload on a
  512-byte boundary (what torch's device allocator gives: routes that choose vector paths from pointer alignment keep their route),
  the payload pre-filled with the poison `fill`: QNAN (0x7fc00000) or ONES (0xffffffff: NaN as fp32, -1 as int32); 16-bit types get
  their own NaN / all-ones, 8-bit types the top byte (0x7f / 0xff);
* `op_cases.OUT_FILL` is set, so the outputs the case tables pre-make on the host are poisoned as well;
* on leaving the context every guard band is compared bytewise; a mismatch raises GuardViolated with the allocation's shape, dtype,
  call site (two frames) and the first / last dirty byte offset.

`hold(be, fn, ...)` is what a test row runs: clean, clean again (NotReproducible if the bits differ: a finding of its own), then
guarded once per fill (PoisonDiffers if any tensor handed to `rel_err` / `stored_ok`, or returned by the case, is not bit-identical
to the clean run); the case's own assertions run inside `fn` each time, so NaN in a result fails them.

64 KiB is larger than any single partial table of the library at the test shapes; an overrun up to that size lands in memory the
test owns. Out-of-bounds READS are invisible to a guard band (the emulator under a host sanitizer is the tool for those).
"""
import collections
import contextlib
import importlib
import os
import traceback

import torch

import act_storage_cases as S
import op_cases as C
from oracle import torch_ops as O

GUARD = 64 << 10
ALIGN = 512
GUARD_BYTE = 0xA5
QNAN = C.QNAN
ONES = C.ONES
PACKAGE_MODULES = ("ops", "unet", "dynunet", "engine", "losses", "prepost", "augment", "inferer")
_HERE = os.path.abspath(__file__)


class GuardViolated(AssertionError):
    """An op wrote outside what it was handed."""


class NotReproducible(AssertionError):
    """Two clean runs of a case differ bit for bit (nothing to do with poison)."""


class PoisonDiffers(AssertionError):
    """The guarded run differs from the clean run: something read memory it was expected to write first, or accumulated into it."""


class _Alloc:
    __slots__ = ("raw", "off", "nbytes", "shape", "dtype", "site")


class _TorchProxy:
    """`torch` as the package's modules see it under the harness: empty / empty_like on the backend's device are guarded."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        g = self._guard
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        device = torch.device(kw.get("device") or "cpu")
        if set(kw) - {"dtype", "device"} or device.type != g.device.type:
            return torch.empty(*size, **kw)
        return g.alloc(tuple(int(s) for s in size), kw.get("dtype") or torch.get_default_dtype(), device)

    def empty_like(self, t, **kw):
        g = self._guard
        device = torch.device(kw.get("device") or t.device)
        if set(kw) - {"dtype", "device"} or device.type != g.device.type or not t.is_contiguous():
            return torch.empty_like(t, **kw)
        return g.alloc(tuple(t.shape), kw.get("dtype") or t.dtype, device)


class Guard:
    def __init__(self, be, fill):
        self.device = torch.device(be.device)
        self.fill = fill
        self.allocs = []
        self.torch = _TorchProxy(self)

    def alloc(self, shape, dtype, device=None):
        device = self.device if device is None else device
        nbytes = dtype.itemsize
        for s in shape:
            nbytes *= s
        raw = torch.empty(GUARD + ALIGN + nbytes + GUARD, dtype=torch.uint8, device=device)
        off = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
        raw.fill_(GUARD_BYTE)
        payload = raw[off:off + nbytes]
        C.poison_bytes(payload, dtype, self.fill)
        a = _Alloc()
        a.raw, a.off, a.nbytes, a.shape, a.dtype = raw, off, nbytes, shape, dtype
        a.site = [f"{os.path.relpath(f.filename, os.path.dirname(os.path.dirname(_HERE)))}:{f.lineno} {f.name}"
                  for f in traceback.extract_stack(limit=8) if os.path.abspath(f.filename) != _HERE][-2:]
        self.allocs.append(a)
        out = payload.view(dtype).view(shape) if nbytes else torch.empty(shape, dtype=dtype, device=device)
        assert out.data_ptr() % ALIGN == 0 or not nbytes
        return out

    def ws(self, nbytes):
        return self.alloc(((int(nbytes) + 3) // 4,), torch.float32)

    def violations(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        out = []
        for a in self.allocs:
            for name, band, base in (("before", a.raw[:a.off], -a.off), ("after", a.raw[a.off + a.nbytes:], 0)):
                bad = band != GUARD_BYTE
                if bool(bad.any()):
                    idx = bad.nonzero().flatten()
                    out.append(f"{tuple(a.shape)} {a.dtype} allocated at {' <- '.join(reversed(a.site))}: {int(idx.numel())} guard bytes {name} the "
                               f"payload were written, first / last byte offset {int(idx[0]) + base} / {int(idx[-1]) + base} "
                               f"(relative to the payload's {'start' if base else 'end'})")
        return out

    def check(self):
        bad = self.violations()
        if bad:
            raise GuardViolated("guard band violated:\n  " + "\n  ".join(bad))


@contextlib.contextmanager
def guarded(be, fill=QNAN, modules=()):
    """See the module docstring. `be`: a Backend (the session's shared one: every patch is undone on exit). `modules`: further modules
    whose `torch` global gets the proxy (the harness self-test passes its own)."""
    g = Guard(be, fill)
    mods = [importlib.import_module("3dunetcnn_amd." + m) for m in PACKAGE_MODULES] + list(modules)
    mods = [m for m in mods if m.__dict__.get("torch") is torch]
    had_ws = "ws" in be.__dict__
    saved_ws, saved_streams, saved_fill = be.__dict__.get("ws"), dict(be._ws_by_stream), C.OUT_FILL
    try:
        for m in mods:
            m.torch = g.torch
        be.ws = g.ws
        C.OUT_FILL = fill
        try:
            yield g
        except Exception as e:
            # the case failed first (NaN from an overrun neighbour, say): a violated guard is the likelier cause, so it is reported
            # with the case's failure chained to it rather than lost
            bad = g.violations()
            if bad:
                raise GuardViolated("guard band violated (and the case then failed: see the chained exception):\n  " + "\n  ".join(bad)) from e
            raise
        g.check()
    finally:
        C.OUT_FILL = saved_fill
        if had_ws:
            be.ws = saved_ws
        else:
            del be.__dict__["ws"]
        be._ws_by_stream.clear()
        be._ws_by_stream.update(saved_streams)
        for m in mods:
            m.torch = torch


def _tensors(r):
    if isinstance(r, torch.Tensor):
        yield r
    elif isinstance(r, dict):
        for k in sorted(r, key=str):
            yield from _tensors(r[k])
    elif isinstance(r, (tuple, list)):
        for v in r:
            yield from _tensors(v)
    elif hasattr(r, "tensor") and hasattr(r, "buf"):          # ops.Act
        yield r.tensor()


def _digest(t):
    return O.tensor_digest(t.detach().reshape(-1)) + str(tuple(t.shape))        # (tensor_digest views bytes: no 0-dim tensors)


@contextlib.contextmanager
def recording(log):
    """Appends the digest of every kernel result a case hands to op_cases.rel_err (first argument) or act_storage_cases.stored_ok
    (both) to `log`; both are looked up through their modules at call time by every case table."""
    rel_err, stored_ok = C.rel_err, S.stored_ok

    def rec_rel_err(a, b):
        log.append(_digest(a))
        return rel_err(a, b)

    def rec_stored_ok(a16, a32):
        log.append(_digest(a16.tensor()))
        log.append(_digest(a32.tensor()))
        return stored_ok(a16, a32)
    C.rel_err, S.stored_ok = rec_rel_err, rec_stored_ok
    try:
        yield log
    finally:
        C.rel_err, S.stored_ok = rel_err, stored_ok


def run_recorded(fn):
    log = []
    with recording(log):
        r = fn()
    log.extend(_digest(t) for t in _tensors(r))
    return r, log


Held = collections.namedtuple("Held", "results allocations")      # results compared bit for bit; guarded allocations of the poorest run


def hold(be, fn, fills=(QNAN,), modules=()):
    """Runs the case `fn()` clean, clean again and guarded once per fill. `fn` holds the case's own assertions. Returns Held."""
    _, clean = run_recorded(fn)
    _, again = run_recorded(fn)
    assert clean, "the case compares nothing: no rel_err / stored_ok call and no tensor returned"
    if clean != again:
        raise NotReproducible(f"two clean runs differ in results {[i for i, (a, b) in enumerate(zip(clean, again)) if a != b]} of {len(clean)}")
    allocations = []
    for fill in fills:
        with guarded(be, fill, modules) as g:
            _, dirty = run_recorded(fn)
        allocations.append(len(g.allocs))
        # (the guards were checked on leaving the context: an overrun explains a differing result, not the other way round)
        if dirty != clean:
            raise PoisonDiffers(f"with scratch, records and outputs pre-filled with {fill:#010x}, results "
                                f"{[i for i, (a, b) in enumerate(zip(clean, dirty)) if a != b] or 'count'} of {len(clean)} differ from the clean run")
    return Held(len(clean), min(allocations))


@contextlib.contextmanager
def configured(be, precision=None, env=None, storage=None, **attrs):
    """Backend attributes (winograd, wino_form, wgrad_form, WINO_MIN_VOXELS, fused_stats, ...), precision mode, environment switches
    of the library and the 16-bit storage type of act_storage_cases for one case; everything restored."""
    missing = object()
    saved = {k: be.__dict__.get(k, missing) for k in attrs}
    saved_env = {k: os.environ.get(k) for k in (env or {})}
    saved_prec = be.precision
    st = S.storage_type(storage) if storage is not None else contextlib.nullcontext()
    try:
        for k, v in attrs.items():
            setattr(be, k, v)
        os.environ.update(env or {})
        if precision is not None:
            be.set_precision(precision)
        with st:
            yield be
    finally:
        be.precision = saved_prec
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        for k, v in saved.items():
            if v is missing:
                be.__dict__.pop(k, None)
            else:
                setattr(be, k, v)
