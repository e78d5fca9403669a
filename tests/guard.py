"""Guard bands: a software memory-safety check for the HIP kernels (no GPU sanitizer is available to this project).

  guarded(t)       a copy of ``t`` inside a larger uint8 allocation whose bytes outside the interior are all 0xFF: NaN when read
                   as fp32 / bf16 / fp64, -1 as int16 / int64, so one canary serves every dtype the library touches.  An
                   out-of-bounds READ whose value is used turns a result NaN (or changes it between a 0xFF and a 0x00 run);
                   an out-of-bounds WRITE damages a band, which ``check()`` reports by allocation site, side and distance.
  GuardedAlloc()   while active, torch.empty / empty_like / zeros / zeros_like / full / full_like calls that name the device
                   and pass nothing but shape, dtype and device return guarded tensors; ``empty*`` interiors are poisoned too.
  LibProxy(lib)    records which C ABI entry points ran and where each of their pointer arguments pointed; in ``refuse``
                   mode no launching entry point can be reached at all.

The module is device-agnostic (its own logic is tested on the CPU, tests/test_cpu.py) and is not a conftest."""
import bisect
import ctypes
import os
import re
import traceback

import torch

CANARY = 0xFF
MIN_BAND = 4096            # elements on each side, at least
ALIGN = 512                # the interior's byte alignment (torch's caching allocator gives the same)

_REG = []                  # every live guarded buffer, until release()
_VERSION = [0]             # bumped whenever _REG changes (LibProxy rebuilds its interval table)
_ORIG = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like")}
_HERE = os.path.abspath(__file__)


class _Buf:
    __slots__ = ("site", "whole", "off", "nbytes", "dtype", "shape", "canary")

    def interior_ptr(self):
        return self.whole.data_ptr() + self.off


def _site():
    """the allocation site: the innermost frame inside the package, else the innermost one outside this module"""
    stack = traceback.extract_stack()[:-2][::-1]
    for fr in stack:
        if "smilecode_amd" in fr.filename:
            return "%s:%d %s" % (os.path.basename(fr.filename), fr.lineno, fr.name)
    for fr in stack:
        if os.path.abspath(fr.filename) != _HERE:
            return "%s:%d %s" % (os.path.basename(fr.filename), fr.lineno, fr.name)
    return "?"


def band_elems(shape, band=None):
    """elements of band on each side: >= MIN_BAND and >= one outermost slice (numel / shape[0]; one z-plane,
    numel / (shape[0] * shape[1]), for 5-D tensors), so that an off-by-one in x, y or z lands inside it"""
    if band is not None:
        return int(band)
    n = 1
    for s in shape:
        n *= int(s)
    sl = 0
    if len(shape) == 5 and shape[0] * shape[1] > 0:
        sl = n // (int(shape[0]) * int(shape[1]))
    elif len(shape) >= 1 and shape[0] > 0:
        sl = n // int(shape[0])
    return max(MIN_BAND, sl)


def _alloc(shape, dtype, device, band, canary, interior):
    """interior: None = poisoned with the canary, else the byte the interior is filled with (0 for zeros)"""
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = n * item
    bb = -(-band_elems(shape, band) * item // ALIGN) * ALIGN           # band bytes, rounded up to the alignment
    whole = _ORIG["empty"](bb + nbytes + bb + ALIGN, dtype=torch.uint8, device=device)
    off = bb + (-(whole.data_ptr() + bb)) % ALIGN
    whole.fill_(canary)
    if interior is not None and nbytes:
        whole[off:off + nbytes].fill_(interior)
    b = _Buf()
    b.site, b.whole, b.off, b.nbytes, b.dtype, b.shape, b.canary = _site(), whole, off, nbytes, dtype, shape, canary
    _REG.append(b)
    _VERSION[0] += 1
    return whole[off:off + nbytes].view(dtype).view(shape)


def guarded(t, band=None, canary=CANARY):
    """a tensor equal to ``t`` (same dtype, shape and device, contiguous, detached) between two bands of ``canary`` bytes"""
    g = _alloc(t.shape, t.dtype, t.device, band, canary, 0)
    g.copy_(t.detach())
    return g


def guarded_empty(shape, dtype, device, band=None, canary=CANARY):
    """an output buffer between bands whose interior is poisoned with the canary too (what torch.empty gives under GuardedAlloc)"""
    if isinstance(shape, int):
        shape = (shape,)
    return _alloc(shape, dtype, device, band, canary, None)


def guarded_bytes(nbytes, device, canary=CANARY, band=4 * MIN_BAND):
    """a workspace of exactly ``nbytes`` bytes (uint8, poisoned): every byte behind it is band, also the tail up to the next
    multiple of 4 where a *_ws_bytes result is not one"""
    return _alloc((int(nbytes),), torch.uint8, device, band, canary, None)


def release():
    """forget every guarded buffer (after the last check of a test)"""
    del _REG[:]
    _VERSION[0] += 1


def live():
    return list(_REG)


def check():
    """-> the damaged bands, one dict each: site, dtype, interior elements, side ('below' | 'above'), damaged bytes, and the
    distance of the nearest damaged byte from the interior in bytes and in elements (1 = adjacent).  Re-arms the bands."""
    out = []
    for b in _REG:
        lo, hi = b.whole[:b.off], b.whole[b.off + b.nbytes:]
        if int((lo != b.canary).sum()) + int((hi != b.canary).sum()) == 0:
            continue
        item = torch.empty((), dtype=b.dtype).element_size()
        for side, band in (("below", lo), ("above", hi)):
            bad = torch.nonzero(band != b.canary).flatten()
            if bad.numel() == 0:
                continue
            near = (band.numel() - int(bad.max())) if side == "below" else int(bad.min()) + 1
            out.append({"site": b.site, "dtype": str(b.dtype), "interior": b.nbytes // item, "shape": b.shape, "side": side,
                        "bytes": int(bad.numel()), "distance_bytes": near, "distance": -(-near // item)})
            band.fill_(b.canary)
    return out


def describe(bands):
    return "damaged guard bands:\n" + "\n".join(
        "  %(site)s %(dtype)s %(shape)s: %(bytes)d bytes %(side)s the interior, nearest %(distance)d elements "
        "(%(distance_bytes)d bytes) away" % d for d in bands)


def assert_intact(what=""):
    bands = check()
    assert not bands, what + ": " + describe(bands)


# ------------------------------------------------------------------------------------------------ torch allocation calls
def _norm_shape(a):
    if len(a) == 1 and isinstance(a[0], (tuple, list, torch.Size)):
        return tuple(a[0])
    return tuple(a)


class GuardedAlloc:
    """with GuardedAlloc(): every plain allocation on ``device_type`` is guarded (see the module docstring).  ``canary`` /
    ``poison``: the byte of the bands and of ``empty*`` interiors (0x00 for the second run of a comparison)."""

    def __init__(self, device_type="cuda", canary=CANARY, band=None):
        self.device_type, self.canary, self.band = device_type, canary, band

    def _mine(self, dv, k, allowed=("dtype", "device")):
        return dv is not None and torch.device(dv).type == self.device_type and not (k.keys() - set(allowed))

    def _make(self, shape, dtype, device, interior):
        return _alloc(shape, dtype or torch.get_default_dtype(), device, self.band, self.canary, interior)

    def __enter__(self):
        o = _ORIG

        def empty(*a, **k):
            if self._mine(k.get("device"), k) and a:
                return self._make(_norm_shape(a), k.get("dtype"), k["device"], None)
            return o["empty"](*a, **k)

        def zeros(*a, **k):
            if self._mine(k.get("device"), k) and a:
                return self._make(_norm_shape(a), k.get("dtype"), k["device"], 0)
            return o["zeros"](*a, **k)

        def full(*a, **k):
            if self._mine(k.get("device"), k) and len(a) == 2 and k.get("dtype") is not None:
                t = self._make(_norm_shape(a[:1]), k["dtype"], k["device"], 0)
                return t.fill_(a[1])
            return o["full"](*a, **k)

        def _like(t, k):
            return torch.is_tensor(t) and t.device.type == self.device_type and not k and t.is_contiguous()

        def empty_like(t, **k):
            return self._make(t.shape, t.dtype, t.device, None) if _like(t, k) else o["empty_like"](t, **k)

        def zeros_like(t, **k):
            return self._make(t.shape, t.dtype, t.device, 0) if _like(t, k) else o["zeros_like"](t, **k)

        def full_like(t, v, **k):
            return self._make(t.shape, t.dtype, t.device, 0).fill_(v) if _like(t, k) else o["full_like"](t, v, **k)

        for n, f in (("empty", empty), ("zeros", zeros), ("full", full), ("empty_like", empty_like),
                     ("zeros_like", zeros_like), ("full_like", full_like)):
            setattr(torch, n, f)
        return self

    def __exit__(self, *exc):
        for n, f in _ORIG.items():
            setattr(torch, n, f)
        return False


# ------------------------------------------------------------------------------------------------ the library proxy
_QUERY = re.compile(r"(_bytes(_f64)?$|_family|_ok$|_operands$|_version$|_strerror$)")
_NOT_LAUNCHING = re.compile(r"(_bytes(_f64)?$|_family|_ok$|_operands$|_partial_rows$|_version$|_strerror$|_step_ctx_(create|destroy)$)")


def is_query(name):
    """the entry points ``refuse`` mode lets through: pure host-side queries"""
    return bool(_QUERY.search(name))


def is_launching(name):
    """the entry points the coverage test wants seen: everything but the pure queries and the step-context constructor pair"""
    return not _NOT_LAUNCHING.search(name)


def _cuda_segments():
    if not torch.cuda.is_available():
        return []
    return [(s["address"], s["total_size"]) for s in torch.cuda.memory_snapshot()]


class LibProxy:
    """Stands in for the ctypes library object (``monkeypatch.setattr(_lib, "_lib", LibProxy(_lib.load()))``): forwards every
    attribute; for the names of ``signatures`` it records (name, [class of each c_void_p argument]) in ``records`` with
    class = 'null' | 'guarded' (start or inside of a registered guarded interior) | 'torch' (inside a device segment of torch's
    allocator, but not guarded) | 'other' (stream and step-context handles, host arrays)."""

    def __init__(self, real, signatures=None, segments=_cuda_segments, refuse=False):
        if signatures is None:
            from smilecode_amd import _lib
            signatures = _lib.SIGNATURES
        d = self.__dict__
        d["_real"], d["_sig"], d["_segments"], d["refuse"] = real, signatures, segments, refuse
        d["records"], d["_iv"], d["_iv_version"], d["_seg"], d["_other"] = [], ([], []), -1, None, set()
        d["log_args"], d["calls"] = False, []          # log_args: also keep (name, args) of every recorded call in ``calls``

    def __setattr__(self, name, value):
        if name in ("refuse", "log_args"):
            self.__dict__[name] = bool(value)
        else:
            setattr(self._real, name, value)

    def _intervals(self):
        if self._iv_version != _VERSION[0]:
            iv = sorted((b.interior_ptr(), b.interior_ptr() + max(b.nbytes, 1)) for b in _REG)
            self.__dict__["_iv"] = ([s for s, _ in iv], [e for _, e in iv])
            self.__dict__["_iv_version"] = _VERSION[0]
        return self._iv

    def classify(self, v):
        if v is None:
            return "null"
        if isinstance(v, ctypes.c_void_p):
            v = v.value
            if v is None:
                return "null"
        if not isinstance(v, int):
            return "other"
        if v == 0:
            return "null"
        starts, ends = self._intervals()
        i = bisect.bisect_right(starts, v) - 1
        if i >= 0 and v < ends[i]:
            return "guarded"
        if v in self._other:                  # (stream and step-context handles come by with every call)
            return "other"
        for again in (False, True):
            if self._seg is None or again:
                self.__dict__["_seg"] = list(self._segments())
            if any(a <= v < a + n for a, n in self._seg):
                return "torch"
        self._other.add(v)
        return "other"

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = self._sig.get(name)
        if sig is None:
            return fn
        ptr_at = [i for i, t in enumerate(sig[1]) if t is ctypes.c_void_p]

        def call(*a):
            if self.refuse and not is_query(name):
                raise AssertionError("%s reached with the proxy in refuse mode: a host check is missing" % name)
            self.records.append((name, [self.classify(a[i]) for i in ptr_at if i < len(a)]))
            if self.log_args:
                self.calls.append((name, a))
            return fn(*a)
        call.__name__ = name
        return call

    def names(self):
        return {n for n, _ in self.records}
