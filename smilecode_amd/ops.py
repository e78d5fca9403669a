"""Torch-facing operators of the ModeT hot path: thin autograd wrappers over libmodet_hip.so.

PyTorch is plumbing here (device memory from the caching allocator, the current HIP
stream, autograd's tape); every arithmetic kernel is hand-written HIP behind the C ABI of
include/modet_hip.h.  Activations are channels-last ``(B, D, H, W, C)`` fp32 (bf16 inside the ConvInsBlock chains when the model is built with
``act_dtype=torch.bfloat16``, see the end of this file), contiguous.
There is no eager / CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
from typing import Callable, NamedTuple

import torch
from torch.autograd import Function

from . import _lib

LRELU_SLOPE = 0.1


def _L():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(fn, *args):
    """every library call: a failure names the entry point that was entered"""
    _lib.check(fn(*args), fn.__name__)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("smilecode_amd: tensor must live on the GPU (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"smilecode_amd: expected float32, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError("smilecode_amd: tensor must be contiguous")


def _p(t):
    return None if t is None else t.data_ptr()


def _same_shape(op, name, t, want, of=""):
    """refuse a tensor whose shape the kernel would otherwise infer from another argument (None passes: an absent operand)"""
    if t is not None and tuple(t.shape) != tuple(want):
        raise RuntimeError(f"{op}: {name} {tuple(t.shape)} does not match {tuple(want)}" + (f" ({of})" if of else ""))


def _rank5(op, name, t):
    """the kernels take channels-last (B,D,H,W,C) tensors: refuse another rank by name instead of failing to unpack the shape"""
    if t.dim() != 5:
        raise RuntimeError(f"{op}: {name} must be a channels-last (B,D,H,W,C) tensor, got {tuple(t.shape)}")


def _amax_arg(op, amax):
    """a gradient-maximum buffer is read (and by the InstanceNorm backward written) over all its AMAX_FLOATS floats"""
    if amax is not None and amax.numel() < AMAX_FLOATS:
        raise RuntimeError(f"{op}: amax {tuple(amax.shape)} holds fewer than the {AMAX_FLOATS} floats of a gradient-maximum buffer")


def _conv_args(op, x, w, b):
    """x (B,D,H,W,Cin), w (Cout,Cin,3,3,3), b (Cout,) or None"""
    if x.dim() != 5 or w.dim() != 5:
        raise RuntimeError(f"{op}: expects a channels-last (B,D,H,W,Cin) input and a (Cout,Cin,3,3,3) weight, got "
                           f"{tuple(x.shape)} and {tuple(w.shape)}")
    _same_shape(op, "weight", w, (w.shape[0], x.shape[-1], 3, 3, 3), f"input {tuple(x.shape)}")
    _same_shape(op, "bias", b, (w.shape[0],), f"weight {tuple(w.shape)}")


def _ws(nbytes, like):
    return torch.empty((int(nbytes) + 3) // 4 + 1, dtype=torch.float32, device=like.device)


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's live roofline leg).
    ``select`` = None times every tagged launch, or a set of tags to time only those."""

    def __init__(self, select=None):
        self.select = select
        self.records = []          # (tag, flops, bytes, start_event, end_event)

    def summary(self):
        """tag -> dict(calls, ms, flops, bytes); synchronises the events it reads"""
        out = {}
        for tag, fl, by, e0, e1 in self.records:
            e1.synchronize()
            d = out.setdefault(tag, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


_TIMER = None


def set_kernel_timer(timer):
    """install / remove (None) the KernelTimer consulted by every launch below"""
    global _TIMER
    _TIMER = timer


class _Guard:
    """make x's device current for the launch (autograd worker threads, multi-GPU hosts); when a
    KernelTimer is installed, bracket the launch with HIP events on the current stream."""

    def __init__(self, t, tag=None, flops=0.0, nbytes=0.0):
        self.idx = t.device.index
        self.prev = None
        self.tag, self.flops, self.nbytes = tag, flops, nbytes
        self.e0 = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)
        tm = _TIMER
        if tm is not None and self.tag is not None and (tm.select is None or self.tag in tm.select):
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if self.e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _TIMER.records.append((self.tag, self.flops, self.nbytes, self.e0, e1))
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


class _Roctx:
    """roctx ranges around the pyramid levels / phases of a step (SURVEY.md §5 tracing row): visible in
    ``rocprofv3 --marker-trace`` timelines.  Off unless MODET_ROCTX=1 (two ctypes calls per range otherwise wasted)."""

    def __init__(self):
        import ctypes
        import os
        self.lib = None
        if os.environ.get("MODET_ROCTX") == "1":
            for name in ("libroctx64.so", "/opt/rocm/lib/libroctx64.so", "librocprofiler-sdk-roctx.so"):
                try:
                    self.lib = ctypes.CDLL(name)
                    self.lib.roctxRangePushA.argtypes = [ctypes.c_char_p]
                    break
                except OSError:
                    continue

    def push(self, name):
        if self.lib is not None:
            self.lib.roctxRangePushA(name.encode())

    def pop(self):
        if self.lib is not None:
            self.lib.roctxRangePop()


_ROCTX = None


class trace_range:
    """``with ops.trace_range("level3"):`` -- a roctx range when MODET_ROCTX=1, nothing otherwise"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _ROCTX
        if _ROCTX is None:
            _ROCTX = _Roctx()
        _ROCTX.push(self.name)

    def __exit__(self, *a):
        _ROCTX.pop()


_FAM_CACHE = {}
_FAM_SUFFIX = ("", "@split", "@x3", "@direct", "@tr", "@q")     # by family (include/modet_hip.h, modet_conv3d_kernel_family_v)
_FAM_BF16X3_FWD = (1, 2, 5)     # forward kernels on bf16 pieces: fused InstanceNorm statistics cost them nothing
_FAM_F16_DGRAD = (2, 5)         # data-gradient kernels with a two-f16-piece form, which takes max |d_y|
_FAM_F16_FORM = (2, 4, 5)       # every family with a two-f16-piece form (4: the transpose-read weight gradient)


def _conv_tag(kind, x_shape, Cin, Cout, variant=0, f16=None):
    """KernelTimer tag of a conv launch: 'conv_fwd[8->8]@x3' names the kernel family that runs this shape (exact-f32
    MFMA: no suffix; tiled bf16x3: @split; z-marching bf16x3: @x3; small-volume direct MFMA: @direct; transpose-read weight
    gradient: @tr) -- only evaluated while a timer is installed.  ``variant`` = what the launch fuses (it changes the routing,
    include/modet_hip.h modet_conv3d_kernel_family_v): 0 plain, 1 LeakyReLU, 2 normalised input, 3 statistics.  '@x3h': the
    z-marching kernel on two f16 pieces (three products per fp32 product instead of six) -- every forward launch, and the
    backward launches that were given max |d_y| (f16=True)."""
    if _TIMER is None:
        return None
    f16 = (kind == "fwd") if f16 is None else bool(f16)
    key = (kind, tuple(x_shape[:4]), Cin, Cout, variant, f16)
    t = _FAM_CACHE.get(key)
    if t is None:
        B, D, H, W = x_shape[:4]
        fam = _L().modet_conv3d_kernel_family_v(B, D, H, W, Cin, Cout, {"fwd": 0, "dgrad": 1, "wgrad": 2}[kind], variant)
        arrow = f"{Cout}->{Cin}" if kind == "dgrad" else f"{Cin}->{Cout}"
        half = f16 and D * H * W < (1 << 24) and fam in _FAM_F16_FORM
        t = _FAM_CACHE[key] = f"conv_{kind}[{arrow}]{_FAM_SUFFIX[fam]}" + ("h" if half else "")
    return t


def _conv16_tag(kind, x_shape, Cin, Cout, x_bf16):
    """the same for the bf16-storage entry points: 'conv_bf16_fwd[8->8]@x3' = the one-piece z-marching kernel"""
    if _TIMER is None:
        return None
    key = ("b16" + kind, tuple(x_shape[:4]), Cin, Cout, bool(x_bf16))
    t = _FAM_CACHE.get(key)
    if t is None:
        B, D, H, W = x_shape[:4]
        fam = _L().modet_conv3d_bf16_kernel_family(B, D, H, W, Cin, Cout, {"fwd": 0, "dgrad": 1, "wgrad": 2}[kind], int(x_bf16))
        arrow = f"{Cout}->{Cin}" if kind == "dgrad" else f"{Cin}->{Cout}"
        t = _FAM_CACHE[key] = f"conv_bf16_{kind}[{arrow}]" + ("@x3" if fam == 2 else "")
    return t


# ------------------------------------------------------------------------------------------------ raw calls
def _conv_fwd(x, w, b, step, bounded=False, act=False, norm=None, want_stats=False):
    """THE forward conv launch (arguments already checked): output, workspace, statistics buffer, tag and the one library call.
    bounded: x is inside the f16 forms' range; act: fused LeakyReLU; norm = (mean, rstd): x is raw, normalised while staged;
    want_stats: InstanceNorm partial statistics from the epilogue.  Returns (y, stats or None)."""
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    L = _L()
    y = torch.empty((B, D, H, W, Cout), dtype=torch.float32, device=x.device)
    nb = L.modet_conv3d_ws_bytes(Cin, Cout)
    ws = _ws(nb, x)
    sb = (L.modet_conv3d_normin_stats_bytes if norm else L.modet_conv3d_stats_bytes)(B, D, H, W, Cin, Cout) if want_stats else 0
    # (a normalised-input launch goes without statistics where the configuration has none; the statistics launch does not)
    stats = torch.empty(sb // 4, dtype=torch.float32, device=x.device) if sb > 0 or (want_stats and not norm) else None
    n = float(B) * D * H * W
    variant = 2 if norm else (3 if want_stats else int(bool(act)))
    out, dims = (_p(w), _p(b), _p(y), _p(ws), nb), (B, D, H, W, Cin, Cout)
    with _Guard(x, _conv_tag("fwd", x.shape, Cin, Cout, variant, f16=bool(bounded or norm)), 54.0 * Cin * Cout * n, 4.0 * n * (Cin + Cout)):
        if norm:
            _call(L.modet_conv3d_fwd_normin, _p(x), *map(_p, norm), *out, _p(stats), sb, *dims, _stream(), _h(step))
        elif want_stats:
            fn = L.modet_conv3d_fwd_stats_bounded if bounded else L.modet_conv3d_fwd_stats
            _call(fn, _p(x), *out, _p(stats), sb, *dims, _stream(), _h(step))
        else:
            fn = L.modet_conv3d_fwd_bounded if bounded else L.modet_conv3d_fwd
            _call(fn, _p(x), *out, *dims, int(act), _stream(), _h(step))
    return y, stats


def conv3d_forward(x, w, b, act, step=None, x_act=False):
    """x_act: the caller's word that x is an activation inside the f16 forms' range (include/modet_hip.h, "TWO f16 PIECES":
    |x| < 4 094) -> the *_bounded entry point, half the matrix work; without it the launch makes no assumption about x (three
    bf16 pieces: fp32's range), as nn.Conv3d makes none"""
    _chk(x, w, b)
    _rank5("conv3d", "the input", x)
    step = step if step is not None else current_step()
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, Cin, 3, 3, 3):
        raise RuntimeError(f"conv3d: weight {tuple(w.shape)} does not match input channels {Cin}")
    _same_shape("conv3d", "bias", b, (Cout,), f"weight {tuple(w.shape)}")
    return _conv_fwd(x, w, b, step, bounded=x_act, act=act)[0]


def instnorm_stats(x_raw, stats=None, eps=1e-5):
    """per-(sample, channel) mean / rstd of a raw conv output, without the apply pass: from the conv epilogue's partial
    statistics when given, else by one statistics pass over x_raw"""
    _chk(x_raw)
    with _Guard(x_raw, "instnorm_stats", 2.0 * x_raw.numel(), 0.0 if stats is not None else 4.0 * x_raw.numel()):
        return _in_stats(x_raw, stats, eps)


# ---- the fp32 InstanceNorm launches (arguments already checked), one function per library call as _conv_fwd.
# ``stats`` = the producing conv's partial statistics, None = one pass more over x.
def _in_dims(x):
    """(B, V, C) of a channels-last tensor and fresh (mean, rstd) buffers of its B * C instances"""
    B, C = x.shape[0], x.shape[-1]
    mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
    return B, x.numel() // (B * C), C, mean, torch.empty_like(mean)


def _in_stats(x, stats, eps, pass_x=False):
    """THE statistics-only launch -> (mean, rstd), inside the caller's bracket (the pool node times it with its apply pass).
    With stats the kernel never reads x (csrc/norm_act.hip); pass_x hands its address over all the same, as the pool node has."""
    B, V, C, mean, rstd = _in_dims(x)
    L = _L()
    if stats is not None:
        _call(L.modet_instnorm_stats, _p(x) if pass_x else None, _p(mean), _p(rstd), _p(stats), stats.numel() * 4, None, 0, B, V, C,
              eps, _stream())
    else:
        nb = L.modet_instnorm_ws_bytes(B, V, C)
        ws = _ws(nb, x)
        _call(L.modet_instnorm_stats, _p(x), _p(mean), _p(rstd), None, 0, _p(ws), nb, B, V, C, eps, _stream())
    return mean, rstd


def _in_fwd(x, stats, eps):
    """THE InstanceNorm + LeakyReLU forward launch -> (y, mean, rstd)"""
    B, V, C, mean, rstd = _in_dims(x)
    y = torch.empty_like(x)
    L = _L()
    with _Guard(x, "instnorm_lrelu_fwd", 8.0 * x.numel(), 8.0 * x.numel()):
        if stats is not None:
            _call(L.modet_instnorm_lrelu_fwd_stats, _p(x), _p(y), _p(mean), _p(rstd), _p(stats), stats.numel() * 4, B, V, C, eps,
                  _stream())
        else:
            nb = L.modet_instnorm_ws_bytes(B, V, C)
            ws = _ws(nb, x)
            _call(L.modet_instnorm_lrelu_fwd, _p(x), _p(y), _p(mean), _p(rstd), _p(ws), nb, B, V, C, eps, _stream())
    return y, mean, rstd


def _in_bwd(dy, x, mean, rstd):
    """THE InstanceNorm + LeakyReLU backward launch -> d_x, tagged with the fresh buffer the kernel left max |d_x| in (_new_amax)"""
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // (B * C)
    dx = torch.empty_like(x)
    amax = _new_amax(x)
    L = _L()
    nb = L.modet_instnorm_ws_bytes(B, V, C)
    ws = _ws(nb, x)
    with _Guard(x, "instnorm_lrelu_bwd", 14.0 * x.numel(), 12.0 * x.numel()):
        _call(L.modet_instnorm_lrelu_bwd_amax, _p(dy), _p(x), _p(mean), _p(rstd), _p(dx), _p(ws), nb, B, V, C, _p(amax), _stream())
    return _tag_amax(dx, amax)


def conv3d_forward_normin(x_raw, mean, rstd, w, b, want_stats=True, step=None):
    """conv3d(LeakyReLU((x_raw - mean) * rstd), w, b) with the normalisation applied while the input tile is staged;
    returns (y, stats or None)"""
    _chk(x_raw, mean, rstd, w, b)
    _conv_args("conv3d_forward_normin", x_raw, w, b)
    step = step if step is not None else current_step()
    B, Cin = x_raw.shape[0], x_raw.shape[-1]
    _same_shape("conv3d_forward_normin", "mean", mean, (B * Cin,), f"input {tuple(x_raw.shape)}")
    _same_shape("conv3d_forward_normin", "rstd", rstd, (B * Cin,), f"input {tuple(x_raw.shape)}")
    return _conv_fwd(x_raw, w, b, step, norm=(mean, rstd), want_stats=want_stats)


# ---- gradient magnitudes for the f16 forms of the backward convolutions (round 5).  The z-marching kernels run on two f16 pieces
# per operand (three MFMA products instead of the six of three bf16 pieces) when they know max |d_y|: f16 has the mantissa for
# it, not the range.  The InstanceNorm backward that PRODUCES a d_y leaves that maximum in a one-float tensor for free
# (modet_instnorm_lrelu_bwd*_amax) and tags its output with it; the conv backward that CONSUMES the tensor reads the tag.  The tag
# carries the tensor's version counter: if autograd accumulated another gradient into the tensor on the way (in place), the
# maximum no longer bounds it and the consumer falls back to the bf16 pieces.  MODET_GRAD_F16=0: never tag (A/B switch).
GRAD_F16 = os.environ.get("MODET_GRAD_F16", "1") != "0"


AMAX_FLOATS = 64 * 32                     # MODET_AMAX_FLOATS: 64 slots, 128 bytes apart (include/modet_hip.h)


def _new_amax(like):
    """the buffer an InstanceNorm backward leaves max |d_x| in -- only where a conv kernel with an f16 form (families 2 and 5)
    would consume d_x as its d_y, else None (the plain call)"""
    if not GRAD_F16:
        return None
    if like.dim() != 5:
        return None
    B, D, H, W, C = like.shape
    key = ("amax", B, D, H, W, C)
    use = _FAM_CACHE.get(key)
    if use is None:          # (the consumer's other channel count is not known here; the families split by volume and channel class)
        use = _FAM_CACHE[key] = _L().modet_conv3d_kernel_family(B, D, H, W, C, C, 1) in _FAM_F16_DGRAD
    return torch.empty(AMAX_FLOATS, dtype=torch.float32, device=like.device) if use else None


def amax_buffer(value):
    """a gradient-maximum buffer (every slot = value) for callers that know a bound of |d_y| themselves"""
    return value.detach().reshape(1).float().expand(AMAX_FLOATS).contiguous()


def _tag_amax(t, amax):
    if amax is not None:
        t._modet_amax = (amax, t._version)
    return t


def _amax_of(t):
    tag = getattr(t, "_modet_amax", None)
    if tag is None or not GRAD_F16 or tag[1] != t._version:
        return None
    return tag[0]


def conv3d_backward_data(dy, w, Cin, step=None, amax=None):
    _chk(dy, w, amax)
    step = step if step is not None else current_step()
    if dy.dim() != 5:
        raise RuntimeError(f"conv3d_backward_data: expects a channels-last (B,D,H,W,Cout) gradient, got {tuple(dy.shape)}")
    B, D, H, W, Cout = dy.shape
    _same_shape("conv3d_backward_data", "weight", w, (Cout, Cin, 3, 3, 3), f"gradient {tuple(dy.shape)}, Cin {Cin}")
    _amax_arg("conv3d_backward_data", amax)
    dx = torch.empty((B, D, H, W, Cin), dtype=torch.float32, device=dy.device)
    L = _L()
    nb = L.modet_conv3d_ws_bytes(Cin, Cout)
    ws = _ws(nb, dy)
    n = float(B) * D * H * W
    with _Guard(dy, _conv_tag("dgrad", dy.shape, Cin, Cout, f16=amax is not None), 54.0 * Cin * Cout * n, 4.0 * n * (Cin + Cout)):
        _call(L.modet_conv3d_bwd_data_amax, _p(dy), _p(w), _p(dx), _p(ws), nb, B, D, H, W, Cin, Cout, _p(amax), _stream(), _h(step))
    return dx


class StepContext:
    """Caller-owned state of the step-level launch batching (include/modet_hip.h, modet_step_ctx_t): the recorded
    weight-packing jobs of ONE forward+backward computation (one input shape / grad mode) and the weight-gradient
    reductions its backward pass queues.  Nothing is process-wide: every Trainer keeps its own contexts (one per shape it
    has seen), so two trainers in one process -- two threads, two devices, a training and an evaluation model -- never see
    each other's jobs.

      with sc.prepacked():                       # first use records the packing jobs while running normally; later uses
          forward                                # start with ONE launch that packs every recorded weight tensor and the
          with sc.deferred(dst) as scope:        # conv launches skip theirs
              backward                           # ~20 partial-tile reductions -> one launch at scope exit, written to dst

    The scopes bind the context to the calling thread; every conv op picks it up in its forward and hands it to its own
    backward (which runs on the autograd thread), so no op ever consults a global.  The owner guarantees that the weights
    are not modified inside ``prepacked()`` and live at the same addresses from one pass to the next (FlatParams views
    do).  The packed-weights arena lives as long as the context -- a captured hipGraph that bakes its address in stays
    valid however many other shapes the trainer runs eagerly in between."""

    def __init__(self):
        import ctypes
        h = ctypes.c_void_p()
        _call(_L().modet_step_ctx_create, ctypes.byref(h))
        self.handle = h
        self.arena = None            # packed weights of every recorded conv launch (fp32 jobs, then the 16-bit ones)
        self.recorded = False
        self.dst = None              # parameter.data_ptr() -> gradient destination, while a deferred() scope is open
        self.written = set()
        self._keep = []
        self._leaf = []              # queued leaf reductions (modet_leaf_job_t) of the open deferred() scope, see defer_leaf

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        lib = getattr(_lib, "_lib", None) if _lib is not None else None     # (module globals are gone at interpreter exit)
        if h is not None and lib is not None:
            lib.modet_step_ctx_destroy(h)

    class _Bind:
        def __init__(self, sc):
            self.sc = sc

        def __enter__(self):
            self.prev = getattr(_TLS, "step", None)
            _TLS.step = self.sc
            return self

        def __exit__(self, *exc):
            _TLS.step = self.prev
            return False

    class _Prepacked(_Bind):
        def __enter__(self):
            sc, L = self.sc, _L()
            self.recording = not sc.recorded
            if self.recording:
                L.modet_conv3d_prepack_record(sc.handle, 1)
            else:
                _call(L.modet_conv3d_prepack_begin, sc.handle, _p(sc.arena), sc.arena.numel() * 4, _stream())
            return super().__enter__()

        def __exit__(self, *exc):
            sc, L = self.sc, _L()
            super().__exit__(*exc)
            if self.recording:
                L.modet_conv3d_prepack_record(sc.handle, 0)
                if exc[0] is None:
                    dev = torch.device("cuda", torch.cuda.current_device())
                    sc.arena = torch.empty(L.modet_conv3d_prepack_arena_bytes(sc.handle) // 4 + 64, dtype=torch.float32,
                                           device=dev)
                    sc.recorded = True
            else:
                L.modet_conv3d_prepack_end(sc.handle)
            return False

    class _Deferred(_Bind):
        def __init__(self, sc, dst):
            super().__init__(sc)
            self.dst = dst
            self.written = set()

        def __enter__(self):
            sc = self.sc
            if sc.dst is not None:
                raise RuntimeError("StepContext.deferred scopes do not nest")
            sc.dst, sc.written, sc._keep, sc._leaf = self.dst, self.written, [], []
            return super().__enter__()

        def __exit__(self, *exc):
            sc = self.sc
            super().__exit__(*exc)
            sc.dst = None
            rc = _L().modet_conv3d_wgrad_defer_flush(sc.handle, _stream())    # always empties the queue, also on an exception
            jobs, sc._leaf = sc._leaf, []
            if exc[0] is None and jobs:                  # the attention / projection parameter gradients of every level: one launch
                arr = (_lib.LeafJob * len(jobs))(*jobs)            # host table: copied into the launch's arguments
                _call(_L().modet_leaf_reduce_many, ctypes.addressof(arr), len(jobs), _stream())
            sc._keep = []
            if exc[0] is None:
                _lib.check(rc, "modet_conv3d_wgrad_defer_flush")
            return False

    def prepacked(self):
        return StepContext._Prepacked(self)

    def deferred(self, dst):
        """``dst`` maps ``parameter.data_ptr()`` to the tensor that parameter's gradient must be written to (FlatParams: a
        view of the flat gradient buffer).  A conv whose weight (and bias) have a destination writes there -- after the
        flush -- and returns no gradient to autograd, so nothing depends on how autograd hands tensors to ``.grad``; the
        pointers written are in ``scope.written``.  A conv without a destination, or a second use of the same weight inside
        one scope, takes the immediate path."""
        return StepContext._Deferred(self, dst)

    def destinations(self, w, b, want_bias):
        """(d_w, d_bias) destinations for this call, or None -> immediate path"""
        if self.dst is None:
            return None
        dw = self.dst.get(w.data_ptr()) if w is not None else None
        if dw is None or dw.shape != w.shape or w.data_ptr() in self.written:
            return None
        db = None
        if want_bias:
            db = self.dst.get(b.data_ptr()) if b is not None else None
            if db is None or db.shape != b.shape or b.data_ptr() in self.written:
                return None
        return dw, db

    def defer_leaf(self, ws, outer, outer_stride, rows, row_stride, ncols, col_group, col_group_stride, dsts):
        """queue one column-sum job over the partial rows a backward kernel left at the start of ``ws`` (kept alive until the
        scope's flush): see modet_leaf_reduce_many.  ``dsts``: up to four destination tensors, consecutive column segments."""
        j = _lib.LeafJob()
        j.part, j.outer, j.outer_stride, j.rows, j.row_stride = ws.data_ptr(), outer, outer_stride, rows, row_stride
        j.col_group_stride, j.ncols, j.col_group = col_group_stride, ncols, col_group
        for u in range(4):
            j.dst[u] = dsts[u].data_ptr() if u < len(dsts) else None
            j.n[u] = dsts[u].numel() if u < len(dsts) else 0
        if sum(j.n) != ncols:
            raise RuntimeError("defer_leaf: the destination segments do not add up to the job's columns")
        self._leaf.append(j)
        self._keep.append(ws)

    def claim(self, *params):
        """gradient destinations of a node's parameters (projection weight / bias / gamma / beta, an attention's rpb): the
        list of destination tensors when EVERY one has a destination and none was written in this scope yet -- they are then
        marked written and the node's backward kernel writes its results straight there (no gradient returned to autograd,
        no packing copy) -- else None -> the node returns its gradients to autograd as usual."""
        if self.dst is None:
            return None
        out = []
        for p in params:
            d = self.dst.get(p.data_ptr())
            if d is None or d.shape != p.shape or p.data_ptr() in self.written:
                return None
            out.append(d)
        for p in params:
            self.written.add(p.data_ptr())
        return out


# the parameter gradients of the attention / projection nodes (d_rpb; d_gamma, d_beta, d_bias, d_W) of all levels are summed
# by ONE launch at the end of the deferred() scope instead of 2 + 1 launches per level (read at backward time)
DEFER_LEAF_REDUCTIONS = True

_TLS = threading.local()


def _defer_rpb(step, ws, B, D, H, W, heads, hd, drpb):
    """the d_rpb column sums of one attention backward (partial rows at the start of ``ws``: [B][heads][rows][27]) -> the scope's
    single leaf-reduction launch"""
    rows = int(_L().modet_na_bwd_partial_rows(B, D, H, W, heads, hd))
    step.defer_leaf(ws, B, heads * rows * 27, rows, 27, heads * 27, 27, rows * 27, [drpb])


def _defer_proj(step, ws, N, Cin, dim, dW, db, dg, dbeta):
    """the parameter-gradient column sums of one paired projection backward (rows [d_gamma | d_beta | d_bias | d_W])"""
    rows = int(_L().modet_proj_ln_bwd_pair_partial_rows(N, Cin, dim))
    ncols = 3 * dim + dim * Cin
    step.defer_leaf(ws, 1, 0, rows, ncols, ncols, ncols, 0, [dg, dbeta, db, dW])


def current_step():
    """the StepContext bound to this thread by an open ``prepacked()`` / ``deferred()`` scope, or None"""
    return getattr(_TLS, "step", None)


def _h(step):
    return None if step is None else step.handle


def conv3d_backward_weight(x, dy, want_bias, y_act=None, w=None, b=None, step=None, amax=None, norm=None):
    """d_w, d_bias; with y_act (ConvBlock 1 -> 4 only) dy is the gradient w.r.t. LeakyReLU(conv) and the activation's
    derivative is applied while loading it.  With a StepContext (given, or bound to this thread) whose ``deferred()`` scope
    knows destinations for the parameters ``w`` / ``b``, the gradients go straight there at the scope's flush and
    (None, None) is returned.  amax: one-float tensor >= max |dy| (see _tag_amax) and the caller's word that x is an
    activation: the z-marching kernel then runs on two f16 pieces.  norm = (mean, rstd): x is a RAW ConvInsBlock output,
    normalised while the kernel stages it (only where the library's *_normin_ok says so)."""
    _chk(x, dy, y_act, amax)
    if x.dim() != 5 or dy.dim() != 5 or tuple(dy.shape[:4]) != tuple(x.shape[:4]):
        raise RuntimeError(f"conv3d_backward_weight: gradient {tuple(dy.shape)} does not match input {tuple(x.shape)}")
    B, D, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    _same_shape("conv3d_backward_weight", "y_act", y_act, dy.shape, "the gradient")
    _amax_arg("conv3d_backward_weight", amax)
    if norm is not None:
        _chk(*norm)
        _same_shape("conv3d_backward_weight", "mean", norm[0], (B * Cin,), f"input {tuple(x.shape)}")
        _same_shape("conv3d_backward_weight", "rstd", norm[1], (B * Cin,), f"input {tuple(x.shape)}")
    L = _L()
    nb = L.modet_conv3d_bwd_weight_ws_bytes(B, D, H, W, Cin, Cout)
    n = float(B) * D * H * W
    f16 = amax is not None and y_act is None

    def launch(dw, db, ws, scope):
        """the one library call: ``scope`` = the StepContext whose flush reduces the partial tiles, None = they are reduced now"""
        if norm is not None:
            fn, head, tail = L.modet_conv3d_bwd_weight_normin, (x, norm[0], norm[1], dy), (_p(amax), _stream(), _h(scope))
        elif f16:
            fn, head, tail = L.modet_conv3d_bwd_weight_amax, (x, dy), (_p(amax), _stream(), _h(scope))
        elif scope is not None:
            fn, head, tail = L.modet_conv3d_bwd_weight_defer, (x, dy, y_act), (_stream(), _h(scope))
        elif y_act is not None:
            fn, head, tail = L.modet_conv3d_bwd_weight_act, (x, dy, y_act), (_stream(),)
        else:
            fn, head, tail = L.modet_conv3d_bwd_weight, (x, dy), (_stream(),)
        with _Guard(x, _conv_tag("wgrad", x.shape, Cin, Cout, f16=f16), 54.0 * Cin * Cout * n, 4.0 * n * (Cin + Cout)):
            _call(fn, *map(_p, head), _p(dw), _p(db), _p(ws), nb, B, D, H, W, Cin, Cout, *tail)

    scope = step if step is not None else current_step()
    dst = scope.destinations(w, b, want_bias) if scope is not None else None
    ws = _ws(nb, x)
    if dst is None:
        dw = torch.empty((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=x.device)
        db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_bias else None
        launch(dw, db, ws, None)
        return dw, db
    dw, db = dst
    launch(dw, db, ws, scope)
    scope._keep.append(ws)                                # the partial tiles must survive until the flush
    if amax is not None:
        scope._keep.append(amax)                          # (a queued launch reads the maximum at the flush, too)
    if y_act is None and L.modet_conv3d_wgrad_defers_operands(B, D, H, W, Cin, Cout):
        scope._keep.extend((x, dy))                       # small levels: the launch itself is queued and reads them at the flush
    scope.written.add(w.data_ptr())
    if db is not None:
        scope.written.add(b.data_ptr())
    return None, None


# ------------------------------------------------------------------------------------------------ autograd ops
class _Conv3d(Function):
    @staticmethod
    def forward(ctx, x, w, b, act, x_act=False):
        ctx.step = current_step()
        y = conv3d_forward(x, w, b, act, ctx.step, x_act)
        ctx.act = bool(act)
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w, y if act else None, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, b = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.act and not ctx.needs_input_grad[0] and x.shape[-1] == 1 and w.shape[0] == 4:
            # first encoder block: no d_x, and the weight-gradient kernel folds LeakyReLU' into its d_y load
            dw, db = conv3d_backward_weight(x, dy, ctx.has_bias, y_act=y, w=w, b=b, step=ctx.step)
            return None, dw, db, None, None
        if ctx.act:
            g = torch.empty_like(dy)
            with _Guard(dy, "lrelu_bwd", dy.numel(), 12.0 * dy.numel()):
                _call(_L().modet_lrelu_bwd, _p(dy), _p(y), _p(g), dy.numel(), _stream())
            dy = g
        amax = None if ctx.act else _amax_of(dy)                 # (x is whatever the caller convolved: no f16 weight gradient)
        dw, db = conv3d_backward_weight(x, dy, ctx.has_bias, w=w, b=b, step=ctx.step)
        dx = conv3d_backward_data(dy, w, x.shape[-1], ctx.step, amax) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None, None


class _Conv3dStats(Function):
    """conv3d whose epilogue also produces InstanceNorm partial statistics (second output, not differentiable)"""

    @staticmethod
    def forward(ctx, x, w, b, x_act=False):
        _chk(x, w, b)
        _conv_args("conv3d_with_stats", x, w, b)
        ctx.step = current_step()
        ctx.x_act = bool(x_act)                 # x is an activation (bounded: see modet_conv3d_bwd_weight_amax)
        y, stats = _conv_fwd(x, w, b, ctx.step, bounded=ctx.x_act, want_stats=True)
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w, b)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)        # no zeros_like(stats) fill launch for the statistics output's "gradient"
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        if dy is None:
            return None, None, None, None
        x, w, b = ctx.saved_tensors
        dy = dy.contiguous()
        amax = _amax_of(dy)
        dw, db = conv3d_backward_weight(x, dy, ctx.has_bias, w=w, b=b, step=ctx.step, amax=amax if ctx.x_act else None)
        dx = conv3d_backward_data(dy, w, x.shape[-1], ctx.step, amax) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


def _fuse_stats(x, w, needs_grad=None):
    """fuse the InstanceNorm statistics into this conv's epilogue?  The staged epilogue of the 16-wide configurations
    (Cout 4/8/16) carries them for free; in the direct-store configurations they cost the conv ~3 % and only pay off when
    no backward pass follows (measured: training +0.07 ms, inference -0.05 ms)."""
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    L = _L()
    if L.modet_conv3d_stats_bytes(B, D, H, W, Cin, Cout) == 0:
        return False
    if L.modet_conv3d_kernel_family(B, D, H, W, Cin, Cout, 0) in _FAM_BF16X3_FWD:
        return True
    if needs_grad is None:     # (inside an autograd.Function.forward grad mode is off: such callers pass their ctx.needs_input_grad)
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
    return Cout in (4, 8, 16) or not needs_grad


def conv3d_instnorm_lrelu(x, w, b, eps=1e-5, x_act=False):
    """ConvInsBlock = conv + InstanceNorm3d + LeakyReLU(0.1) (reference models.py:135-151); the norm statistics are
    fused into the conv epilogue when the configuration supports it.  x_act: see conv3d_forward"""
    if _fuse_stats(x, w):
        y, stats = _Conv3dStats.apply(x, w, b, x_act)
        return _InstNormLReLU.apply(y, eps, stats)
    return _InstNormLReLU.apply(_Conv3d.apply(x, w, b, False, x_act), eps, None)


def lazy_instnorm_conv3d(x_raw, stats_in, w, b, eps=1e-5, want_stats=True):
    """conv3d(LeakyReLU(InstanceNorm(x_raw)), w, b) -> (z_raw, z_stats or None); want_stats=False when z is not normalised.

    Without gradients (inference) the normalised tensor is never materialised: the statistics come from the previous
    conv's epilogue (or one statistics pass) and the conv kernel normalises its input tile while staging it (-3.5 % on the
    forward pass).  With gradients the tensor is needed by the weight gradient anyway (normalising on the fly there was
    measured slower), so the block runs as InstanceNorm + conv."""
    _conv_args("lazy_instnorm_conv3d", x_raw, w, b)          # (before the statistics launch of the inference form)
    Cin = x_raw.shape[-1]
    needs_grad = torch.is_grad_enabled() and (x_raw.requires_grad or w.requires_grad)
    if not needs_grad and Cin % 4 == 0 and Cin > 1:
        mean, rstd = instnorm_stats(x_raw, stats_in, eps)
        return conv3d_forward_normin(x_raw, mean, rstd, w, b, want_stats)
    return _InstNormConv.apply(x_raw, stats_in, w, b, eps, want_stats)


# The data gradient of a conv whose input is LeakyReLU(InstanceNorm(x_raw)) can form that norm's backward statistics in
# its own epilogue (modet_conv3d_bwd_data_instats: kernel family 2 only): the norm's backward then skips its first pass
# over (d_y, x_raw).  False = the two ops run back to back as before (A/B switch of the parity tests).
FUSE_IN_DGRAD = os.environ.get("MODET_FUSE_IN_DGRAD", "1") != "0"
# Round 5: where the weight-gradient kernel can normalise its x operand while staging it (modet_conv3d_bwd_weight_normin_ok: the
# z-marching kernel, i.e. the level-1 layers) the TRAINING step does not materialise LeakyReLU(InstanceNorm(x_raw)) either: forward
# = statistics finalize + modet_conv3d_fwd_normin, weight gradient = modet_conv3d_bwd_weight_normin, data gradient and the norm's
# backward as before (they never needed the normalised tensor).  Saves the apply pass (0.12 ms at level 1) and 315 MB.
# False = materialise as before (A/B switch).
LAZY_IN_TRAIN = os.environ.get("MODET_LAZY_IN_TRAIN", "1") != "0"


class _InstNormConv(Function):
    """z = conv3d(LeakyReLU(InstanceNorm(x_raw)), w, b) as ONE autograd node (ConvInsBlock -> conv, reference
    models.py:186-219 / :252-254), so that its backward can hand the conv's data gradient and the norm's backward
    statistics over inside one kernel.  Returns (z, z_stats or None)."""

    @staticmethod
    def forward(ctx, x_raw, stats_in, w, b, eps, want_stats):
        _chk(x_raw, stats_in, w, b)
        _conv_args("lazy_instnorm_conv3d", x_raw, w, b)
        ctx.step = current_step()
        B, C = x_raw.shape[0], x_raw.shape[-1]
        ctx.lazy = False
        if (LAZY_IN_TRAIN and x_raw.dim() == 5 and C % 4 == 0 and
                _L().modet_conv3d_bwd_weight_normin_ok(B, x_raw.shape[1], x_raw.shape[2], x_raw.shape[3], C, w.shape[0])):
            mean, rstd = instnorm_stats(x_raw, stats_in, eps)
            z, stats = conv3d_forward_normin(x_raw, mean, rstd, w, b, want_stats, ctx.step)
            if stats is not None:
                ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)
            ctx.has_bias = b is not None
            ctx.lazy = True
            ctx.save_for_backward(x_raw, mean, rstd, None, w, b)
            return z, stats
        y, mean, rstd = _in_fwd(x_raw, stats_in, eps)
        stats = None
        if want_stats and _fuse_stats(y, w, needs_grad=any(ctx.needs_input_grad)):
            z, stats = _conv_fwd(y, w, b, ctx.step, bounded=True, want_stats=True)      # (y: LeakyReLU(InstanceNorm(.)))
            ctx.mark_non_differentiable(stats)
        else:
            z = conv3d_forward(y, w, b, False, ctx.step, x_act=True)
        ctx.set_materialize_grads(False)        # no zeros_like(stats) fill launch for the statistics output's "gradient"
        ctx.has_bias = b is not None
        ctx.save_for_backward(x_raw, mean, rstd, y, w, b)
        return z, stats

    @staticmethod
    def backward(ctx, dz, _dstats):
        if dz is None:
            return None, None, None, None, None, None
        x_raw, mean, rstd, y, w, b = ctx.saved_tensors
        dz = dz.contiguous()
        B, D, H, W, C = x_raw.shape
        Cout = w.shape[0]
        V = D * H * W
        L = _L()
        d_raw = None
        amax = _amax_of(dz)
        if ctx.lazy:
            dw, db = conv3d_backward_weight(x_raw, dz, ctx.has_bias, w=w, b=b, step=ctx.step, amax=amax, norm=(mean, rstd))
        else:
            dw, db = conv3d_backward_weight(y, dz, ctx.has_bias, w=w, b=b, step=ctx.step, amax=amax)   # (first: see _Conv3d.backward)
        if ctx.needs_input_grad[0]:
            rb = L.modet_conv3d_bwd_data_instats_bytes(B, D, H, W, C, Cout) if FUSE_IN_DGRAD else 0
            if rb > 0:
                d_raw = torch.empty_like(x_raw)
                amax_raw = _new_amax(x_raw)
                d_y = torch.empty_like(x_raw)
                rows = torch.empty(rb // 4, dtype=torch.float32, device=x_raw.device)
                nb = L.modet_conv3d_ws_bytes(C, Cout)
                ws = _ws(nb, dz)
                n = float(B) * V
                with _Guard(dz, _conv_tag("dgrad", dz.shape, C, Cout, f16=amax is not None), 54.0 * C * Cout * n, 4.0 * n * (2 * C + Cout)):
                    _call(L.modet_conv3d_bwd_data_instats_amax, _p(dz), _p(w), _p(d_y), _p(x_raw), _p(mean), _p(rstd), _p(rows), rb,
                          _p(ws), nb, B, D, H, W, C, Cout, _p(amax), _stream(), _h(ctx.step))
                nb2 = 2 * B * C * 4
                ws2 = _ws(nb2, x_raw)
                with _Guard(x_raw, "instnorm_lrelu_bwd", 7.0 * x_raw.numel(), 12.0 * x_raw.numel()):
                    _call(L.modet_instnorm_lrelu_bwd_rows_amax, _p(d_y), _p(x_raw), _p(mean), _p(rstd), _p(d_raw), _p(rows), rb,
                          _p(ws2), nb2, B, V, C, _p(amax_raw), _stream())
                _tag_amax(d_raw, amax_raw)
            else:
                d_raw = _in_bwd(conv3d_backward_data(dz, w, C, ctx.step, amax), x_raw, mean, rstd)
        return d_raw, None, dw, db, None, None


def conv3d_with_stats(x, w, b, x_act=False):
    """raw 3x3x3 conv output plus, when the configuration supports it, the InstanceNorm partial statistics from its
    epilogue (else None).  x_act: the caller's word that x is an activation (a ConvBlock / ConvInsBlock output or a pooled
    one), which lets the weight gradient split it into f16 pieces with a fixed scale."""
    if _fuse_stats(x, w):
        return _Conv3dStats.apply(x, w, b, x_act)
    return _Conv3d.apply(x, w, b, False, x_act), None


def conv3d(x, w, b=None, act=False, x_act=False):
    """3x3x3 conv, zero pad 1 (+ fused LeakyReLU(0.1) if act).  reference: nn.Conv3d, models.py:127,:144,:254.  Any input range
    (x_act=True: the caller's word that |x| < 4 094 -- half the matrix work, see conv3d_forward)"""
    return _Conv3d.apply(x, w, b, act, x_act)


class _InstNormLReLU(Function):
    @staticmethod
    def forward(ctx, x, eps, stats=None):
        _chk(x)
        y, mean, rstd = _in_fwd(x, stats, eps)
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        return _in_bwd(dy.contiguous(), x, mean, rstd), None, None


def instnorm_lrelu(x, eps=1e-5):
    """InstanceNorm3d(affine=False) + LeakyReLU(0.1), channels-last.  reference: models.py:144-150"""
    return _InstNormLReLU.apply(x, eps, None)


def _pool_fwd(x):
    """THE AvgPool3d(2) forward launch (x: a checked fp32 (B,D,H,W,C) tensor)"""
    B, D, H, W, C = x.shape
    y = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    with _Guard(x, "avgpool2_fwd", x.numel(), 4.5 * x.numel()):
        _call(_L().modet_avgpool2_fwd, _p(x), _p(y), B, D, H, W, C, _stream())
    return y


def _pool_bwd(gy, shape, parts, nbytes):
    """THE AvgPool3d(2) backward: d_x = unpool(gy) / 8 + addend, one launch per (lo, hi, addend or None) batch range of
    ``parts`` inside one bracket; nbytes: the bracket's bytes per element of d_x"""
    D, H, W, C = shape[1:]
    dx = torch.empty(shape, dtype=torch.float32, device=gy.device)
    with _Guard(gy, "avgpool2_bwd", dx.numel(), nbytes * dx.numel()):
        for lo, hi, add in parts:
            add = None if add is None else add.contiguous()
            _call(_L().modet_avgpool2_bwd, _p(gy[lo:hi]), _p(add), _p(dx[lo:hi]), hi - lo, D, H, W, C, _stream())
    return dx


def _halves(ga, gb, Bh, shape):
    """[ga ; gb] as one fp32 tensor of ``shape``, zeros for an absent half"""
    g = torch.empty(shape, dtype=torch.float32, device=(ga if ga is not None else gb).device)
    for part, src in ((g[:Bh], ga), (g[Bh:], gb)):
        if src is None:
            part.zero_()
        else:
            part.copy_(src)
    return g


class _AvgPool2(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        _rank5("avgpool2", "x", x)
        ctx.shape = tuple(x.shape)
        return _pool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return _pool_bwd(dy.contiguous(), ctx.shape, ((0, ctx.shape[0], None),), 4.5)


def avgpool2(x):
    """nn.AvgPool3d(2), channels-last.  reference: models.py:201,:207,:213,:219"""
    return _AvgPool2.apply(x)


class _PoolTee(Function):
    """x -> (avgpool2(x), x): the pyramid feeds every feature map both to the next level's pooling and to the
    attention/warp branch; one backward kernel returns g_x + unpool(g_pooled)/8 instead of a pool-backward pass
    followed by autograd's add over two full-size tensors."""

    @staticmethod
    def forward(ctx, x):
        _chk(x)
        _rank5("pool_tee", "x", x)
        ctx.shape = tuple(x.shape)
        return _pool_fwd(x), x.view_as(x)

    @staticmethod
    def backward(ctx, gy, gx):
        if gy is None:
            return gx
        gx = None if gx is None else gx.contiguous()
        return _pool_bwd(gy.contiguous(), ctx.shape, ((0, ctx.shape[0], gx),), 4.5 if gx is None else 8.5)


def pool_tee(x):
    """(avgpool2(x), x) with a fused backward; see _PoolTee"""
    return _PoolTee.apply(x)


class _PoolTeeSplit(Function):
    """x (2B,...) -> (avgpool2(x), x[:B], x[B:]): _PoolTee for the [moving; fixed] batch whose two halves go to
    different consumers (warp / projection).  The backward runs the fused unpool+add once per half, each with its own
    addend, so the two half gradients are never concatenated."""

    @staticmethod
    def forward(ctx, x, Bh):
        _chk(x)
        _rank5("pool_tee_split", "x", x)
        B, D, H, W, C = x.shape
        if not 0 < Bh < B:
            raise RuntimeError(f"pool_tee_split: split {Bh} is not inside the batch of {tuple(x.shape)}")
        ctx.shape = (B, D, H, W, C)
        ctx.Bh = Bh
        return _pool_fwd(x), x[:Bh], x[Bh:]

    @staticmethod
    def backward(ctx, gy, ga, gb):
        B, Bh = ctx.shape[0], ctx.Bh
        if gy is None:
            return _halves(ga, gb, Bh, ctx.shape), None
        return _pool_bwd(gy.contiguous(), ctx.shape, ((0, Bh, ga), (Bh, B, gb)), 8.5), None


def pool_tee_split(x, Bh):
    """(avgpool2(x), x[:Bh], x[Bh:]) with a fused backward; see _PoolTeeSplit"""
    return _PoolTeeSplit.apply(x, Bh)


class _InstNormLReLUPoolSplit(Function):
    """_InstNormLReLU followed by _PoolTeeSplit as ONE node: x_raw (2B,...) -> (avgpool2(y), y[:B], y[B:]) with
    y = LeakyReLU(InstanceNorm(x_raw)).  Forward: statistics (finalize only, or one pass), then one kernel that writes y
    and its pooled copy (modet_instnorm_lrelu_apply_pool: the separate AvgPool3d re-read y).  Backward: the two nodes'
    backward kernels in sequence, unchanged.  Bit-identical to the two-node form."""

    @staticmethod
    def forward(ctx, x, eps, stats, Bh):
        _chk(x, stats)
        _rank5("instnorm_lrelu_pool_tee_split", "x_raw", x)
        B, D, H, W, C = x.shape
        if not 0 < Bh < B:
            raise RuntimeError(f"instnorm_lrelu_pool_tee_split: split {Bh} is not inside the batch of {tuple(x.shape)}")
        y = torch.empty_like(x)
        pooled = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
        with _Guard(x, "instnorm_lrelu_fwd", 9.0 * x.numel(), 8.5 * x.numel()):
            mean, rstd = _in_stats(x, stats, eps, pass_x=True)
            _call(_L().modet_instnorm_lrelu_apply_pool, _p(x), _p(mean), _p(rstd), _p(y), _p(pooled), B, D, H, W, C, _stream())
        ctx.save_for_backward(x, mean, rstd)
        ctx.Bh = Bh
        ctx.set_materialize_grads(False)        # an unused output arrives as None (no zeros fill launch); handled below
        return pooled, y[:Bh], y[Bh:]

    @staticmethod
    def backward(ctx, gy, ga, gb):
        if not ctx.needs_input_grad[0] or (gy is None and ga is None and gb is None):
            return None, None, None, None
        x, mean, rstd = ctx.saved_tensors
        B, D, H, W, C = x.shape
        Bh = ctx.Bh
        if gy is None:
            return _in_bwd(_halves(ga, gb, Bh, x.shape), x, mean, rstd), None, None, None
        # d_y = unpool(gy) / 8 + [ga ; gb] is formed inside the two InstanceNorm backward passes, never written
        gy = gy.contiguous()
        ga = None if ga is None else ga.contiguous()
        gb = None if gb is None else gb.contiguous()
        dx = torch.empty_like(x)
        amax = _new_amax(x)
        L = _L()
        nb = L.modet_instnorm_ws_bytes(B, D * H * W, C)
        ws = _ws(nb, x)
        with _Guard(x, "instnorm_lrelu_bwd", 15.0 * x.numel(), 12.5 * x.numel()):
            _call(L.modet_instnorm_lrelu_bwd_pool_amax, _p(gy), _p(ga), _p(gb), Bh, _p(x), _p(mean), _p(rstd), _p(dx), _p(ws), nb,
                  B, D, H, W, C, _p(amax), _stream())
        return _tag_amax(dx, amax), None, None, None


def instnorm_lrelu_pool_tee_split(x_raw, stats, Bh, eps=1e-5):
    """(avgpool2(y), y[:Bh], y[Bh:]) for y = LeakyReLU(InstanceNorm(x_raw)); see _InstNormLReLUPoolSplit"""
    return _InstNormLReLUPoolSplit.apply(x_raw, eps, stats, Bh)


def _proj_args(op, Cin, Wt, b, gamma, beta):
    """Wt (dim, Cin); b, gamma, beta (dim,)"""
    if Wt.dim() != 2:
        raise RuntimeError(f"{op}: expects a (dim, Cin) weight, got {tuple(Wt.shape)}")
    _same_shape(op, "weight", Wt, (Wt.shape[0], Cin), f"input channels {Cin}")
    for name, t in (("bias", b), ("gamma", gamma), ("beta", beta)):
        _same_shape(op, name, t, (Wt.shape[0],), f"weight {tuple(Wt.shape)}")


def _param_dsts(step, *params):
    """where a matching node's backward writes its parameter gradients -> (destinations, later, what goes back to autograd).
    Claimed from the step's deferred() scope (StepContext.claim): written in place, autograd gets None for each, and ``later``
    says that the kernel leaves partial rows which the scope's one leaf-reduction launch sums (DEFER_LEAF_REDUCTIONS).
    Otherwise fresh tensors, reduced by the launch itself and returned to autograd."""
    dst = step.claim(*params) if step is not None else None
    if dst is not None:
        return dst, DEFER_LEAF_REDUCTIONS, [None] * len(params)
    dst = [torch.empty_like(p) for p in params]
    return dst, False, dst


def _proj_pair_bwd(x1, dy1, x2, dy2, Wt, b, gamma, eps, step, dsts, later, typed=False):
    """THE paired projection backward launch -> (d_x1, d_x2), fp32; dsts = (d_W, d_bias, d_gamma, d_beta) of _param_dsts.
    typed: the bf16-storage node's entry point (modet_proj_ln_bwd_pair_t: each input fp32 or bf16), whose byte figure counts
    one bf16 and one fp32 input; the fp32 node keeps the plain one."""
    Cin, dim = x1.shape[-1], Wt.shape[0]
    N = x1.numel() // Cin
    L = _L()
    dx1 = torch.empty(x1.shape, dtype=torch.float32, device=x1.device)
    dx2 = torch.empty(x2.shape, dtype=torch.float32, device=x2.device)
    nb = L.modet_proj_ln_bwd_pair_ws_bytes(N, Cin, dim)
    if nb == 0:
        raise RuntimeError(f"{'level attention (bf16)' if typed else 'proj_ln_pair'}: no paired projection backward for Cin {Cin}, dim {dim}")
    ws = _ws(nb, x1)
    out4 = map(_p, (None, None, None, None) if later else dsts)
    with _Guard(x1, f"proj_ln_bwd[{Cin}->{dim}]", 2.0 * N * (6.0 * Cin * dim + 20.0 * dim), N * ((14.0 if typed else 16.0) * Cin + 8.0 * dim)):
        if typed:
            _call(L.modet_proj_ln_bwd_pair_t, _p(x1), _isbf(x1), _p(dy1), _p(dx1), _p(x2), _isbf(x2), _p(dy2), _p(dx2), _p(Wt), _p(b),
                  _p(gamma), *out4, _p(ws), nb, N, Cin, dim, eps, _stream())
        else:
            _call(L.modet_proj_ln_bwd_pair, _p(x1), _p(dy1), _p(dx1), _p(x2), _p(dy2), _p(dx2), _p(Wt), _p(b), _p(gamma), *out4,
                  _p(ws), nb, N, Cin, dim, eps, _stream())
    if later:
        _defer_proj(step, ws, N, Cin, dim, *dsts)
    return dx1, dx2


def _na_fwd(q, k, rpb, heads, scale, need_grad):
    """THE attention forward launch -> (out, lse or None): modet_na_fwd for fp32 q / k, modet_na_fwd_t for bf16 ones"""
    B, D, H, W, C = q.shape
    typed = q.dtype == torch.bfloat16
    L = _L()
    out = torch.empty((B, D, H, W, heads * 3), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, D, H, W, heads), dtype=torch.float32, device=q.device) if need_grad else None
    nvh = float(B) * D * H * W * heads      # 12 elements of q,k + 12 B of out, ~620 flop per voxel-head
    head = (_p(q), _p(k), 1) if typed else (_p(q), _p(k))
    with _Guard(q, f"na_fwd[h{heads}]", 620.0 * nvh, (12.0 + 12.0 * q.element_size()) * nvh):
        _call(L.modet_na_fwd_t if typed else L.modet_na_fwd, *head, _p(rpb), _p(out), _p(lse), B, D, H, W, heads, C // heads,
              float(scale), _stream())
    return out, lse


def _na_bwd(q, k, rpb, out, lse, dout, heads, scale, step, drpb, later):
    """THE attention backward launch -> (d_q, d_k), fp32; entry point by q's dtype as _na_fwd; drpb: _param_dsts' destination"""
    B, D, H, W, C = q.shape
    typed = q.dtype == torch.bfloat16
    L = _L()
    dq = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    dk = torch.empty_like(dq)
    nb = L.modet_na_bwd_ws_bytes(B, D, H, W, heads)
    ws = _ws(nb, q)
    nvh = float(B) * D * H * W * heads      # reads q,k (12 elements), d_out,out,lse (7 floats), writes d_q,d_k (12)
    head = (_p(q), _p(k), 1) if typed else (_p(q), _p(k))
    with _Guard(q, f"na_bwd[h{heads}]", 1900.0 * nvh, (76.0 + 12.0 * q.element_size()) * nvh):
        _call(L.modet_na_bwd_t if typed else L.modet_na_bwd, *head, _p(rpb), _p(out), _p(lse), _p(dout), _p(dq), _p(dk),
              _p(None if later else drpb), _p(ws), nb, B, D, H, W, heads, C // heads, scale, _stream())
    if later:
        _defer_rpb(step, ws, B, D, H, W, heads, C // heads, drpb)
    return dq, dk


class _ProjLN(Function):
    @staticmethod
    def forward(ctx, x, Wt, b, gamma, beta, eps):
        _chk(x, Wt, b, gamma, beta)
        Cin = x.shape[-1]
        dim = Wt.shape[0]
        _proj_args("proj_ln", Cin, Wt, b, gamma, beta)
        N = x.numel() // Cin
        y = torch.empty(x.shape[:-1] + (dim,), dtype=torch.float32, device=x.device)
        with _Guard(x, f"proj_ln_fwd[{Cin}->{dim}]", N * (2.0 * Cin * dim + 8.0 * dim), 4.0 * N * (Cin + dim)):
            _call(_L().modet_proj_ln_fwd, _p(x), _p(Wt), _p(b), _p(gamma), _p(beta), _p(y), N, Cin, dim, eps, _stream())
        ctx.save_for_backward(x, Wt, b, gamma, beta)
        ctx.eps = eps
        ctx.step = current_step()
        return y

    @staticmethod
    def backward(ctx, dy):
        x, Wt, b, gamma, beta = ctx.saved_tensors
        dy = dy.contiguous()
        Cin = x.shape[-1]
        dim = Wt.shape[0]
        N = x.numel() // Cin
        dx = torch.empty_like(x)
        (dW, db, dg, dbeta), _, ret = _param_dsts(ctx.step, Wt, b, gamma, beta)       # (this kernel reduces them itself)
        L = _L()
        nb = L.modet_proj_ln_bwd_ws_bytes(N, Cin, dim)
        ws = _ws(nb, x)
        with _Guard(x, f"proj_ln_bwd[{Cin}->{dim}]", N * (6.0 * Cin * dim + 20.0 * dim), 4.0 * N * (2 * Cin + dim)):
            _call(L.modet_proj_ln_bwd, _p(x), _p(Wt), _p(b), _p(gamma), _p(dy), _p(dx), _p(dW), _p(db), _p(dg), _p(dbeta), _p(ws), nb,
                  N, Cin, dim, ctx.eps, _stream())
        return (dx, *ret, None)


class _ProjLNPair(Function):
    """The projection layer applied to two inputs of one shape with the same parameters; the backward sums the
    parameter gradients of both uses in one reduction (modet_proj_ln_bwd_pair) instead of autograd adding two results."""

    @staticmethod
    def forward(ctx, x1, x2, Wt, b, gamma, beta, eps):
        _chk(x1, x2, Wt, b, gamma, beta)
        Cin = x1.shape[-1]
        dim = Wt.shape[0]
        _same_shape("proj_ln_pair", "x2", x2, x1.shape, "x1")
        _proj_args("proj_ln_pair", Cin, Wt, b, gamma, beta)
        N = x1.numel() // Cin
        L = _L()
        ys = [torch.empty(x.shape[:-1] + (dim,), dtype=torch.float32, device=x.device) for x in (x1, x2)]
        with _Guard(x1, f"proj_ln_fwd[{Cin}->{dim}]", 2 * N * (2.0 * Cin * dim + 8.0 * dim), 8.0 * N * (Cin + dim)):
            _call(L.modet_proj_ln_fwd_pair, _p(x1), _p(x2), _p(Wt), _p(b), _p(gamma), _p(beta), _p(ys[0]), _p(ys[1]), N, Cin, dim, eps,
                  _stream())
        ctx.save_for_backward(x1, x2, Wt, b, gamma, beta)
        ctx.eps = eps
        ctx.step = current_step()
        return ys[0], ys[1]

    @staticmethod
    def backward(ctx, dy1, dy2):
        x1, x2, Wt, b, gamma, beta = ctx.saved_tensors
        dy1, dy2 = dy1.contiguous(), dy2.contiguous()
        dsts, later, ret = _param_dsts(ctx.step, Wt, b, gamma, beta)
        dx1, dx2 = _proj_pair_bwd(x1, dy1, x2, dy2, Wt, b, gamma, ctx.eps, ctx.step, dsts, later)
        return (dx1, dx2, *ret, None)


def proj_ln_pair(x1, x2, Wt, b, gamma, beta, eps=1e-5):
    """(proj_ln(x1), proj_ln(x2)) with shared parameters -- ModeT's q / k projections of a level (models.py:371-372)"""
    if (x1.shape == x2.shape and torch.is_grad_enabled() and x1.requires_grad and x2.requires_grad and
            _L().modet_proj_ln_bwd_pair_ws_bytes(x1.numel() // x1.shape[-1], x1.shape[-1], Wt.shape[0]) > 0):
        return _ProjLNPair.apply(x1, x2, Wt, b, gamma, beta, eps)
    return _ProjLN.apply(x1, Wt, b, gamma, beta, eps), _ProjLN.apply(x2, Wt, b, gamma, beta, eps)


def proj_ln(x, Wt, b, gamma, beta, eps=1e-5):
    """Linear + LayerNorm on channels-last voxels.  reference: ProjectionLayer, models.py:230-241"""
    return _ProjLN.apply(x, Wt, b, gamma, beta, eps)


POSENC_DIM = 6                   # MODET_POSENC_DIM of include/modet_hip_posenc.h: the only width the kernels have


def posenc_table(D, H, W, device=None):
    """the (cos, sin) table of include/modet_hip_posenc.h for a (D,H,W) grid, (D+H+W, 2) fp32: row p of an axis of length n holds
    cos and sin of p * pi / (n - 1), computed in fp64 and rounded once"""
    rows = []
    for n in (D, H, W):
        if int(n) < 2:
            raise RuntimeError(f"posenc_table: every axis needs at least 2 voxels (p * pi / (n - 1)), got {(D, H, W)}")
        t = torch.arange(int(n), dtype=torch.float64) * (math.pi / (int(n) - 1))
        rows.append(torch.stack((t.cos(), t.sin()), -1))
    return torch.cat(rows).float().to(device).contiguous()


def _posenc_args(op, x1, x2, Wt, b, alpha, tab):
    """x1 (and x2) (B,D,H,W,Cin) fp32; Wt (6,Cin); b (6,); alpha (1,); tab (D+H+W, 2) -> (B, D, H, W, Cin)"""
    for name, t in (("x1", x1), ("x2", x2)):
        if t is not None and getattr(t, "data16", None) is not None:
            raise RuntimeError(f"{op}: {name} is a bf16 feature handle; the positional-encoding kernels are fp32 only")
    _chk(x1, x2, Wt, b, alpha, tab)
    _rank5(op, "x1", x1)
    _same_shape(op, "x2", x2, x1.shape, "x1")
    B, D, H, W, Cin = x1.shape
    if Wt.dim() != 2 or Wt.shape[0] != POSENC_DIM:
        raise RuntimeError(f"{op}: expects a ({POSENC_DIM}, Cin) weight (dim = {POSENC_DIM} only), got {tuple(Wt.shape)}")
    _same_shape(op, "weight", Wt, (POSENC_DIM, Cin), f"input channels {Cin}")
    _same_shape(op, "bias", b, (POSENC_DIM,))
    _same_shape(op, "alpha", alpha, (1,))
    if B < 1 or min(D, H, W) < 2:
        raise RuntimeError(f"{op}: needs a batch and at least 2 voxels along every axis (the embedding divides by n - 1), got {tuple(x1.shape)}")
    _same_shape(op, "tab", tab, (D + H + W, 2), f"posenc_table({D}, {H}, {W})")
    if Cin % 4 != 0 or not 4 <= Cin <= 128:
        raise RuntimeError(f"{op}: {Cin} input channels: the kernels take a multiple of 4 up to 128")
    if _L().modet_posenc_ws_bytes(B, D, H, W, Cin, POSENC_DIM) == 0:
        raise RuntimeError(f"{op}: no kernel covers the shape {tuple(x1.shape)}")
    return B, D, H, W, Cin


class _PosEncPair(Function):
    """The positional-encoding projection applied to one or two inputs of one shape with the same parameters (x2 None: one);
    the backward sums the parameter gradients of both uses in one reduction (modet_posenc_bwd_params_pair)."""

    @staticmethod
    def forward(ctx, x1, x2, Wt, b, alpha, tab):
        B, D, H, W, Cin = _posenc_args("posenc_pair" if x2 is not None else "posenc", x1, x2, Wt, b, alpha, tab)
        N, uses = B * D * H * W, 1 if x2 is None else 2
        ys = [None if x is None else torch.empty(x.shape[:-1] + (POSENC_DIM,), dtype=torch.float32, device=x.device) for x in (x1, x2)]
        with _Guard(x1, f"posenc_fwd[{Cin}]", uses * N * (12.0 * Cin + 18.0), 4.0 * uses * N * (Cin + POSENC_DIM)):
            _call(_L().modet_posenc_fwd_pair, _p(x1), _p(x2), _p(Wt), _p(b), _p(alpha), _p(tab), _p(ys[0]), _p(ys[1]), B, D, H, W, Cin,
                  POSENC_DIM, _stream())
        ctx.save_for_backward(x1, x2, Wt, b, alpha, tab)
        ctx.step = current_step()
        return ys[0], ys[1]

    @staticmethod
    def backward(ctx, dy1, dy2):
        x1, x2, Wt, b, alpha, tab = ctx.saved_tensors
        B, D, H, W, Cin = x1.shape
        N, uses, L = B * D * H * W, 1 if x2 is None else 2, _L()
        dy1 = dy1.contiguous()
        dy2 = None if x2 is None else dy2.contiguous()
        dims = (B, D, H, W, Cin, POSENC_DIM)
        dx1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        dx2 = torch.empty_like(x2) if (x2 is not None and ctx.needs_input_grad[1]) else None
        if dx1 is not None or dx2 is not None:
            n = (dx1 is not None) + (dx2 is not None)
            with _Guard(x1, f"posenc_bwd_data[{Cin}]", n * N * 12.0 * Cin, 4.0 * n * N * (Cin + POSENC_DIM)):
                _call(L.modet_posenc_bwd_data_pair, _p(dy1), _p(dy2), _p(Wt), _p(dx1), _p(dx2), *dims, _stream())
        ret = [None, None, None]
        if any(ctx.needs_input_grad[2:5]):
            # written straight into the step's gradient buffer where the scope hands out destinations; the launch reduces its own
            # partial rows (it does not join the scope's leaf-reduction launch: DESIGN.md 4.10)
            (dW, db, da), _, ret = _param_dsts(ctx.step, Wt, b, alpha)
            nb = L.modet_posenc_ws_bytes(*dims)
            ws = _ws(nb, x1)
            with _Guard(x1, f"posenc_bwd_params[{Cin}]", uses * N * (12.0 * Cin + 24.0), 4.0 * uses * N * (Cin + POSENC_DIM)):
                _call(L.modet_posenc_bwd_params_pair, _p(x1), _p(dy1), _p(x2), _p(dy2), _p(tab), _p(dW), _p(db), _p(da), _p(ws), nb,
                      *dims, _stream())
        return (dx1, dx2, *ret, None)


def posenc_pair(x1, x2, Wt, b, alpha, tab):
    """(layer(x1), layer(x2)) for the reference's PositionalEncodingLayer with shared parameters -- Im2Grid's q / k of a level
    ("Baseline methods/Im2Grid/models.py":360-380); tab = posenc_table(D, H, W)"""
    if x2 is None:
        raise RuntimeError("posenc_pair: x2 is missing (ops.posenc is the single-input form)")
    return _PosEncPair.apply(x1, x2, Wt, b, alpha, tab)


def posenc(x, Wt, b, alpha, tab):
    """Linear(Cin -> 6) + alpha * sinusoidal position embedding on channels-last voxels (PositionalEncodingLayer, models.py:238-274)"""
    return _PosEncPair.apply(x, None, Wt, b, alpha, tab)[0]


CONVS2_MAX_CHANNELS = 256        # MODET_CONVS2_MAX_CHANNELS of include/modet_hip_convs2.h
DECONV_MAX_CHANNELS = 1024       # MODET_DECONV_MAX_CHANNELS of include/modet_hip_deconv.h


def conv3d_s2_out_shape(D, H, W):
    """the output grid of a 3x3x3 convolution with stride 2 and padding 1: (n - 1) // 2 + 1 per axis"""
    return tuple((int(n) - 1) // 2 + 1 for n in (D, H, W))


def conv_transpose3d_k4s2_out_shape(D, H, W):
    """the output grid of a 4x4x4 transposed convolution with stride 2 and padding 1: 2 n per axis"""
    return tuple(2 * int(n) for n in (D, H, W))


class _Strided(NamedTuple):
    """One stride-2 layer family (csrc/strided.h has what their kernels share): all that differs between conv3d_s2 and
    conv_transpose3d_k4s2 on the way to the library.  _strided_args and _StridedLayer do the rest once."""
    op: str                  # the public wrapper, as the refusals name it
    tag: str                 # the kernel-timer tags are <tag>_fwd[..], <tag>_bwd_data[..], <tag>_bwd_weight[..]
    lib: str                 # the entry points are modet_<lib>_fwd, _bwd_data, _bwd_weight and _ws_bytes
    kind: str                # what a bf16 feature handle is told the kernels are
    w_shape: Callable        # (Cin, Cout) -> the weight's shape
    cout_axis: int           # the axis of w that counts output channels
    out_shape: Callable      # (D, H, W) -> the output grid
    flops: Callable          # (Cin, Cout, input voxels, output voxels) -> of one pass
    refusal: Callable        # (x, w, Cin, Cout) -> what is wrong with the channel counts or the grid, or None


def _convs2_refusal(x, w, Cin, Cout):
    if not (Cin == 1 or (Cin % 4 == 0 and Cin >= 4)) or Cin > CONVS2_MAX_CHANNELS:
        return f"x has {Cin} channels: the kernels take 1 or a multiple of 4 up to {CONVS2_MAX_CHANNELS}"
    if Cout % 4 != 0 or not 4 <= Cout <= CONVS2_MAX_CHANNELS:
        return f"weight has {Cout} output channels: the kernels take a multiple of 4 up to {CONVS2_MAX_CHANNELS}"
    if min(x.shape[:4]) < 1:
        return f"x {tuple(x.shape)} is empty"
    return None


def _deconv_refusal(x, w, Cin, Cout):
    if min(*x.shape, Cout) < 1:
        return f"x {tuple(x.shape)} or weight {tuple(w.shape)} is empty"
    if Cin > DECONV_MAX_CHANNELS:
        return f"x has {Cin} channels: the kernels take 1 to {DECONV_MAX_CHANNELS}"
    if Cout > DECONV_MAX_CHANNELS:
        return f"weight has {Cout} output channels: the kernels take 1 to {DECONV_MAX_CHANNELS}"
    return None


_CONVS2 = _Strided("conv3d_s2", "convs2", "convs2", "stride-2 convolution", lambda Cin, Cout: (Cout, Cin, 3, 3, 3), 0, conv3d_s2_out_shape,
                   lambda Cin, Cout, n_in, n_out: 54.0 * Cin * Cout * n_out, _convs2_refusal)
_DECONV = _Strided("conv_transpose3d_k4s2", "deconv", "deconv4s2", "transposed-convolution", lambda Cin, Cout: (Cin, Cout, 4, 4, 4), 1,
                   conv_transpose3d_k4s2_out_shape, lambda Cin, Cout, n_in, n_out: 128.0 * Cin * Cout * n_in, _deconv_refusal)


def _strided_args(lay, op, x, w, b, slope):
    """x (B,D,H,W,Cin); w lay.w_shape(Cin, Cout); b (Cout,) or None; slope None or a float >= 0 -> (B, D, H, W, Cin, Cout, act, slope)"""
    if getattr(x, "data16", None) is not None:
        raise RuntimeError(f"{op}: x is a bf16 feature handle; the {lay.kind} kernels are fp32 only")
    _chk(x, w, b)
    _rank5(op, "x", x)
    if w.dim() != 5:
        raise RuntimeError(f"{op}: weight must be ({','.join(map(str, lay.w_shape('Cin', 'Cout')))}), got {tuple(w.shape)}")
    B, D, H, W, Cin = x.shape
    Cout = w.shape[lay.cout_axis]
    _same_shape(op, "weight", w, lay.w_shape(Cin, Cout), f"x {tuple(x.shape)}")
    _same_shape(op, "bias", b, (Cout,), f"weight {tuple(w.shape)}")
    if slope is not None and not (isinstance(slope, (int, float)) and not isinstance(slope, bool) and slope >= 0.0):
        raise RuntimeError(f"{op}: slope must be None (no activation) or a number >= 0 (0.0: ReLU), got {slope!r}")
    why = lay.refusal(x, w, Cin, Cout)
    if why is not None:
        raise RuntimeError(f"{op}: {why}")
    if getattr(_L(), f"modet_{lay.lib}_ws_bytes")(B, D, H, W, Cin, Cout, 0) == 0:
        raise RuntimeError(f"{op}: x {tuple(x.shape)} -> {Cout} channels: a tensor of 2^31 elements or more (the kernels' limit)")
    return B, D, H, W, Cin, Cout, int(slope is not None), float(slope or 0.0)


def _convs2_args(op, x, w, b, slope):
    """x (B,D,H,W,Cin); w (Cout,Cin,3,3,3); b (Cout,) or None; slope None or a float >= 0 -> (B, D, H, W, Cin, Cout, act, slope)"""
    return _strided_args(_CONVS2, op, x, w, b, slope)


def _deconv_args(op, x, w, b, slope):
    """x (B,D,H,W,Cin); w (Cin,Cout,4,4,4); b (Cout,) or None; slope None or a float >= 0 -> (B, D, H, W, Cin, Cout, act, slope)"""
    return _strided_args(_DECONV, op, x, w, b, slope)


class _StridedLayer(Function):
    """nn.Conv3d(Cin, Cout, 3, stride=2, padding=1) or nn.ConvTranspose3d(Cin, Cout, 4, stride=2, padding=1) [+ LeakyReLU(slope)]
    on channels-last voxels, by ``lay``; the backward folds the activation's derivative into its d_y loads and skips the data
    gradient of an input that needs none (the image)."""

    @staticmethod
    def forward(ctx, lay, x, w, b, slope):
        B, D, H, W, Cin, Cout, act, sl = _strided_args(lay, lay.op, x, w, b, slope)
        L = _L()
        y = torch.empty((B, *lay.out_shape(D, H, W), Cout), dtype=torch.float32, device=x.device)
        nb = getattr(L, f"modet_{lay.lib}_ws_bytes")(B, D, H, W, Cin, Cout, 0)
        ws = _ws(nb, x)
        with _Guard(x, f"{lay.tag}_fwd[{Cin}->{Cout}]", lay.flops(Cin, Cout, B * D * H * W, y.numel() // Cout), 4.0 * (x.numel() + y.numel())):
            _call(getattr(L, f"modet_{lay.lib}_fwd"), _p(x), _p(w), _p(b), _p(y), _p(ws), nb, B, D, H, W, Cin, Cout, act, sl, _stream())
        ctx.save_for_backward(x, w, b, y if act else None)
        ctx.lay, ctx.act, ctx.slope, ctx.step = lay, act, sl, current_step()
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, y = ctx.saved_tensors
        B, D, H, W, Cin = x.shape
        lay, L = ctx.lay, _L()
        Cout = w.shape[lay.cout_axis]
        dy = dy.contiguous()
        dims = (B, D, H, W, Cin, Cout, ctx.act, ctx.slope)
        flops = lay.flops(Cin, Cout, float(x.numel() // Cin), float(dy.numel() // Cout))
        nbytes = 4.0 * (x.numel() + (1 + ctx.act) * dy.numel())
        need_x, need_w, need_b = ctx.needs_input_grad[1:4]
        dx = None
        if need_x:
            dx = torch.empty_like(x)
            nb = getattr(L, f"modet_{lay.lib}_ws_bytes")(B, D, H, W, Cin, Cout, 1)
            ws = _ws(nb, x)
            with _Guard(x, f"{lay.tag}_bwd_data[{Cout}->{Cin}]", flops, nbytes):
                _call(getattr(L, f"modet_{lay.lib}_bwd_data"), _p(dy), _p(y), _p(w), _p(dx), _p(ws), nb, *dims, _stream())
        ret = [None, None]
        if need_w or (b is not None and need_b):
            # written straight into the step's gradient buffer where the scope hands out destinations; the launch reduces its own
            # partial rows
            params = (w,) if b is None else (w, b)
            dsts, _, back = _param_dsts(ctx.step, *params)
            ret = list(back) + [None] * (2 - len(back))
            nb = getattr(L, f"modet_{lay.lib}_ws_bytes")(B, D, H, W, Cin, Cout, 2)
            ws = _ws(nb, x)
            with _Guard(x, f"{lay.tag}_bwd_weight[{Cin}->{Cout}]", flops, nbytes):
                _call(getattr(L, f"modet_{lay.lib}_bwd_weight"), _p(x), _p(dy), _p(y), _p(dsts[0]), _p(dsts[1] if b is not None else None),
                      _p(ws), nb, *dims, _stream())
        return (None, dx, ret[0], ret[1], None)


def conv3d_s2(x, w, b=None, slope=None):
    """3x3x3 convolution with stride 2 and padding 1 on channels-last voxels, then LeakyReLU(slope) (slope=None: no activation,
    0.0: ReLU) -- the ConvBlock(cin, cout, 3, 2, 1) of the RDN / PCNet / PR++ encoders ("Baseline methods/RDN/models.py":172-192).
    x (B,D,H,W,Cin) -> (B,Do,Ho,Wo,Cout), conv3d_s2_out_shape."""
    return _StridedLayer.apply(_CONVS2, x, w, b, slope)


def conv_transpose3d_k4s2(x, w, b=None, slope=None):
    """4x4x4 transposed convolution with stride 2 and padding 1 on channels-last voxels, then LeakyReLU(slope) (slope=None: no
    activation, 0.0: ReLU) -- the upsampling layer of the RCN / VTN decoder ("Baseline methods/RCN/models.py": ConvTranspose3d(4,
    stride=2) and the crop [1:-1] of every axis, the same function).  x (B,D,H,W,Cin), w (Cin,Cout,4,4,4) -> (B,2D,2H,2W,Cout)."""
    return _StridedLayer.apply(_DECONV, x, w, b, slope)


class _CatChannels(Function):
    @staticmethod
    def forward(ctx, a, b):
        for name, t in (("a", a), ("b", b)):
            if getattr(t, "data16", None) is not None:
                raise RuntimeError(f"cat_channels: {name} is a bf16 feature handle; the concatenation kernels are fp32 only")
        _chk(a, b)
        if a.dim() < 2 or b.dim() != a.dim() or tuple(a.shape[:-1]) != tuple(b.shape[:-1]):
            raise RuntimeError(f"cat_channels: a {tuple(a.shape)} and b {tuple(b.shape)} must agree in every dimension but the last")
        C1, C2 = a.shape[-1], b.shape[-1]
        N = a.numel() // max(C1, 1)
        if N < 1 or C1 < 1 or C2 < 1:
            raise RuntimeError(f"cat_channels: a {tuple(a.shape)} or b {tuple(b.shape)} is empty")
        if N * (C1 + C2) >= 2 ** 31:
            raise RuntimeError(f"cat_channels: the result {tuple(a.shape[:-1]) + (C1 + C2,)} has 2^31 elements or more (the kernels' limit)")
        out = torch.empty(tuple(a.shape[:-1]) + (C1 + C2,), dtype=torch.float32, device=a.device)
        with _Guard(a, f"cat_channels_fwd[{C1}+{C2}]", 0.0, 8.0 * out.numel()):
            _call(_L().modet_cat_channels2_fwd, _p(a), _p(b), _p(out), N, C1, C2, _stream())
        ctx.dims = (N, C1, C2, tuple(a.shape), tuple(b.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        N, C1, C2, sa, sb = ctx.dims
        dout = dout.contiguous()
        da = torch.empty(sa, dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[0] else None
        db = torch.empty(sb, dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            with _Guard(dout, f"cat_channels_bwd[{C1}+{C2}]", 0.0, 8.0 * dout.numel()):
                _call(_L().modet_cat_channels2_bwd, _p(dout), _p(da), _p(db), N, C1, C2, _stream())
        return da, db


def cat_channels(a, b):
    """torch.cat([a, b], -1) of two channels-last tensors (RDN's Estimator input, "Baseline methods/RDN/models.py":211-214: the
    reference concatenates along dim 1 of its planar layout); the backward splits the gradient"""
    return _CatChannels.apply(a, b)


def _na_args(op, C, heads, rpb, bf16):
    """head_dim of C channels in ``heads`` heads; rpb holds heads * 27 biases.  The kernels: head_dim 6 (fused), and in fp32 any
    multiple of 8 up to 128 (csrc/na.hip gen_hd_ok)."""
    heads = int(heads)
    if heads < 1 or C % heads != 0:
        raise RuntimeError(f"{op}: {C} channels do not split into {heads} heads")
    hd = C // heads
    if hd != 6 and (bf16 or hd % 8 != 0 or hd > 128):
        raise RuntimeError(f"{op}: head_dim {hd} is not supported (6" + ("" if bf16 else ", or a multiple of 8 up to 128") + ")")
    if rpb.numel() != heads * 27:
        raise RuntimeError(f"{op}: rpb {tuple(rpb.shape)} does not hold {heads} x 27 biases")
    return hd


class _NA(Function):
    @staticmethod
    def forward(ctx, q, k, rpb, heads, scale):
        _chk(q, k, rpb)
        if q.dim() != 5:
            raise RuntimeError(f"neighbourhood attention: expects channels-last (B,D,H,W,heads*head_dim) q and k, got {tuple(q.shape)}")
        if k.shape != q.shape:
            raise RuntimeError("neighbourhood attention: q and k shapes differ")
        _na_args("neighbourhood attention", q.shape[-1], heads, rpb, False)
        need_grad = any(ctx.needs_input_grad[:3])
        out, lse = _na_fwd(q, k, rpb, heads, scale, need_grad)
        if need_grad:
            ctx.save_for_backward(q, k, rpb, out, lse)
        ctx.heads, ctx.scale = heads, float(scale)
        ctx.step = current_step()
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, rpb, out, lse = ctx.saved_tensors
        (drpb,), later, ret = _param_dsts(ctx.step, rpb)
        dq, dk = _na_bwd(q, k, rpb, out, lse, dout.contiguous(), ctx.heads, ctx.scale, ctx.step, drpb, later)
        return dq, dk, ret[0], None, None


class _LevelAttnBF16(Function):
    """One pyramid level's matching step with bf16 STORAGE of its internal tensors (BASELINE.json configs[4]):
        Mw = warp(M, flow) (or M itself at the coarsest level)  ->  q = proj_ln(F), k = proj_ln(Mw)  ->  out = NA(q, k, rpb)
    as ONE autograd node, so that Mw, q and k -- which no other op reads -- live in HBM as bf16 and never cross an autograd edge
    (autograd would cast fp32 gradients arriving at a bf16 tensor; here every gradient stays fp32).  All arithmetic is the fp32
    kernels': a bf16 input is widened on load, a bf16 output rounded to nearest even on store
    (modet_warp_fwd_o16, modet_proj_ln_fwd_t, modet_na_fwd_t / _bwd_t, modet_proj_ln_bwd_pair_t).
    reference: ModeT/models.py:371-376 (projection + attention of a level), :55-67 (the warp in front of it)."""

    @staticmethod
    def forward(ctx, F, M, flow, Wt, b, gamma, beta, rpb, heads, scale, eps, tee=False):
        _chk(Wt, b, gamma, beta, rpb)
        ctx.tee = bool(tee) and flow is not None
        ctx.set_materialize_grads(False)
        ctx.step = current_step()
        ctx.beta_ref = beta                  # (only its address and shape: the key of its gradient destination)
        _rank5("level attention (bf16)", "F", F)
        B, D, H, W, Cin = F.shape
        dim = Wt.shape[0]
        _same_shape("level attention (bf16)", "M", M, F.shape, "F")
        _same_shape("level attention (bf16)", "flow", flow, (B, D, H, W, 3), f"F {tuple(F.shape)}")
        _proj_args("level attention (bf16)", Cin, Wt, b, gamma, beta)
        _na_args("level attention (bf16)", dim, heads, rpb, True)
        N = B * D * H * W
        L = _L()
        n = float(N)
        # level features handed over as fp32 handles with bf16 data (_InstNormLReLUBF16PoolSplit, features16): read the data
        # (the handles themselves own one element of storage expanded to the shape)
        Fd, Md = getattr(F, "data16", None), getattr(M, "data16", None)
        Fd = F if Fd is None else Fd
        Md = M if Md is None else Md
        _chk16(Fd, Md)
        _same_shape("level attention (bf16)", "F's bf16 data", Fd, F.shape, "F")
        _same_shape("level attention (bf16)", "M's bf16 data", Md, M.shape, "M")
        m16 = int(Md.dtype == torch.bfloat16)
        if flow is not None:
            _chk(flow)
            Mw = torch.empty(M.shape, dtype=torch.bfloat16, device=M.device)
            with _Guard(M, f"warp_fwd[C{Cin}]", n * (24.0 * Cin + 30.0), n * ((2.0 if m16 else 4.0) * Cin + 2.0 * Cin + 12.0)):
                _call(L.modet_warp_fwd_t, _p(Md), m16, _p(flow), _p(Mw), 1, B, D, H, W, Cin, _stream())
        else:
            Mw = Md
        q = torch.empty((B, D, H, W, dim), dtype=torch.bfloat16, device=F.device)
        k = torch.empty_like(q)
        for x, y in ((Fd, q), (Mw, k)):
            x16 = int(x.dtype == torch.bfloat16)
            with _Guard(F, f"proj_ln_fwd[{Cin}->{dim}]", n * (2.0 * Cin * dim + 8.0 * dim), n * ((2.0 if x16 else 4.0) * Cin + 2.0 * dim)):
                _call(L.modet_proj_ln_fwd_t, _p(x), x16, _p(Wt), _p(b), _p(gamma), _p(beta), _p(y), 1, N, Cin, dim, eps, _stream())
        need_grad = any(ctx.needs_input_grad)
        out, lse = _na_fwd(q, k, rpb, heads, scale, need_grad)
        if need_grad:
            ctx.save_for_backward(Fd, Md, flow, Mw if flow is not None else None, q, k, Wt, b, gamma, rpb, out, lse)
        ctx.heads, ctx.scale, ctx.eps = heads, float(scale), eps
        if ctx.tee:                                        # the flow's second consumer takes this alias (see _WarpTee)
            return out, flow.view_as(flow)
        return out

    @staticmethod
    def backward(ctx, dout, galias=None):
        F, M, flow, Mw, q, k, Wt, b, gamma, rpb, out, lse = ctx.saved_tensors      # (F, M: the data, fp32 or bf16)
        if dout is None:                                   # (only the alias was used)
            return None, None, galias, None, None, None, None, None, None, None, None, None
        dout = dout.contiguous()
        galias = None if galias is None else galias.contiguous()
        # the five parameter gradients straight into the flat gradient buffer when a deferred() scope offers destinations
        dsts, later, ret = _param_dsts(ctx.step, Wt, b, gamma, ctx.beta_ref, rpb)
        dq, dk = _na_bwd(q, k, rpb, out, lse, dout, ctx.heads, ctx.scale, ctx.step, dsts[4], later)
        dF, dMw = _proj_pair_bwd(F, dq, Mw if flow is not None else M, dk, Wt, b, gamma, ctx.eps, ctx.step, dsts[:4], later, typed=True)
        if flow is None:
            return (dF, dMw, None, *ret, None, None, None, None)
        dM, dflow = None, galias
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dM, dflow = _warp_bwd(M, flow, dMw, ctx.needs_input_grad[1], ctx.needs_input_grad[2], galias)
        return (dF, dM, dflow, *ret, None, None, None, None)


def level_attention_bf16(F, M, flow, Wt, b, gamma, beta, rpb, heads, scale, eps=1e-5, tee=False):
    """NA(proj_ln(F), proj_ln(warp(M, flow))) with the warped features, q and k stored as bf16 (flow None: no warp); see
    _LevelAttnBF16.  Returns the expected offset (B, D, H, W, heads * 3), fp32; with ``tee`` (and a flow) the pair
    (offset, flow): the flow's other consumer takes the returned flow and its gradient is added inside the node's warp
    backward kernel (as ops.warp_tee)."""
    return _LevelAttnBF16.apply(F, M, flow, Wt, b, gamma, beta, rpb, heads, scale, eps, tee)


class _Corr3d(Function):
    @staticmethod
    def forward(ctx, mov, fix):
        _chk(mov, fix)
        if mov.dim() != 5:
            raise RuntimeError(f"correlation3d: expects channels-last (B,D,H,W,C) features, got {tuple(mov.shape)}")
        B, D, H, W, C = mov.shape
        if fix.shape != mov.shape:
            raise RuntimeError("correlation3d: mov and fix shapes differ")
        L = _L()
        corr = torch.empty((B, 27, D, H, W), dtype=torch.float32, device=mov.device)
        nb = L.modet_corr3d_ws_bytes(B, D, H, W, C)
        ws = _ws(nb, mov)
        n = float(B) * D * H * W
        with _Guard(mov, f"corr3d_fwd[C{C}]", n * C * (54.0 + 54.0), 4.0 * n * (2 * C + 27)):
            _call(L.modet_corr3d_fwd, _p(mov), _p(fix), _p(corr), _p(ws), nb, B, D, H, W, C, _stream())
        ctx.save_for_backward(mov, fix)
        return corr

    @staticmethod
    def backward(ctx, dcorr):
        mov, fix = ctx.saved_tensors
        dcorr = dcorr.contiguous()
        B, D, H, W, C = mov.shape
        L = _L()
        dmov, dfix = torch.empty_like(mov), torch.empty_like(fix)
        nb = L.modet_corr3d_ws_bytes(B, D, H, W, C)
        ws = _ws(nb, mov)
        n = float(B) * D * H * W
        with _Guard(mov, f"corr3d_bwd[C{C}]", n * C * 4 * 54.0, 4.0 * n * (4 * C + 27)):
            _call(L.modet_corr3d_bwd, _p(mov), _p(fix), _p(dcorr), _p(dmov), _p(dfix), _p(ws), nb, B, D, H, W, C, _stream())
        return dmov, dfix


def correlation3d(mov, fix):
    """PR++ Correlation3D on channels-last features (B,D,H,W,C) -> (B,27,D,H,W); see csrc/corr3d.hip"""
    return _Corr3d.apply(mov, fix)


def neighbourhood_attention(q, k, rpb, heads, scale):
    """Fused ModeTransformer.forward: (B,D,H,W,heads*6) x2 -> (B,D,H,W,heads*3).  reference: models.py:308-334"""
    return _NA.apply(q, k, rpb.contiguous(), heads, scale)


def _warp_fwd(src, flow, mode=0, add_flow=0):
    """THE fp32 warp forward launch, with its argument checks"""
    _chk(src, flow)
    _rank5("warp", "src", src)
    B, D, H, W, C = src.shape
    if tuple(flow.shape) != (B, D, H, W, 3):
        raise RuntimeError(f"warp: flow {tuple(flow.shape)} does not match src {tuple(src.shape)}")
    out = torch.empty_like(src)
    n = float(B) * D * H * W                # 4*(2C+3) B per voxel
    with _Guard(src, f"warp_fwd[C{C}]", n * (24.0 * C + 30.0), 4.0 * n * (2 * C + 3)):
        _call(_L().modet_warp_fwd, _p(src), _p(flow), _p(out), B, D, H, W, C, mode, int(add_flow), _stream())
    return out


class _Warp(Function):
    @staticmethod
    def forward(ctx, src, flow, mode, add_flow, flow_bound=0):
        out = _warp_fwd(src, flow, mode, add_flow)
        ctx.save_for_backward(src, flow)
        ctx.mode, ctx.add_flow, ctx.flow_bound = mode, int(add_flow), int(flow_bound)
        return out

    @staticmethod
    def backward(ctx, dout):
        src, flow = ctx.saved_tensors
        if ctx.mode != 0:
            raise RuntimeError("warp: nearest mode is not differentiable")
        dsrc, dflow = _warp_bwd(src, flow, dout.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1], None, ctx.add_flow,
                                ctx.flow_bound if src.shape[-1] == 3 else 0)
        return dsrc, dflow, None, None, None


# Deterministic warp backward (opt-in; modet_warp_bwd_det): d_src through 64-bit fixed-point integer atomics instead of float
# atomics -- bit-identical from run to run, and so is the whole train step (the warp scatter holds its only atomics).
DETERMINISTIC = os.environ.get("MODET_DETERMINISTIC", "0") == "1"


def set_deterministic(on=True):
    """run-to-run bit-identical gradients (costs ~0.3 ms per 160x192x160 train step: profiles/r05z_deterministic_fullsize.txt);
    returns the previous setting"""
    global DETERMINISTIC
    prev, DETERMINISTIC = DETERMINISTIC, bool(on)
    return prev


# The feature warps' backward by destination tiles (csrc/warp_tile.hip): integer sums in an LDS window instead of float atomics on
# global memory.  Round 5 built it (off: break-even in the step); round 6 rebuilt it (payload lists, zero-d_out entries dropped
# while binning, d_flow in the fill pass) and made it the default: faster AND bit-reproducible, so the plain step has no float
# atomics left and set_deterministic() costs nothing for these warps.  WARP_TILES = False brings the float-atomic kernel back
# (tools/ A/B runs).
WARP_TILES = True


def _warp_bwd_kind(src, dout, dsrc, add_flow, flow_bound):
    """THE choice of a warp backward's kernels, for the launch and for its tag -> (kind, workspace bytes):
    'tiles'  destination tiles (feature warps: C % 8 == 0, and the fp32 C == 3 warps; d_src wanted, fp32 d_out)
    'det'    deterministic mode, d_src of another channel count: 64-bit integer atomics on global memory
    'acc'    the float-atomic kernel -- with flow_bound (C == 3) its d_src is a gather without atomics"""
    B, D, H, W, C = src.shape
    if dsrc is not None and not flow_bound:
        if (WARP_TILES and (C == 3 or not add_flow) and not (C == 3 and src.dtype == torch.bfloat16)
                and dout.dtype == torch.float32):
            nb = _L().modet_warp_bwd_dsrc_tiles_ws_bytes(B, D, H, W, C)
            if nb:
                return "tiles", nb
        if DETERMINISTIC:
            return "det", _L().modet_warp_bwd_det_ws_bytes(B, D, H, W, C)
    return "acc", 0


def _warp_bwd_tag(src, dout, dsrc, add_flow, flow_bound):
    """launch tag of a warp backward = the kernels that run (bench.py maps tags to kernel families); like _conv_tag only
    evaluated while a timer is installed"""
    if _TIMER is None:
        return None
    C = src.shape[-1]
    kind, _ = _warp_bwd_kind(src, dout, dsrc, add_flow, flow_bound)
    if kind == "tiles":
        return f"warp_bwd_tiles[C{C}]"
    return "warp_bwd_gather3[C3]" if C == 3 and flow_bound else f"warp_bwd[C{C}]"


def _warp_backward(src, flow, dout, dsrc, dflow, galias, add_flow, flow_bound):
    """launch the warp backward _warp_bwd_kind chooses; galias = a second flow gradient added on the way out"""
    B, D, H, W, C = src.shape
    L = _L()
    s16 = _isbf(src)
    kind, nb = _warp_bwd_kind(src, dout, dsrc, add_flow, flow_bound)
    if kind == "tiles":
        ws = _ws(nb, src)
        if dflow is not None:
            _call(L.modet_warp_bwd_tiles, _p(src), s16, _p(flow), _p(dout), _p(dsrc), _p(dflow), _p(galias), _p(ws), nb, B, D, H, W, C,
                  int(add_flow), _stream())
        else:
            _call(L.modet_warp_bwd_dsrc_tiles, _p(flow), _p(dout), _p(dsrc), _p(ws), nb, B, D, H, W, C, _stream())
        return
    galias = galias if dflow is not None else None
    if kind == "det":
        ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=src.device)
        _call(L.modet_warp_bwd_det, _p(src), s16, _p(flow), _p(dout), _p(dsrc), _p(dflow), _p(galias), _p(ws), nb, B, D, H, W, C,
              int(add_flow), _stream())
        return
    _call(L.modet_warp_bwd_acc, _p(src), s16, _p(flow), _p(dout), _p(dsrc), _p(dflow), _p(galias), B, D, H, W, C, int(add_flow),
          int(flow_bound), _stream())


def _warp_bwd(src, flow, dout, want_src, want_flow, galias=None, add_flow=0, flow_bound=0, alias_counted=False):
    """THE bracket of a warp backward: gradient buffers, tag, figures and launch -> (d_src, d_flow), each None when not wanted.
    alias_counted: the byte figure includes reading galias (_WarpTee's does, the level node's never did)"""
    B, D, H, W, C = src.shape
    dsrc = torch.empty(src.shape, dtype=torch.float32, device=src.device) if want_src else None
    dflow = torch.empty_like(flow) if want_flow else None
    n = float(B) * D * H * W
    with _Guard(src, _warp_bwd_tag(src, dout, dsrc, add_flow, flow_bound), n * (60.0 * C + 40.0),
                4.0 * n * (3 * C + 6 + (3 if alias_counted and galias is not None else 0))):
        _warp_backward(src, flow, dout, dsrc, dflow, galias, add_flow, flow_bound)
    return dsrc, dflow


class _WarpTee(Function):
    """warp(src, flow) for a flow that has a SECOND consumer: returns (out, flow_alias) -- the other consumer takes the alias.
    In the backward pass the other consumer's gradient arrives here (it ran later in the forward pass, so its backward ran
    first) and the warp kernel adds it while writing its own d_flow (modet_warp_bwd_acc): one pass instead of the
    element-wise add autograd would launch over two full-size tensors."""

    @staticmethod
    def forward(ctx, src, flow):
        out = _warp_fwd(src, flow)
        ctx.save_for_backward(src, flow)
        ctx.set_materialize_grads(False)
        return out, flow.view_as(flow)

    @staticmethod
    def backward(ctx, dout, galias):
        src, flow = ctx.saved_tensors
        if dout is None:
            return None, galias
        dout = dout.contiguous()
        galias = None if galias is None else galias.contiguous()
        return _warp_bwd(src, flow, dout, ctx.needs_input_grad[0], ctx.needs_input_grad[1], galias, alias_counted=True)


def warp_tee(src, flow):
    """(warp(src, flow), flow) for a flow with a second consumer, which must take the RETURNED flow; see _WarpTee"""
    return _WarpTee.apply(src, flow)


def cat_batch(a, b):
    """torch.cat([a, b], 0) -- without the copy when the two are adjacent halves of one buffer (engine.Trainer's static input
    buffer of a captured step: the [moving; fixed] batch of the shared encoder then costs nothing)"""
    if (a.shape == b.shape and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel() and not a.requires_grad and not b.requires_grad):
        return torch.as_strided(a, (2 * a.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())
    return torch.cat([a, b], 0)


def warp(src, flow, mode=0, add_flow=False, flow_bound=0):
    """SpatialTransformer on channels-last tensors; add_flow -> warp(src,flow)+flow.  reference: models.py:25-67.
    flow_bound=1 promises |flow| <= 1 voxel (attention outputs): the backward then gathers d_src without atomics."""
    return _Warp.apply(src, flow, mode, add_flow, flow_bound)


class _Upsample2(Function):
    @staticmethod
    def forward(ctx, x, scale):
        _chk(x)
        _rank5("upsample2", "x", x)
        B, d, h, w, C = x.shape
        y = torch.empty((B, 2 * d, 2 * h, 2 * w, C), dtype=torch.float32, device=x.device)
        with _Guard(x, f"upsample2_fwd[C{C}]", 16.0 * y.numel(), 4.0 * (x.numel() + y.numel())):
            _call(_L().modet_upsample2_fwd, _p(x), _p(y), B, d, h, w, C, float(scale), _stream())
        ctx.shape, ctx.scale = (B, d, h, w, C), float(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        B, d, h, w, C = ctx.shape
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        L = _L()
        nb = L.modet_upsample2_bwd_sep_ws_bytes(B, d, h, w, C)       # > 0: large level, three 1-D passes
        ws = _ws(nb, dy) if nb else None
        with _Guard(dy, f"upsample2_bwd[C{C}]", 16.0 * dy.numel(), 4.0 * (dx.numel() + dy.numel())):
            if nb:
                _call(L.modet_upsample2_bwd_sep, _p(dy), _p(dx), _p(ws), nb, B, d, h, w, C, ctx.scale, _stream())
            else:
                _call(L.modet_upsample2_bwd, _p(dy), _p(dx), B, d, h, w, C, ctx.scale, _stream())
        return dx, None


def upsample2(x, scale=1.0):
    """scale * Upsample(x2, trilinear, align_corners=True), channels-last.  reference: models.py:354,:257-261"""
    return _Upsample2.apply(x, scale)


class _CwmTail(Function):
    @staticmethod
    def forward(ctx, x, logits):
        _chk(x, logits)
        heads = logits.shape[-1]
        _same_shape("cwm_tail", "x", x, tuple(logits.shape[:-1]) + (heads * 3,), f"logits {tuple(logits.shape)}: heads * 3 channels")
        N = logits.numel() // heads
        out = torch.empty(logits.shape[:-1] + (3,), dtype=torch.float32, device=x.device)
        with _Guard(x, "cwm_tail_fwd", 12.0 * x.numel(), 4.0 * (x.numel() + logits.numel() + out.numel())):
            _call(_L().modet_cwm_tail_fwd, _p(x), _p(logits), _p(out), N, heads, _stream())
        ctx.save_for_backward(x, logits)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, logits = ctx.saved_tensors
        dout = dout.contiguous()
        heads = logits.shape[-1]
        N = logits.numel() // heads
        dx, dl = torch.empty_like(x), torch.empty_like(logits)
        with _Guard(x, "cwm_tail_bwd", 20.0 * x.numel(), 8.0 * (x.numel() + logits.numel()) + 4.0 * dout.numel()):
            _call(_L().modet_cwm_tail_bwd, _p(x), _p(logits), _p(dout), _p(dx), _p(dl), N, heads, _stream())
        return dx, dl


def cwm_tail(x, logits):
    """2 * sum_h softmax_h(logits) * x[..., 3h:3h+3].  reference: CWM.forward, models.py:263-275"""
    return _CwmTail.apply(x, logits)


# ---- the PCNet family (include/modet_hip_pcnet.h): upsampling by 2 / 4 / 8 into a slice of a row, DFI's gated sum, the NFF tail
_UP_FACTORS, _UP_ROWS = (2, 4, 8), (3, 6, 9)


def _up_args(op, x, f, out, offset):
    _chk(x, out)
    _rank5(op, "x", x)
    B, d, h, w, C = x.shape
    if C != 3:
        raise RuntimeError(f"{op}: x {tuple(x.shape)} must have 3 channels (a displacement field)")
    if f not in _UP_FACTORS:
        raise RuntimeError(f"{op}: f must be one of {_UP_FACTORS}, got {f!r}")
    if B < 1 or min(d, h, w) < 2:
        raise RuntimeError(f"{op}: x {tuple(x.shape)} needs a batch and at least 2 voxels along every axis (align_corners=True has "
                           "no scale for an axis of 1)")
    ld = 3 if out is None else (out.shape[-1] if out.dim() == 5 else -1)
    if out is not None:
        if ld not in _UP_ROWS:
            raise RuntimeError(f"{op}: out {tuple(out.shape)} must be channels-last with 3, 6 or 9 channels")
        _same_shape(op, "out", out, (B, f * d, f * h, f * w, ld), f"x {tuple(x.shape)} upsampled by {f}")
    elif offset != 0:
        raise RuntimeError(f"{op}: offset {offset!r} needs an out tensor to index")
    if not isinstance(offset, int) or offset < 0 or offset + 3 > ld:
        raise RuntimeError(f"{op}: offset {offset!r} does not leave 3 channels in a row of {ld}")
    if B * d * h * w * f ** 3 * ld >= 2 ** 31:
        raise RuntimeError(f"{op}: the result of x {tuple(x.shape)} upsampled by {f} has 2^31 elements or more (the kernels' limit)")
    return B, d, h, w, ld


class _UpsamplePow2(Function):
    """out is written in place in its channels [offset, offset + 3) and returned: autograd sees a fresh view of it per call, so
    the three upsamplings of a DFI block chain through the one buffer and each backward reads its own slice of the gradient"""

    @staticmethod
    def forward(ctx, x, f, out, offset):
        B, d, h, w, ld = _up_args("upsample_pow2", x, f, out, offset)
        y = out if out is not None else torch.empty((B, f * d, f * h, f * w, 3), dtype=torch.float32, device=x.device)
        nfine = B * d * h * w * f ** 3
        with _Guard(x, f"upsample_pow2_fwd[x{f}]", 3.0 * 14.0 * nfine, 4.0 * (x.numel() + 3.0 * nfine)):
            _call(_L().modet_pcnet_upsample_fwd, _p(x), _p(y), B, d, h, w, f, ld, offset, _stream())
        if out is not None:
            ctx.mark_dirty(out)
        ctx.dims = (B, d, h, w, f, ld, offset)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, d, h, w, f, ld, offset = ctx.dims
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((B, d, h, w, 3), dtype=torch.float32, device=dy.device)
            nfine = B * d * h * w * f ** 3
            with _Guard(dy, f"upsample_pow2_bwd[x{f}]", 8.0 * 6.0 * nfine, 4.0 * (dx.numel() + 3.0 * nfine)):
                _call(_L().modet_pcnet_upsample_bwd, _p(dy), _p(dx), B, d, h, w, f, ld, offset, _stream())
        # the rows' other channels belong to the calls before this one: their gradient passes through; this call's slice was overwritten
        dprev = None
        if ctx.needs_input_grad[2]:
            dprev = torch.empty_like(dy)
            dprev.copy_(dy)
            dprev[..., offset:offset + 3] = 0
        return dx, None, dprev, None


def upsample_pow2(x, f, out=None, offset=0):
    """nn.Upsample(scale_factor=f, mode='trilinear', align_corners=True) of a channels-last 3-channel field, f in (2, 4, 8):
    DFIBlock.upsample ("Baseline methods/PCnet/models.py":247-256).  With ``out`` (B,fd,fh,fw,ld), ld in (3, 6, 9), the result is
    written into channels [offset, offset + 3) of it and ``out`` is returned (the torch.cat of DFIBlock.forward without a
    concatenation kernel); the other channels are left untouched."""
    return _UpsamplePow2.apply(x, f, out, offset)


class _DfiGate(Function):
    @staticmethod
    def forward(ctx, x, logits):
        _chk(x, logits)
        if x.dim() < 2 or x.shape[-1] not in (3, 6, 9):
            raise RuntimeError(f"dfi_gate: x {tuple(x.shape)} must end in 3, 6 or 9 channels (n fields of 3)")
        _same_shape("dfi_gate", "logits", logits, tuple(x.shape), "x")
        n = x.shape[-1] // 3
        N = x.numel() // (3 * n)
        if N < 1:
            raise RuntimeError(f"dfi_gate: x {tuple(x.shape)} is empty")
        out = torch.empty(tuple(x.shape[:-1]) + (3,), dtype=torch.float32, device=x.device)
        with _Guard(x, f"dfi_gate_fwd[n{n}]", 8.0 * x.numel(), 4.0 * (2 * x.numel() + out.numel())):
            _call(_L().modet_pcnet_dfi_gate_fwd, _p(x), _p(logits), _p(out), N, n, _stream())
        ctx.save_for_backward(x, logits)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, logits = ctx.saved_tensors
        dout = dout.contiguous()
        n = x.shape[-1] // 3
        N = x.numel() // (3 * n)
        dx, dl = torch.empty_like(x), torch.empty_like(logits)
        with _Guard(x, f"dfi_gate_bwd[n{n}]", 12.0 * x.numel(), 4.0 * (4 * x.numel() + dout.numel())):
            _call(_L().modet_pcnet_dfi_gate_bwd, _p(x), _p(logits), _p(dout), _p(dx), _p(dl), N, n, _stream())
        return dx, dl


def dfi_gate(x, logits):
    """sum_i x[..., 3i:3i+3] * sigmoid(logits[..., 3i:3i+3]) over the n = C / 3 fields of x (..., 3n), n in (1, 2, 3): the weighted
    sum of DFIBlock.forward ("Baseline methods/PCnet/models.py":261-267) in one pass; the backward recomputes the sigmoid"""
    return _DfiGate.apply(x, logits)


def _nff_args(op, t0, t1, t2, logits, W1, W2):
    _chk(t0, t1, t2, logits, W1, W2)
    _rank5(op, "t0", t0)
    B, D, H, W, C = t0.shape
    _same_shape(op, "t1", t1, tuple(t0.shape), "t0")
    _same_shape(op, "t2", t2, tuple(t0.shape), "t0")
    _same_shape(op, "logits", logits, (B, D, H, W, 3), f"t0 {tuple(t0.shape)}: one logit per map and voxel")
    V = D * H * W
    if B < 1 or V < 1:
        raise RuntimeError(f"{op}: t0 {tuple(t0.shape)} is empty")
    if _L().modet_pcnet_nff_ws_bytes(B, V, C, 0) == 0:
        raise RuntimeError(f"{op}: t0 {tuple(t0.shape)}: the kernels take a channel count that is a multiple of 4 from 4 to "
                           f"{_lib_limit('MODET_PCNET_MAX_C')}, up to 65535 samples and fewer than 2^31 voxels per sample")
    _same_shape(op, "W1", W1, (3 * C // 8, 3 * C), f"t0 {tuple(t0.shape)}: (3C // 8, 3C)")
    _same_shape(op, "W2", W2, (3 * C, 3 * C // 8), f"t0 {tuple(t0.shape)}: (3C, 3C // 8)")
    return B, V, C


def _lib_limit(name):
    """an enum constant of include/modet_hip_pcnet.h, read from the header the library was built from"""
    import re
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, open(_lib.FAMILIES["pcnet"][0]).read())
    return int(m.group(1))


class _NffFuse(Function):
    """pool -> gate -> apply in one node; the concatenation is never stored: the backward forms it again from the inputs"""

    @staticmethod
    def forward(ctx, t0, t1, t2, logits, W1, W2):
        B, V, C = _nff_args("nff_fuse", t0, t1, t2, logits, W1, W2)
        L, dev = _L(), t0.device
        avg, mx, g = (torch.empty((B, 3 * C), dtype=torch.float32, device=dev) for _ in range(3))
        arg = torch.empty((B, 3 * C), dtype=torch.int32, device=dev)
        out = torch.empty(tuple(t0.shape[:-1]) + (3 * C,), dtype=torch.float32, device=dev)
        nb = L.modet_pcnet_nff_ws_bytes(B, V, C, 0)
        ws = _ws(nb, t0)
        nin = 3.0 * t0.numel() + logits.numel()
        with _Guard(t0, f"nff_pool[C{C}]", 3.0 * 3 * t0.numel(), 4.0 * nin):
            _call(L.modet_pcnet_nff_pool, _p(t0), _p(t1), _p(t2), _p(logits), _p(avg), _p(mx), _p(arg), _p(ws), nb, B, V, C, _stream())
        with _Guard(t0, f"nff_gate_fwd[C{C}]", 4.0 * B * 3 * C * (3 * C // 8) * 2, 4.0 * 2 * W1.numel()):
            _call(L.modet_pcnet_nff_gate_fwd, _p(avg), _p(mx), _p(W1), _p(W2), _p(g), B, C, _stream())
        with _Guard(t0, f"nff_apply_fwd[C{C}]", 2.0 * 3 * t0.numel(), 4.0 * (nin + out.numel())):
            _call(L.modet_pcnet_nff_apply_fwd, _p(t0), _p(t1), _p(t2), _p(logits), _p(g), _p(out), B, V, C, _stream())
        ctx.save_for_backward(t0, t1, t2, logits, W1, W2, avg, mx, arg, g)
        ctx.dims = (B, V, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        t0, t1, t2, logits, W1, W2, avg, mx, arg, g = ctx.saved_tensors
        B, V, C = ctx.dims
        L, dev = _L(), t0.device
        dout = dout.contiguous()
        need = ctx.needs_input_grad
        need_w = need[4] or need[5]
        if not any(need):
            return (None,) * 6
        nin = 3.0 * t0.numel() + logits.numel()
        dg, davg, dmx = (torch.empty((B, 3 * C), dtype=torch.float32, device=dev) for _ in range(3))
        nb = L.modet_pcnet_nff_ws_bytes(B, V, C, 1)
        ws = _ws(nb, t0)
        with _Guard(t0, f"nff_apply_bwd_gate[C{C}]", 3.0 * 3 * t0.numel(), 4.0 * (nin + dout.numel())):
            _call(L.modet_pcnet_nff_apply_bwd_gate, _p(t0), _p(t1), _p(t2), _p(logits), _p(dout), _p(dg), _p(ws), nb, B, V, C, _stream())
        dW1 = torch.empty_like(W1) if need_w else None
        dW2 = torch.empty_like(W2) if need_w else None
        nb = L.modet_pcnet_nff_ws_bytes(B, V, C, 2)
        ws = _ws(nb, t0)
        with _Guard(t0, f"nff_gate_bwd[C{C}]", 8.0 * B * 3 * C * (3 * C // 8) * 2, 4.0 * 4 * W1.numel()):
            _call(L.modet_pcnet_nff_gate_bwd, _p(avg), _p(mx), _p(W1), _p(W2), _p(g), _p(dg), _p(davg), _p(dmx), _p(dW1), _p(dW2),
                  _p(ws), nb, B, C, _stream())
        grads = [torch.empty_like(t) if n else None for t, n in zip((t0, t1, t2, logits), need[:4])]
        if any(n for n in need[:4]):
            nout = sum(t.numel() for t in grads if t is not None)
            with _Guard(t0, f"nff_apply_bwd[C{C}]", 6.0 * 3 * t0.numel(), 4.0 * (nin + dout.numel() + nout)):
                _call(L.modet_pcnet_nff_apply_bwd, _p(t0), _p(t1), _p(t2), _p(logits), _p(dout), _p(g), _p(davg), _p(dmx), _p(arg),
                      *(_p(t) for t in grads), B, V, C, _stream())
        return (*grads, dW1 if need[4] else None, dW2 if need[5] else None)


def nff_fuse(t0, t1, t2, logits, W1, W2):
    """The tail of NFFBlock.forward ("Baseline methods/PCnet/models.py":316-322, 285-292): w = softmax(logits) over its 3 entries,
    cat = [t0 w0, t1 w1, t2 w2] along the channels, g = sigmoid(fc(avgpool(cat)) + fc(maxpool(cat))) with fc = W2 relu(W1 .),
    returns cat * g, (B,D,H,W,3C).  t_k (B,D,H,W,C), logits (B,D,H,W,3), W1 (3C // 8, 3C), W2 (3C, 3C // 8)."""
    return _NffFuse.apply(t0, t1, t2, logits, W1, W2)


def residual_add(a, b):
    """a + b elementwise in one kernel (ResBlock's ``self.block(x) + x``); autograd's own accumulation carries the gradient to
    both addends"""
    return _ResidualAdd.apply(a, b)


class _ResidualAdd(Function):
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, b)
        _same_shape("residual_add", "b", b, tuple(a.shape), "a")
        if a.numel() < 1:
            raise RuntimeError(f"residual_add: a {tuple(a.shape)} is empty")
        s = torch.empty_like(a)
        with _Guard(a, "residual_add", float(a.numel()), 12.0 * a.numel()):
            _call(_L().modet_pcnet_add, _p(a), _p(b), _p(s), a.numel(), _stream())
        return s

    @staticmethod
    def backward(ctx, ds):
        return ds, ds


# ------------------------------------------------------------------------------------------------ the PR++ family
PRPP_CORR = 27                   # MODET_PRPP_CORR of include/modet_hip_prpp.h: the correlation channels of a stack row


def _prpp_limit(name):
    """an enum constant of include/modet_hip_prpp.h, read from the header the library was built from"""
    import re
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, open(_lib.FAMILIES["prpp"][0]).read()).group(1))


class _UpsampleNearestCat(Function):
    @staticmethod
    def forward(ctx, x, skip):
        op = "upsample_nearest_cat"
        _chk(x, skip)
        _rank5(op, "x", x)
        _rank5(op, "skip", skip)
        B, d, h, w, C1 = x.shape
        C2 = skip.shape[-1]
        if B < 1 or min(d, h, w, C1, C2) < 1:
            raise RuntimeError(f"{op}: x {tuple(x.shape)} or skip {tuple(skip.shape)} is empty")
        _same_shape(op, "skip", skip, (B, 2 * d, 2 * h, 2 * w, C2), f"x {tuple(x.shape)} upsampled by 2")
        out = torch.empty((B, 2 * d, 2 * h, 2 * w, C1 + C2), dtype=torch.float32, device=x.device)
        with _Guard(x, f"upcat_fwd[{C1}+{C2}]", 0.0, 4.0 * (x.numel() + skip.numel() + out.numel())):
            _call(_L().modet_prpp_upcat_fwd, _p(x), _p(skip), _p(out), B, d, h, w, C1, C2, _stream())
        ctx.dims = (B, d, h, w, C1, C2)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, d, h, w, C1, C2 = ctx.dims
        dout = dout.contiguous()
        dx = torch.empty((B, d, h, w, C1), dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[0] else None
        ds = torch.empty((B, 2 * d, 2 * h, 2 * w, C2), dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[1] else None
        if dx is not None or ds is not None:
            nout = sum(t.numel() for t in (dx, ds) if t is not None)
            with _Guard(dout, f"upcat_bwd[{C1}+{C2}]", 7.0 * (0 if dx is None else dx.numel()), 4.0 * (dout.numel() + nout)):
                _call(_L().modet_prpp_upcat_bwd, _p(dout), _p(dx), _p(ds), B, d, h, w, C1, C2, _stream())
        return dx, ds


def upsample_nearest_cat(x, skip):
    """torch.cat([nn.Upsample(scale_factor=2)(x), skip], channels) of channels-last x (B,d,h,w,C1) and skip (B,2d,2h,2w,C2) in one
    pass: DecoderBlock.forward before its convolution ("Baseline methods/PR++/models.py":150-160); the backward gathers d_x"""
    return _UpsampleNearestCat.apply(x, skip)


class _Relu(Function):
    @staticmethod
    def forward(ctx, t):
        _chk(t)
        if t.numel() < 1:
            raise RuntimeError(f"relu: t {tuple(t.shape)} is empty")
        y = torch.empty_like(t)
        with _Guard(t, "relu_fwd", float(t.numel()), 8.0 * t.numel()):
            _call(_L().modet_prpp_relu_fwd, _p(t), _p(y), t.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dt = torch.empty_like(dy)
        with _Guard(dy, "relu_bwd", float(dy.numel()), 12.0 * dy.numel()):
            _call(_L().modet_prpp_relu_bwd, _p(dy), _p(y), _p(dt), dy.numel(), _stream())
        return dt


def relu(t):
    """max(t, 0) (nn.ReLU of the PR++ ConvBlock and blocks); the gradient at 0 is 0"""
    return _Relu.apply(t)


class _ReluAdd(Function):
    @staticmethod
    def forward(ctx, x, t):
        _chk(x, t)
        _same_shape("relu_add", "t", t, tuple(x.shape), "x")
        if x.numel() < 1:
            raise RuntimeError(f"relu_add: x {tuple(x.shape)} is empty")
        out = torch.empty_like(x)
        with _Guard(x, "relu_add_fwd", 2.0 * x.numel(), 12.0 * x.numel()):
            _call(_L().modet_prpp_relu_add_fwd, _p(x), _p(t), _p(out), x.numel(), _stream())
        ctx.save_for_backward(t)
        return out

    @staticmethod
    def backward(ctx, dout):
        (t,) = ctx.saved_tensors
        dt = None
        if ctx.needs_input_grad[1]:
            dout = dout.contiguous()
            dt = torch.empty_like(dout)
            with _Guard(dout, "relu_bwd", float(dout.numel()), 12.0 * dout.numel()):
                _call(_L().modet_prpp_relu_bwd, _p(dout), _p(t), _p(dt), dout.numel(), _stream())
        return dout, dt          # d_x is d_out itself: autograd accumulates it (as residual_add)


def relu_add(x, t):
    """x + max(t, 0) in one pass: ``x + res`` of PRplusplusBlock.forward with conv2's trailing ReLU ("Baseline methods/PR++/
    models.py":261-281)"""
    return _ReluAdd.apply(x, t)


def _stack_args(op, mov, fix):
    _chk(mov, fix)
    _rank5(op, "mov", mov)
    _same_shape(op, "fix", fix, tuple(mov.shape), "mov")
    B, D, H, W, C = mov.shape
    if B < 1 or min(D, H, W) < 1:
        raise RuntimeError(f"{op}: mov {tuple(mov.shape)} is empty")
    nb = _L().modet_prpp_stack_ws_bytes(B, D, H, W, C)
    if nb == 0:
        raise RuntimeError(f"{op}: mov {tuple(mov.shape)}: the kernels take a channel count that is a multiple of 4 from 4 to "
                           f"{_prpp_limit('MODET_PRPP_MAX_C')} and fewer than 2^31 elements on the grid extended by one voxel")
    return B, D, H, W, C, nb


class _CorrStack(Function):
    @staticmethod
    def forward(ctx, mov, fix):
        B, D, H, W, C, nb = _stack_args("corr_stack", mov, fix)
        out = torch.empty((B, D, H, W, 2 * C + PRPP_CORR), dtype=torch.float32, device=mov.device)
        ws = _ws(nb, mov)
        n = float(B) * D * H * W
        with _Guard(mov, f"corr_stack_fwd[C{C}]", n * C * (54.0 + 54.0), 4.0 * n * (4 * C + 27)):
            _call(_L().modet_prpp_stack_fwd, _p(mov), _p(fix), _p(out), _p(ws), nb, B, D, H, W, C, _stream())
        ctx.save_for_backward(mov, fix)
        ctx.nb = nb
        return out

    @staticmethod
    def backward(ctx, dout):
        mov, fix = ctx.saved_tensors
        B, D, H, W, C = mov.shape
        dout = dout.contiguous()
        dmov = torch.empty_like(mov) if ctx.needs_input_grad[0] else None
        dfix = torch.empty_like(fix) if ctx.needs_input_grad[1] else None
        if dmov is not None or dfix is not None:
            ws = _ws(ctx.nb, mov)
            n = float(B) * D * H * W
            with _Guard(mov, f"corr_stack_bwd[C{C}]", n * C * 4 * 54.0, 4.0 * n * (6 * C + 27)):
                _call(_L().modet_prpp_stack_bwd, _p(mov), _p(fix), _p(dout), _p(dmov), _p(dfix), _p(ws), ctx.nb, B, D, H, W, C, _stream())
        return dmov, dfix


def corr_stack(mov, fix):
    """torch.cat([mov, Correlation3D(mov, fix), fix], channels) of channels-last features (B,D,H,W,C) -> (B,D,H,W,2C+27): the stack
    of PRplusplusBlock.forward ("Baseline methods/PR++/models.py":276-278) in one row, the correlation by correlation3d's kernels"""
    return _CorrStack.apply(mov, fix)


def _compose_args(op, src, w):
    _chk(src, w)
    _rank5(op, "src", src)
    _rank5(op, "w", w)
    if src.shape[-1] != 3 or w.shape[-1] != 3 or src.shape[0] != w.shape[0]:
        raise RuntimeError(f"{op}: src {tuple(src.shape)} and w {tuple(w.shape)} must be 3-channel fields of one batch")
    if src.shape[0] < 1 or min(src.shape[1:4]) < 1 or min(w.shape[1:4]) < 2:
        raise RuntimeError(f"{op}: src {tuple(src.shape)} needs a voxel and w {tuple(w.shape)} two voxels along every axis "
                           "(align_corners=True has no scale for an axis of 1)")
    return (src.shape[0],) + tuple(src.shape[1:4]) + tuple(w.shape[1:4])


class _ComposeCross(Function):
    @staticmethod
    def forward(ctx, src, w):
        dims = _compose_args("compose_cross", src, w)
        out = torch.empty_like(w)
        n = float(w.numel() // 3)
        with _Guard(w, "compose_cross_fwd", n * 102.0, 4.0 * (src.numel() + 2 * w.numel())):
            _call(_L().modet_prpp_compose_fwd, _p(src), _p(w), _p(out), *dims, _stream())
        ctx.save_for_backward(src, w)
        ctx.dims = dims
        return out

    @staticmethod
    def backward(ctx, dout):
        src, w = ctx.saved_tensors
        dout = dout.contiguous()
        dsrc = torch.empty_like(src) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        if dsrc is None and dw is None:
            return None, None
        L = _L()
        nb = L.modet_prpp_compose_ws_bytes(*ctx.dims[:4]) if dsrc is not None else 0
        ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=w.device) if nb else None
        n = float(w.numel() // 3)
        with _Guard(w, "compose_cross_bwd", n * 200.0, 4.0 * (3 * src.numel() + 3 * w.numel()) + 2.0 * nb):
            _call(L.modet_prpp_compose_bwd, _p(src), _p(w), _p(dout), _p(dsrc), _p(dw), _p(ws), nb, *ctx.dims, _stream())
        return dsrc, dw


def compose_cross(src, w):
    """SpatialTransformer(w's grid)(src, w) + w for a field ``src`` (B,Dc,Hc,Wc,3) on ANOTHER grid than ``w`` (B,Df,Hf,Wf,3), as
    PRNetplusplus.forward composes the coarse flow with a block's field ("Baseline methods/PR++/models.py":338-345): the sample
    point is (p + w) (Sc - 1) / (Sf - 1) in src's coordinates, corners outside contribute zero, src is not rescaled.  This is not
    upsample-then-warp.  The backward's d_src is a deterministic fixed-point scatter in every mode."""
    return _ComposeCross.apply(src, w)


# ---- the resize family (include/modet_hip_resize.h): trilinear resizing between any two grids, and a stage's flow pyramid
RESIZE_MAX_CHANNELS = 256        # MODET_RESIZE_MAX_C of include/modet_hip_resize.h
PYRAMID_MIN_SIZE = 8             # MODET_RESIZE_PYRAMID_MIN: the 1/8 output then has one voxel along that axis
_PYRAMID = ((2, 0.5), (4, 0.25), (8, 0.125))


def _resize_args(op, x, size, scale):
    _chk(x)
    _rank5(op, "x", x)
    size = tuple(size)
    if len(size) != 3 or any(isinstance(s, bool) or int(s) != s or s < 1 for s in size):
        raise RuntimeError(f"{op}: size {size!r} must be three positive integers (D, H, W)")
    B, D, H, W, C = x.shape
    if B < 1 or min(D, H, W) < 1:
        raise RuntimeError(f"{op}: x {tuple(x.shape)} is empty")
    if B > 65535 or not 1 <= C <= RESIZE_MAX_CHANNELS:
        raise RuntimeError(f"{op}: x {tuple(x.shape)}: the kernels take up to 65535 samples and 1 to {RESIZE_MAX_CHANNELS} channels")
    if not math.isfinite(scale):
        raise RuntimeError(f"{op}: scale = {scale!r} must be finite")
    return (B, D, H, W) + tuple(int(s) for s in size) + (C,)


class _Resize(Function):
    @staticmethod
    def forward(ctx, x, size, scale):
        dims = _resize_args("resize", x, size, scale)
        B, C = dims[0], dims[-1]
        y = torch.empty((B,) + dims[4:7] + (C,), dtype=torch.float32, device=x.device)
        with _Guard(x, f"resize_fwd[C{C}]", 16.0 * y.numel(), 4.0 * (x.numel() + y.numel())):
            _call(_L().modet_resize_fwd, _p(x), _p(y), *dims, float(scale), _stream())
        ctx.dims, ctx.scale = dims, float(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        dims = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty((dims[0],) + dims[1:4] + (dims[-1],), dtype=torch.float32, device=dy.device)
        with _Guard(dy, f"resize_bwd[C{dims[-1]}]", 16.0 * dy.numel(), 4.0 * (dx.numel() + dy.numel())):
            _call(_L().modet_resize_bwd, _p(dy), _p(dx), *dims, ctx.scale, _stream())
        return dx, None, None


def resize(x, size, scale=1.0):
    """scale * F.interpolate(x, size=size, mode='trilinear', align_corners=True) of a channels-last (B,D,H,W,C) volume onto ANY
    (D', H', W'): down, up or identity, per axis (the reference's ResizeTransform, "Baseline methods/RDN/models.py":91-117).  The
    backward is a gather: no atomics, bit-reproducible."""
    return _Resize.apply(x, size, scale)


def flow_pyramid_sizes(D, H, W):
    """the three output grids of flow_pyramid: floor(S / 2), floor(S / 4), floor(S / 8), as nnf.interpolate(scale_factor=) sizes them"""
    return tuple((D // f, H // f, W // f) for f, _ in _PYRAMID)


class _FlowPyramid(Function):
    """one node with three outputs: the forward reads the field once, the backward is ONE gather launch over whichever
    cotangents arrived (an output nobody differentiates is passed as NULL)"""

    @staticmethod
    def forward(ctx, flow):
        op = "flow_pyramid"
        _chk(flow)
        _rank5(op, "flow", flow)
        B, D, H, W, C = flow.shape
        if C != 3:
            raise RuntimeError(f"{op}: flow {tuple(flow.shape)} must have 3 channels (a displacement field)")
        if not 1 <= B <= 65535 or min(D, H, W) < PYRAMID_MIN_SIZE:
            raise RuntimeError(f"{op}: flow {tuple(flow.shape)} needs 1 to 65535 samples and at least {PYRAMID_MIN_SIZE} voxels along "
                               "every axis (the 1/8 grid would be empty)")
        ys = tuple(torch.empty((B,) + s + (3,), dtype=torch.float32, device=flow.device) for s in flow_pyramid_sizes(D, H, W))
        nout = sum(y.numel() for y in ys)
        with _Guard(flow, "flow_pyramid_fwd", 16.0 * nout, 4.0 * (flow.numel() + nout)):
            _call(_L().modet_resize_pyramid_fwd, _p(flow), _p(ys[0]), _p(ys[1]), _p(ys[2]), B, D, H, W, _stream())
        ctx.dims = (B, D, H, W)
        ctx.set_materialize_grads(False)
        return ys

    @staticmethod
    def backward(ctx, d2, d4, d8):
        gs = [None if g is None else g.contiguous() for g in (d2, d4, d8)]
        if all(g is None for g in gs):
            return None
        ref = next(g for g in gs if g is not None)
        B, D, H, W = ctx.dims
        dx = torch.empty((B, D, H, W, 3), dtype=torch.float32, device=ref.device)
        nin = sum(g.numel() for g in gs if g is not None)
        with _Guard(ref, "flow_pyramid_bwd", 16.0 * nin, 4.0 * (dx.numel() + nin)):
            _call(_L().modet_resize_pyramid_bwd, _p(gs[0]), _p(gs[1]), _p(gs[2]), None, _p(dx), B, D, H, W, _stream())
        return dx


def flow_pyramid(flow):
    """(0.5 resize(flow, S // 2), 0.25 resize(flow, S // 4), 0.125 resize(flow, S // 8)) of a channels-last field (B,D,H,W,3): the
    three rescaled trilinear downsamplings a recursive RDN stage warps its coarser features by ("Baseline methods/RDN/models.py":
    480-486), from one launch; each output holds the bits of ``resize`` at the same size and scale.  One launch backwards too."""
    return _FlowPyramid.apply(flow)


class _ToCL(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        B, C = x.shape[0], x.shape[1]
        V = x.numel() // (B * C)
        if C == 1:
            return x.reshape((B,) + tuple(x.shape[2:]) + (1,))
        y = torch.empty((B,) + tuple(x.shape[2:]) + (C,), dtype=torch.float32, device=x.device)
        with _Guard(x, "layout", 0.0, 8.0 * x.numel()):
            _call(_L().modet_ncdhw_to_cl, _p(x), _p(y), B, C, V, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        return _ToNCDHW.apply(dy.contiguous())


class _ToNCDHW(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        B, C = x.shape[0], x.shape[-1]
        V = x.numel() // (B * C)
        if C == 1:
            return x.reshape((B, 1) + tuple(x.shape[1:-1]))
        y = torch.empty((B, C) + tuple(x.shape[1:-1]), dtype=torch.float32, device=x.device)
        with _Guard(x, "layout", 0.0, 8.0 * x.numel()):
            _call(_L().modet_cl_to_ncdhw, _p(x), _p(y), B, C, V, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        return _ToCL.apply(dy.contiguous())


def to_channels_last(x):
    """(B,C,D,H,W) -> (B,D,H,W,C) (a free view when C == 1)"""
    return _ToCL.apply(x)


def to_ncdhw(x):
    """(B,D,H,W,C) -> (B,C,D,H,W)"""
    return _ToNCDHW.apply(x)


def _scale_by(x, s):
    y = torch.empty_like(x)
    with _Guard(x, "scale", x.numel(), 8.0 * x.numel()):
        _call(_L().modet_scale_by_dev_scalar, _p(x), _p(s), _p(y), x.numel(), _stream())
    return y


def _volume(op, name, t):
    """one non-empty (B,1,D,H,W) volume"""
    if t.dim() != 5 or t.shape[1] != 1 or t.numel() == 0:
        raise RuntimeError(f"{op}: {name} must be a non-empty (B,1,D,H,W) volume, got {tuple(t.shape)}")


def _pair_shapes(op, a, b, name_a, name_b):
    """two volumes of equal shape -- the shapes alone: the module classes of losses.py name them on tensors they have yet to
    make contiguous"""
    _volume(op, name_a, a)
    _volume(op, name_b, b)
    if a.shape != b.shape:
        raise RuntimeError(f"{op}: {name_b} {tuple(b.shape)} does not match {name_a} {tuple(a.shape)}: they differ in shape")


def _volume_pair(op, a, b, name_a, name_b):
    """what every similarity term takes: two non-empty float32 (B,1,D,H,W) volumes of equal shape, refused in that order (the
    dtype is looked at before the shape is)"""
    _chk(a, b)
    _pair_shapes(op, a, b, name_a, name_b)


def _loss_bufs(x, wants, nbytes, refused=None):
    """what every loss call writes: (the (1,) loss, [a gradient like x or None per entry of wants], the workspace of a *_ws_bytes
    query).  ``refused``: the term's error when the query answers 0 bytes (out of the kernels' range)"""
    if refused and nbytes == 0:
        raise RuntimeError(refused)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    return loss, [torch.empty_like(x) if w else None for w in wants], _ws(nbytes, x)


class _Similarity(Function):
    """every similarity term: ``launch(a, b, want_a, want_b, grad_scale, **params) -> (loss (1,), d_a | None, d_b | None)`` yields
    the value and whichever of the two gradients are needed; backward multiplies the saved gradients by the upstream scalar"""

    @staticmethod
    def forward(ctx, a, b, launch, params):
        loss, d_a, d_b = launch(a, b, ctx.needs_input_grad[0], ctx.needs_input_grad[1], 1.0, **params)
        ctx.save_for_backward(d_a, d_b)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_a, d_b = ctx.saved_tensors
        g = g.contiguous().reshape(1)
        return (None if d_a is None else _scale_by(d_a, g)), (None if d_b is None else _scale_by(d_b, g)), None, None


class _FlowTerm(Function):
    """every regulariser of one flow: ``launch(flow, *params, want_grad, grad_scale=1.0) -> (loss (1,), d_flow | None)``, as
    _Similarity"""

    @staticmethod
    def forward(ctx, flow, launch, params):
        loss, df = launch(flow, *params, ctx.needs_input_grad[0])
        ctx.save_for_backward(df)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        return (None if df is None else _scale_by(df, g.contiguous().reshape(1))), None, None


# ------------------------------------------------------------------------------------------------ NCC, Grad3d
def _ncc_once(I, J, want_grad, win, grad_scale=None):
    """one call in the kernel's roles: (loss (1,), d loss / d J or None); win = 3 | 5 | 7 | 9 (cubic: the z-marching kernel,
    modet_ncc_fwd_bwd_win, or with a grad_scale modet_ncc_fwd_bwd_win_scaled) or a tuple (wz, wy, wx) of any positive sizes
    (modet_ncc_fwd_bwd_box: the reference's padding rule, separable sums)"""
    B, _, D, H, W = I.shape
    L = _L()
    nv = float(I.numel())
    if isinstance(win, tuple):
        wz, wy, wx = win
        nb = L.modet_ncc_box_ws_bytes(B, D, H, W, wz, wy, wx)
        loss, (dJ,), ws = _loss_bufs(J, (want_grad,), nb, f"NCC: window {list(win)} leaves no output voxel on a {(D, H, W)} volume")
        with _Guard(I, "ncc_fwd_bwd_box", 30.0 * (wz + wy + wx) * nv, 150.0 * nv):
            _call(L.modet_ncc_fwd_bwd_box, _p(I), _p(J), _p(loss), _p(dJ), _p(ws), nb, B, D, H, W, wz, wy, wx, _stream())
        return loss, dJ
    nb = L.modet_ncc_ws_bytes(B, D, H, W)
    loss, (dJ,), ws = _loss_bufs(J, (want_grad,), nb)
    with _Guard(I, "ncc_fwd_bwd", 400.0 * nv, 12.0 * nv):               # reads I,J once, writes d_J once
        if grad_scale is None:
            _call(L.modet_ncc_fwd_bwd_win, _p(I), _p(J), _p(loss), _p(dJ), _p(ws), nb, B, D, H, W, int(win), _stream())
        else:
            _call(L.modet_ncc_fwd_bwd_win_scaled, _p(I), _p(J), _p(loss), _p(dJ), _p(ws), nb, B, D, H, W, int(win),
                  float(grad_scale), _stream())
    return loss, dJ


def _ncc_launch(a, b, want_a, want_b, grad_scale, win=9, scaled=False):
    """cc is symmetric in its two arguments (losses.py:85-93), so the gradient w.r.t. a is the kernel's d_J with the roles
    swapped.  The VALUE always comes from the call with the arguments in their own order: the kernel's expanded formula rounds
    differently with the roles swapped, and the value would depend (in its last bit) on which argument is differentiated -- a
    third call when only a needs a gradient.  scaled: the entry point that multiplies the gradient by grad_scale (the autograd
    node's backward does that itself).  The reference's train loop differentiates the FIRST argument (train.py:127:
    ``loss_function(output[n], y)`` = NCC_vxm.forward(y_true=y_moved, y_pred=fixed))."""
    gs = grad_scale if scaled else None
    loss, d_b = _ncc_once(a, b, want_b, win, gs)
    d_a = _ncc_once(b, a, True, win, gs)[1] if want_a else None
    return loss, d_a, d_b


def ncc_loss(y_true, y_pred, win=9):
    """NCC_vxm: -mean(cc) over the windows; win = an int (cubic) or [wz, wy, wx].  Cubic 3 / 5 / 7 / 9 run the z-marching
    kernel, every other window the general separable path.  reference: losses.py:34-94"""
    if isinstance(win, (list, tuple)):
        w = tuple(int(v) for v in win)
        if len(w) != 3 or min(w) < 1:
            raise RuntimeError(f"NCC: a window is three positive sizes, got {win}")
    else:
        w = (int(win),) * 3
    _volume_pair("NCC", y_true, y_pred, "y_true", "y_pred")
    cubic = w[0] == w[1] == w[2] and w[0] in (3, 5, 7, 9)
    return _Similarity.apply(y_true, y_pred, _ncc_launch, {"win": w[0] if cubic else w})


def _grad3d_args(flow, penalty, channels_last):
    """(B, D, H, W) of a planar (B,3,D,H,W) or channels-last (B,D,H,W,3) flow"""
    if penalty not in ("l1", "l2"):
        raise RuntimeError(f"Grad3d: unknown penalty {penalty!r}")
    _chk(flow)
    if flow.dim() != 5 or flow.shape[-1 if channels_last else 1] != 3:
        raise RuntimeError(f"Grad3d: expects a {'channels-last (B,D,H,W,3)' if channels_last else '(B,3,D,H,W)'} flow")
    return (flow.shape[0],) + tuple(flow.shape[1:4] if channels_last else flow.shape[2:])


def _grad3d_launch(flow, penalty, dims, channels_last, want_grad, grad_scale=1.0):
    """modet_grad3d_fwd_bwd (planar; the autograd node's backward scales) / modet_grad3d_fwd_bwd_cl (channels-last, scaled here):
    (loss (1,), d loss / d flow in the flow's layout or None)"""
    L = _L()
    nb = L.modet_grad3d_ws_bytes(*dims)
    loss, (df,), ws = _loss_bufs(flow, (want_grad,), nb)
    pen = 1 if penalty == "l1" else 2
    with _Guard(flow, "grad3d_fwd_bwd", 20.0 * flow.numel(), 8.0 * flow.numel()):
        if channels_last:
            _call(L.modet_grad3d_fwd_bwd_cl, _p(flow), _p(loss), _p(df), _p(ws), nb, *dims, pen, float(grad_scale), _stream())
        else:
            _call(L.modet_grad3d_fwd_bwd, _p(flow), _p(loss), _p(df), _p(ws), nb, *dims, pen, _stream())
    return loss, df


def grad3d_loss(flow, penalty="l2"):
    """Grad3d(penalty='l1' | 'l2') on a planar (B,3,D,H,W) flow.  reference: losses.py:6-31"""
    dims = _grad3d_args(flow, penalty, False)
    return _FlowTerm.apply(flow, _grad3d_launch, (penalty, dims, False))


# ------------------------------------------------------------------------------------------------ MIND-SSC
MIND_BYTES_PER_VOXEL = 352.0     # modet_mind_fwd_bwd with a gradient, its own traffic: 2 x (4 + 48) descriptor passes, 96 + 48 pointwise,
                                 # 48 + 4 + 24 box adjoint, 24 + 4 gather


def _mind_params(op, radius, dilation):
    if int(radius) != 2 or int(dilation) != 2:
        raise RuntimeError(f"{op}: only radius 2 and dilation 2 exist (the reference hard-codes them), got {radius} and {dilation}")


def mind_ssc(img, radius=2, dilation=2):
    """the MIND-SSC descriptor (B,12,D,H,W) of a (B,1,D,H,W) image in the reference's channel order.
    reference: Baseline methods/RCN/losses.py:350-396 (MIND_loss.MINDSSC)"""
    _chk(img)
    _volume("mind_ssc", "img", img)
    _mind_params("mind_ssc", radius, dilation)
    B, _, D, H, W = img.shape
    out = torch.empty((B, 12, D, H, W), dtype=torch.float32, device=img.device)
    L = _L()
    nb = L.modet_mind_ws_bytes(B, D, H, W, 1)
    if nb == 0:
        raise RuntimeError(f"mind_ssc: volume {tuple(img.shape)} is out of the kernels' range")
    ws = _ws(nb, img)
    nv = float(img.numel())
    with _Guard(img, "mind_descriptor", 600.0 * nv, 148.0 * nv):
        _call(L.modet_mind_descriptor, _p(img), _p(out), _p(ws), nb, B, D, H, W, 2, 2, _stream())
    return out


def _mind_once(a, b, want_grad, grad_scale):
    """modet_mind_fwd_bwd(a, b): (loss (1,), grad_scale * d loss / d b or None)"""
    B, _, D, H, W = a.shape
    L = _L()
    nb = L.modet_mind_ws_bytes(B, D, H, W, 2)
    loss, (d_b,), ws = _loss_bufs(b, (want_grad,), nb, f"MIND: volume {tuple(a.shape)} is out of the kernels' range")
    nv = float(a.numel())
    with _Guard(a, "mind_fwd_bwd", 1500.0 * nv, (MIND_BYTES_PER_VOXEL if want_grad else 200.0) * nv):
        _call(L.modet_mind_fwd_bwd, _p(a), _p(b), _p(loss), _p(d_b), _p(ws), nb, B, D, H, W, 2, 2, float(grad_scale), _stream())
    return loss, d_b


def _mind_launch(a, b, want_a, want_b, grad_scale):
    """the loss is symmetric in its two arguments, so the gradient w.r.t. the first is the kernel's d_b with the roles swapped
    (as _ncc_launch).  The value of the swapped call is the same sum in the same order: whichever call ran gives the loss."""
    loss = d_a = d_b = None
    if want_b or not want_a:
        loss, d_b = _mind_once(a, b, want_b, grad_scale)
    if want_a:
        l2, d_a = _mind_once(b, a, True, grad_scale)
        loss = l2 if loss is None else loss
    return loss, d_a, d_b


def mind_loss(a, b):
    """mean((MIND-SSC(a) - MIND-SSC(b))^2) of two (B,1,D,H,W) volumes.  reference: Baseline methods/RCN/losses.py:398-399"""
    _volume_pair("MIND", a, b, "first volume", "second volume")
    return _Similarity.apply(a, b, _mind_launch, {})


# ------------------------------------------------------------------------------------------------ mutual information
MI_BINS = 32                     # the MFMA tile's edge: the only bin count the kernels have (csrc/mi.hip)
MI_MAX_PATCH = 16
# per voxel: the histogram product and each gradient product are 32 x 32 FMA (2048 FLOP) on the fp32 MFMA; the 64 Parzen weights
# of a pass (subtract, square, scale, exp2, normalise) about 512 more.  Traffic: each pass reads both images, a gradient is
# written once; the partials and the two 32 x 32 matrices are noise beside that
MI_FLOP_PER_PASS = 2048.0 + 512.0
MI_BYTES_PER_PASS = 8.0


def _mi_args(op, y_true, y_pred, sigma_ratio, minval, maxval, num_bin, patch_size=None):
    _volume_pair(op, y_true, y_pred, "y_true", "y_pred")
    if int(num_bin) != MI_BINS:
        raise RuntimeError(f"{op}: only num_bin = {MI_BINS} exists, got {num_bin}")
    if not (float(maxval) > 0.0 and float(maxval) > float(minval) and float(sigma_ratio) > 0.0):
        raise RuntimeError(f"{op}: needs maxval > 0, maxval > minval and sigma_ratio > 0, got minval {minval}, maxval {maxval}, "
                           f"sigma_ratio {sigma_ratio}")
    if patch_size is not None and not (int(patch_size) == patch_size and 1 <= int(patch_size) <= MI_MAX_PATCH):
        raise RuntimeError(f"{op}: patch_size must be an integer in 1..{MI_MAX_PATCH}, got {patch_size}")
    return {"sigma_ratio": sigma_ratio, "minval": minval, "maxval": maxval, "patch_size": patch_size}


def _mi_launch(a, b, want_a, want_b, grad_scale, sigma_ratio, minval, maxval, patch_size=None):
    """modet_mi_fwd_bwd / modet_lmi_fwd_bwd (patch_size given): (loss (1,), grad_scale * d loss / d a or None, the same for b)"""
    B, _, D, H, W = a.shape
    L = _L()
    nb = L.modet_mi_ws_bytes(B, D, H, W, 0 if patch_size is None else int(patch_size))
    loss, (d_a, d_b), ws = _loss_bufs(a, (want_a, want_b), nb, f"mutual information: volume {tuple(a.shape)} is out of the kernels' range")
    nv = float(a.numel())
    ngrad = int(bool(want_a)) + int(bool(want_b))
    with _Guard(a, "mi_fwd_bwd" if patch_size is None else "lmi_fwd_bwd", MI_FLOP_PER_PASS * (1 + ngrad) * nv,
                (MI_BYTES_PER_PASS * (1 + min(ngrad, 1)) + 4.0 * ngrad) * nv):
        if patch_size is None:
            _call(L.modet_mi_fwd_bwd, _p(a), _p(b), _p(loss), _p(d_a), _p(d_b), _p(ws), nb, B, D, H, W, MI_BINS, float(minval),
                  float(maxval), float(sigma_ratio), float(grad_scale), _stream())
        else:
            _call(L.modet_lmi_fwd_bwd, _p(a), _p(b), _p(loss), _p(d_a), _p(d_b), _p(ws), nb, B, D, H, W, MI_BINS, float(minval),
                  float(maxval), float(sigma_ratio), int(patch_size), float(grad_scale), _stream())
    return loss, d_a, d_b


def mi_loss(y_true, y_pred, sigma_ratio=1, minval=0.0, maxval=1.0, num_bin=32):
    """-mutual information of two (B,1,D,H,W) volumes over 32 Parzen-window bins, averaged over the batch.
    reference: Baseline methods/RCN/losses.py:401-457 (MutualInformation)"""
    return _Similarity.apply(y_true, y_pred, _mi_launch, _mi_args("mi_loss", y_true, y_pred, sigma_ratio, minval, maxval, num_bin))


def lmi_loss(y_true, y_pred, sigma_ratio=1, minval=0.0, maxval=1.0, num_bin=32, patch_size=5):
    """-mutual information per non-overlapping patch of patch_size^3 voxels of the zero-padded volumes, averaged over all patches.
    reference: Baseline methods/RCN/losses.py:459-556 (localMutualInformation)"""
    return _Similarity.apply(y_true, y_pred, _mi_launch,
                             _mi_args("lmi_loss", y_true, y_pred, sigma_ratio, minval, maxval, num_bin, patch_size))


# ------------------------------------------------------------------------------------------------ SSIM3D
SSIM_MAX_WINDOW = 11             # odd windows 1..11 are instantiated (csrc/ssim.hip)
SSIM_TILE_Y = 16                 # the march kernel's (y, x) tile is 16 x 32: the x pass also filters the 2 p halo rows


def _ssim_counts(window, want_a, want_b):
    """(FLOP, bytes) per voxel of one call, this implementation's own count.  A symmetric 1-D filter
    output costs p pair additions, p + 1 products and p accumulations; the forward filters five fields in x (over 16 + 2 p rows
    per 16), y and z, forms three products per halo voxel and ends in about 40 operations per voxel; a gradient filters three
    coefficient volumes and ends in 5.  Traffic: the forward reads both images and writes 2 + (gradients) coefficient volumes,
    each gradient reads three of them and both images and writes itself; halo re-reads are served by the caches."""
    p = int(window) // 2
    f = 3.0 * p + 1.0
    rows = (SSIM_TILE_Y + 2.0 * p) / SSIM_TILE_Y
    ngrad = int(bool(want_a)) + int(bool(want_b))
    flop = 5.0 * f * (rows + 2.0) + 3.0 * rows + 40.0 + ngrad * (3.0 * f * (rows + 2.0) + 5.0)
    nbytes = 8.0 + (4.0 * (2 + ngrad) if ngrad else 0.0) + 24.0 * ngrad
    return flop, nbytes


def _ssim_args(op, img1, img2, window_size):
    _volume_pair(op, img1, img2, "img1", "img2")
    if not (int(window_size) == window_size and 1 <= int(window_size) <= SSIM_MAX_WINDOW and int(window_size) % 2 == 1):
        raise RuntimeError(f"{op}: window_size must be an odd integer in 1..{SSIM_MAX_WINDOW}, got {window_size}")
    return {"window_size": window_size}


def _ssim_launch(a, b, want_a, want_b, grad_scale, window_size):
    """modet_ssim_fwd_bwd: (loss (1,), grad_scale * d loss / d a or None, the same for b)"""
    B, _, D, H, W = a.shape
    L = _L()
    nb = L.modet_ssim_ws_bytes(B, D, H, W, int(window_size))
    loss, (d_a, d_b), ws = _loss_bufs(a, (want_a, want_b), nb, f"ssim_loss: volume {tuple(a.shape)} is out of the kernels' range")
    nv = float(a.numel())
    flop, nbytes = _ssim_counts(window_size, want_a, want_b)
    with _Guard(a, "ssim_fwd_bwd", flop * nv, nbytes * nv):
        _call(L.modet_ssim_fwd_bwd, _p(a), _p(b), _p(loss), _p(d_a), _p(d_b), _p(ws), nb, B, D, H, W, int(window_size),
              float(grad_scale), _stream())
    return loss, d_a, d_b


def ssim_loss(img1, img2, window_size=11):
    """1 - mean SSIM of two (B,1,D,H,W) volumes under a zero-padded Gaussian window (sigma 1.5) of window_size^3 voxels, applied
    as three 1-D filters.  reference: Baseline methods/RCN/losses.py:103-126 (SSIM3D)"""
    return _Similarity.apply(img1, img2, _ssim_launch, _ssim_args("ssim_loss", img1, img2, window_size))


# ------------------------------------------------------------------------------------------------ flow regularisers beside Grad3d
REG_KINDS = {"itv": 0, "gradient-l2": 1, "gradient-l1": 2, "bending": 3}      # the enum of include/modet_hip_reg.h
REG_MIN_SIZE = {"itv": 2, "gradient-l2": 3, "gradient-l1": 3, "bending": 5}   # the shortest axis that holds a stencil point
# (FLOP, bytes) per ELEMENT of the flow of one call, this implementation's own count (csrc/reg.hip): the
# traffic is the flow read once and the gradient written once, neighbour reads are served by the caches; the arithmetic is the
# gathered adjoint -- iTV: four norms (3 differences, 3 products, a root, a division each); gradient: 6 differences and their
# penalties; bending: 9 axial and 12 mixed second differences of 3 operations, their squares and signed sums.
_REG_COUNTS = {"itv": (60.0, 8.0), "gradient-l2": (20.0, 8.0), "gradient-l1": (24.0, 8.0), "bending": (110.0, 8.0)}


def _reg_args(op, flow, kind, channels_last):
    """(B, C, D, H, W) of a planar (B,C,D,H,W) or channels-last (B,D,H,W,3) flow that the kind accepts"""
    if kind not in REG_KINDS:
        raise RuntimeError(f"{op}: unknown kind {kind!r} (there are {', '.join(REG_KINDS)})")
    _chk(flow)
    if flow.dim() != 5:
        raise RuntimeError(f"{op}: expects a {'channels-last (B,D,H,W,3)' if channels_last else 'planar (B,C,D,H,W)'} flow, got "
                           f"{tuple(flow.shape)}")
    if channels_last:
        B, D, H, W, C = flow.shape
        if C != 3:
            raise RuntimeError(f"{op}: expects a channels-last (B,D,H,W,3) flow, got {tuple(flow.shape)} (a planar one goes through "
                               "reg_loss)")
    else:
        B, C, D, H, W = flow.shape
        if C != 3 and kind != "itv":
            raise RuntimeError(f"{op}: '{kind}' takes a flow of 3 channels (B,3,D,H,W), got {tuple(flow.shape)}")
    if B < 1 or C < 1 or min(D, H, W) < REG_MIN_SIZE[kind]:
        raise RuntimeError(f"{op}: '{kind}' needs a non-empty flow with D, H, W >= {REG_MIN_SIZE[kind]}, got {tuple(flow.shape)}")
    return B, C, D, H, W


def _reg_launch(flow, kind, dims, channels_last, want_grad, grad_scale=1.0):
    """modet_reg_fwd_bwd: (loss (1,), grad_scale * d loss / d flow in the flow's layout or None)"""
    L = _L()
    nb = L.modet_reg_ws_bytes(REG_KINDS[kind], *dims)
    loss, (df,), ws = _loss_bufs(flow, (want_grad,), nb, f"reg_loss: flow {tuple(flow.shape)} is out of the kernels' range")
    flop, nbytes = _REG_COUNTS[kind]
    with _Guard(flow, f"reg_fwd_bwd[{kind}]", flop * flow.numel(), (nbytes if want_grad else 4.0) * flow.numel()):
        _call(L.modet_reg_fwd_bwd, _p(flow), _p(loss), _p(df), _p(ws), nb, REG_KINDS[kind], *dims, int(bool(channels_last)),
              float(grad_scale), _stream())
    return loss, df


def reg_loss(flow, kind):
    """a regulariser of a planar flow: 'itv' (B,C,D,H,W), the isotropic total variation (reference Baseline methods/RCN/losses.py:
    203-221), or on (B,3,D,H,W) 'gradient-l2', 'gradient-l1' and 'bending' (the same file, 223-268)"""
    dims = _reg_args("reg_loss", flow, kind, False)
    return _FlowTerm.apply(flow, _reg_launch, (kind, dims, False))


# ------------------------------------------------------------------------------------------------ label overlap (soft Dice)
SEGDICE_MAX_LABELS = 256         # MODET_SEGDICE_MAX_LABELS of include/modet_hip_segdice.h
# per voxel of one call with a gradient, computed from the shapes (csrc/segdice.hip): the sums pass reads
# the flow (12 B) and the fixed label (2 B), the gradient pass both again and writes d_flow (12 B); the eight gathered moving
# labels of either pass come through the caches (2 B of the map per voxel and pass)
SEGDICE_BYTES_PER_VOXEL = (12.0 + 2.0 + 2.0) + (12.0 + 2.0 + 2.0 + 12.0)


def _segdice_args(op, mov_lab, flow, fix_lab, nlabels, channels_last):
    """(B, D, H, W) of two (B,1,D,H,W) int16 label maps and a planar (B,3,D,H,W) or channels-last (B,D,H,W,3) float32 flow"""
    if isinstance(nlabels, bool) or not isinstance(nlabels, int) or not 1 <= nlabels <= SEGDICE_MAX_LABELS:
        raise RuntimeError(f"{op}: nlabels must be an integer in 1..{SEGDICE_MAX_LABELS}, got {nlabels!r}")
    for name, t in (("mov_lab", mov_lab), ("fix_lab", fix_lab)):
        if not t.is_cuda:
            raise RuntimeError(f"{op}: {name} must live on the GPU (the HIP path has no CPU fallback)")
        if t.dtype != torch.int16:
            raise RuntimeError(f"{op}: {name} must be int16, got {t.dtype}: convert the label map with .to(torch.int16)")
        if not t.is_contiguous():
            raise RuntimeError(f"{op}: {name} must be contiguous")
    _chk(flow)
    _pair_shapes(op, mov_lab, fix_lab, "mov_lab", "fix_lab")
    B, _, D, H, W = mov_lab.shape
    want = (B, D, H, W, 3) if channels_last else (B, 3, D, H, W)
    if flow.dim() != 5 or tuple(flow.shape) != want:
        raise RuntimeError(f"{op}: expects a {'channels-last (B,D,H,W,3)' if channels_last else 'planar (B,3,D,H,W)'} flow "
                           f"{want} for labels {tuple(mov_lab.shape)}, got {tuple(flow.shape)}")
    for name, t in (("mov_lab", mov_lab), ("fix_lab", fix_lab)):
        if t.device != flow.device:
            raise RuntimeError(f"{op}: {name} lives on {t.device}, the flow on {flow.device}")
    return B, D, H, W


def _segdice_ws(op, flow, dims, nlabels):
    nb = _L().modet_segdice_ws_bytes(*dims, nlabels)
    if nb == 0:
        raise RuntimeError(f"{op}: labels {dims} with {nlabels} labels are out of the kernels' range")
    # (a float64 tensor: the workspace begins with 64-bit sums)
    return nb, torch.empty((int(nb) + 7) // 8, dtype=torch.float64, device=flow.device)


def _segdice_launch(flow, mov_lab, fix_lab, nlabels, dims, channels_last, want_grad, grad_scale=1.0, d_flow_add=None):
    """modet_segdice_fwd_bwd: (loss (1,), grad_scale * d loss / d flow in the flow's layout or None, table (B,3,L+1) float64);
    ``d_flow_add``: the gradient is added into this buffer, which is returned"""
    nb, ws = _segdice_ws("seg_dice_loss", flow, dims, nlabels)
    loss = torch.empty(1, dtype=torch.float32, device=flow.device)
    table = torch.empty((dims[0], 3, nlabels + 1), dtype=torch.float64, device=flow.device)
    df = d_flow_add if d_flow_add is not None else (torch.empty_like(flow) if want_grad else None)
    n = float(flow.numel()) / 3
    with _Guard(flow, f"segdice[{nlabels}]", 120.0 * n, (SEGDICE_BYTES_PER_VOXEL if df is not None else 16.0) * n):
        _call(_L().modet_segdice_fwd_bwd, _p(mov_lab), _p(flow), _p(fix_lab), _p(loss), _p(table), _p(df), _p(ws), nb, *dims,
              nlabels, int(bool(channels_last)), float(grad_scale), int(d_flow_add is not None), _stream())
    return loss, df, table


def _segdice_term(flow, mov_lab, fix_lab, nlabels, dims, want_grad):
    return _segdice_launch(flow, mov_lab, fix_lab, nlabels, dims, False, want_grad)[:2]


def seg_dice_loss(mov_lab, flow, fix_lab, nlabels):
    """1 - mean soft Dice of the moving labels warped trilinearly by a planar flow (B,3,D,H,W) against the fixed labels, both
    (B,1,D,H,W) int16 with labels 1..nlabels (include/modet_hip_segdice.h has the formulae): the differentiable form of what
    ``infer`` reports (reference utils.py:86-106, dice_val_VOI).  The gradient is with respect to the flow only."""
    dims = _segdice_args("seg_dice_loss", mov_lab, flow, fix_lab, nlabels, False)
    return _FlowTerm.apply(flow, _segdice_term, (mov_lab, fix_lab, nlabels, dims))


def seg_dice_sums(mov_lab, flow, fix_lab, nlabels, channels_last=False):
    """the (B,3,nlabels+1) float64 table [I, P, T] of seg_dice_loss: per batch item and label the overlap, the warped moving and the
    fixed volume; on an integer-valued flow the counts [2], [0], [1] of label_warp_counts.  Column 0 is 0."""
    dims = _segdice_args("seg_dice_sums", mov_lab, flow, fix_lab, nlabels, channels_last)
    nb, ws = _segdice_ws("seg_dice_sums", flow, dims, nlabels)
    table = torch.empty((dims[0], 3, nlabels + 1), dtype=torch.float64, device=flow.device)
    n = float(flow.numel()) / 3
    with _Guard(flow, f"segdice_sums[{nlabels}]", 60.0 * n, 16.0 * n):
        _call(_L().modet_segdice_sums, _p(mov_lab), _p(flow), _p(fix_lab), _p(table), _p(ws), nb, *dims, nlabels,
              int(bool(channels_last)), _stream())
    return table


# ------------------------------------------------------------------------------------------------ velocity-field integration
VECINT_MAX_STEPS = 12       # MODET_VECINT_MAX_STEPS of include/modet_hip_vecint.h


def _vecint_args(op, vec, nsteps, bound):
    """(B, D, H, W) of a channels-last (B,D,H,W,3) fp32 field; nsteps and bound in the library's range"""
    if isinstance(nsteps, bool) or not isinstance(nsteps, int) or not 0 <= nsteps <= VECINT_MAX_STEPS:
        raise RuntimeError(f"{op}: nsteps must be an integer in 0..{VECINT_MAX_STEPS}, got {nsteps!r}")
    bound = float(bound)
    if not (0.0 <= bound < float("inf")):
        raise RuntimeError(f"{op}: bound must be finite and >= 0 (0 = no promise on max |vec|), got {bound!r}")
    _chk(vec)
    _rank5(op, "vec", vec)
    B, D, H, W, C = vec.shape
    if C != 3:
        raise RuntimeError(f"{op}: vec must be a channels-last (B,D,H,W,3) field, got {tuple(vec.shape)}")
    if min(B, D, H, W) < 1 or vec.numel() >= 2 ** 31:
        raise RuntimeError(f"{op}: vec {tuple(vec.shape)} must be non-empty and hold fewer than 2^31 elements")
    return B, D, H, W


def _vecint_general_steps(nsteps, bound):
    """how many of the backward's steps take the scatter path (include/modet_hip_vecint.h: bound * 2^(k - nsteps) > 1, or no bound)"""
    return sum(1 for k in range(nsteps) if not (bound > 0.0 and bound * 2.0 ** (k - nsteps) <= 1.0))


def _vecint_fwd(vec, nsteps, want_steps):
    """modet_vecint_fwd -> (out, steps or None).  Per voxel and step, this implementation's own count: the footprint (3 floors, 3
    fractions, 8 weights of 2 products) and 8 corners x 3 channels of a masked fma, ~80 FLOP; the field read once and written once
    (12 + 12 B; the corner reads are served by the caches)."""
    B, D, H, W = vec.shape[:4]
    out = torch.empty_like(vec)
    steps = scratch = None
    if nsteps >= 2:
        if want_steps:
            steps = torch.empty((nsteps - 1,) + tuple(vec.shape), dtype=torch.float32, device=vec.device)
        else:
            scratch = torch.empty_like(vec)
    n = float(B) * D * H * W
    with _Guard(vec, f"vecint_fwd[n{nsteps}]", 80.0 * n * nsteps, 24.0 * n * max(nsteps, 1)):
        _call(_L().modet_vecint_fwd, _p(vec), _p(out), _p(steps), _p(scratch), B, D, H, W, nsteps, _stream())
    return out, steps


def _vecint_bwd(vec, steps, dout, nsteps, bound):
    """modet_vecint_bwd -> d_vec.  Per voxel and step: the 27-neighbour hat weights and their fma (27 x 14) plus the flow term
    (8 corners x (5 + 9)) and the sum, ~500 FLOP bounded; a general step has the flow term and the sum (~130) beside the scatter's
    own work, which is not counted here.  Bytes: v and g read, d_v written (36 B), a general step also writes and reads the
    scattered sum (+ 24 B)."""
    B, D, H, W = vec.shape[:4]
    L = _L()
    dvec = torch.empty_like(vec)
    scratch = torch.empty_like(vec) if nsteps >= 2 else None
    nb = L.modet_vecint_ws_bytes(B, D, H, W, nsteps, bound)
    ng = _vecint_general_steps(nsteps, bound)
    if ng and not nb:
        raise RuntimeError(f"vecint: field {tuple(vec.shape)} is out of the kernels' range")
    ws = _ws(nb, vec) if nb else None
    n = float(B) * D * H * W
    with _Guard(vec, f"vecint_bwd[n{nsteps},g{ng}]", n * (500.0 * (nsteps - ng) + 130.0 * ng),
                n * (36.0 * max(nsteps, 1) + 24.0 * ng)):
        _call(L.modet_vecint_bwd, _p(vec), _p(steps), _p(dout), _p(dvec), _p(scratch), _p(ws), nb, B, D, H, W, nsteps, bound,
              _stream())
    return dvec


class _VecInt(Function):
    """saves vec and the inputs of steps 1 .. nsteps-1 (the input of step 0 is recomputed from vec)"""

    @staticmethod
    def forward(ctx, vec, nsteps, bound):
        out, steps = _vecint_fwd(vec, nsteps, ctx.needs_input_grad[0])
        ctx.save_for_backward(vec, steps)
        ctx.nsteps, ctx.bound = nsteps, bound
        return out

    @staticmethod
    def backward(ctx, dout):
        vec, steps = ctx.saved_tensors
        dout = dout.contiguous()
        _chk(dout)
        return _vecint_bwd(vec, steps, dout, ctx.nsteps, ctx.bound), None, None


def vecint(flow_cl, nsteps=7, bound=0.0):
    """VecInt(nsteps) of a channels-last (B,D,H,W,3) velocity field in voxels: v = vec / 2^nsteps, then nsteps times
    v = v + sample(v, p + v) (reference: models.py:70-87).  bound > 0 promises max |vec| <= bound: the backward of every step whose
    field is then bounded by one voxel (bound * 2^(k - nsteps) <= 1) is one gather without atomics.  A broken promise may give a
    wrong gradient, never an out-of-range access."""
    _vecint_args("vecint", flow_cl, nsteps, bound)
    return _VecInt.apply(flow_cl, nsteps, float(bound))


# ------------------------------------------------------------------------------------------------ non-autograd
# (the term as a device scalar, grad_scale * d term / d its second argument, or its flow) from one call of the term's launch
# function above -- no autograd node: the trainer seeds its backward with the gradient (engine.Trainer._seeded_loss)
def _seed(launch, a, b, grad_scale, **params):
    loss, _, d_b = launch(a, b, False, True, grad_scale, **params)
    return loss.reshape(()), d_b


def ncc_value_and_grad(y_true, y_pred, win=9, grad_scale=1.0):
    """(NCC_vxm(y_true, y_pred) as a device scalar, grad_scale * d loss / d y_pred) from one call -- no autograd node: the
    trainer seeds its backward with the gradient (engine.Trainer._seeded_loss).  Cubic windows 3 / 5 / 7 / 9.
    reference: losses.py:34-94, train.py:127"""
    _volume_pair("NCC", y_true, y_pred, "y_true", "y_pred")
    return _seed(_ncc_launch, y_true, y_pred, grad_scale, win=int(win), scaled=True)


def mind_value_and_grad(a, b, grad_scale=1.0):
    """(mind_loss(a, b) as a device scalar, grad_scale * d loss / d b) from one call -- no autograd node: the trainer seeds its
    backward with the gradient (engine.Trainer._seeded_loss)"""
    _volume_pair("MIND", a, b, "first volume", "second volume")
    return _seed(_mind_launch, a, b, grad_scale)


def mi_value_and_grad(y_true, y_pred, sigma_ratio=1, minval=0.0, maxval=1.0, num_bin=32, grad_scale=1.0):
    """(mi_loss(y_true, y_pred) as a device scalar, grad_scale * d loss / d y_pred) from one call -- no autograd node: the trainer
    seeds its backward with the gradient (engine.Trainer._seeded_loss)"""
    return _seed(_mi_launch, y_true, y_pred, grad_scale, **_mi_args("mi_loss", y_true, y_pred, sigma_ratio, minval, maxval, num_bin))


def lmi_value_and_grad(y_true, y_pred, sigma_ratio=1, minval=0.0, maxval=1.0, num_bin=32, patch_size=5, grad_scale=1.0):
    """(lmi_loss(y_true, y_pred) as a device scalar, grad_scale * d loss / d y_pred) from one call, as mi_value_and_grad"""
    return _seed(_mi_launch, y_true, y_pred, grad_scale,
                 **_mi_args("lmi_loss", y_true, y_pred, sigma_ratio, minval, maxval, num_bin, patch_size))


def ssim_value_and_grad(img1, img2, window_size=11, grad_scale=1.0):
    """(ssim_loss(img1, img2) as a device scalar, grad_scale * d loss / d img2) from one call, as mi_value_and_grad"""
    return _seed(_ssim_launch, img1, img2, grad_scale, **_ssim_args("ssim_loss", img1, img2, window_size))


def grad3d_value_and_grad_cl(flow_cl, penalty="l2", grad_scale=1.0):
    """(Grad3d(penalty) as a device scalar, grad_scale * d loss / d flow) of a CHANNELS-LAST flow (B,D,H,W,3), gradient in the
    same layout -- no autograd node, no planar copy of the flow.  reference: losses.py:6-31, train.py:128"""
    dims = _grad3d_args(flow_cl, penalty, True)
    loss, df = _grad3d_launch(flow_cl, penalty, dims, True, True, grad_scale)
    return loss.reshape(()), df


def reg_value_and_grad_cl(flow_cl, kind, grad_scale=1.0):
    """(reg_loss(kind) as a device scalar, grad_scale * d loss / d flow) of a CHANNELS-LAST flow (B,D,H,W,3), gradient in the same
    layout -- no autograd node, no planar copy of the flow: the counterpart of grad3d_value_and_grad_cl"""
    dims = _reg_args("reg_loss", flow_cl, kind, True)
    loss, df = _reg_launch(flow_cl, kind, dims, True, True, grad_scale)
    return loss.reshape(()), df


def seg_dice_value_and_grad_cl(flow_cl, mov_lab, fix_lab, nlabels, grad_scale=1.0, d_flow_add=None):
    """(seg_dice_loss as a device scalar, grad_scale * d loss / d flow) of a CHANNELS-LAST flow (B,D,H,W,3), gradient in the same
    layout -- no autograd node.  ``d_flow_add``: a (B,D,H,W,3) buffer the gradient is ADDED into (and which is returned): the
    step folds this term's seed into the regulariser's without another pass over the flow."""
    dims = _segdice_args("seg_dice_loss", mov_lab, flow_cl, fix_lab, nlabels, True)
    if d_flow_add is not None:
        _chk(d_flow_add)
        _same_shape("seg_dice_loss", "d_flow_add", d_flow_add, flow_cl.shape, f"flow {tuple(flow_cl.shape)}")
        if d_flow_add.device != flow_cl.device:
            raise RuntimeError(f"seg_dice_loss: d_flow_add lives on {d_flow_add.device}, the flow on {flow_cl.device}")
    loss, df, _ = _segdice_launch(flow_cl, mov_lab, fix_lab, nlabels, dims, True, True, grad_scale, d_flow_add)
    return loss.reshape(()), df


def adam_amsgrad_step_(p, g, m, v, vmax, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """in-place Adam(amsgrad=True) over flat buffers.  reference: train.py:101,:131-133"""
    _chk(p, g, m, v, vmax)
    for name, t in (("g", g), ("m", m), ("v", v), ("vmax", vmax)):
        if t.numel() != p.numel():
            raise RuntimeError(f"adam_amsgrad_step_: {name} {tuple(t.shape)} does not match p {tuple(p.shape)}")
    with _Guard(p, "adam_amsgrad", 12.0 * p.numel(), 28.0 * p.numel()):
        _call(_L().modet_adam_amsgrad_step, _p(p), _p(g), _p(m), _p(v), _p(vmax), p.numel(), float(lr), beta1, beta2, eps, int(step),
              float(grad_scale), _stream())


def label_warp_counts(lab_moving, flow_cl, lab_fixed, nlabels=54, want_warped=True):
    """nearest label warp + Dice voxel counts on the GPU.  lab_* (D,H,W) int16, flow_cl (1,D,H,W,3).
    reference: utils.py:74-106, infer.py:86-92.  Returns (warped int16 or None, counts int64 (3, nlabels+1))."""
    if lab_moving.dtype != torch.int16 or lab_fixed.dtype != torch.int16:
        raise RuntimeError("label_warp_counts: labels must be int16")
    _chk(flow_cl)
    if lab_moving.dim() < 3 or lab_moving.numel() != lab_moving.shape[-3] * lab_moving.shape[-2] * lab_moving.shape[-1]:
        raise RuntimeError(f"label_warp_counts: lab_moving {tuple(lab_moving.shape)} is not one (D,H,W) volume")
    D, H, W = lab_moving.shape[-3:]
    if lab_fixed.dim() < 3 or tuple(lab_fixed.shape[-3:]) != (D, H, W) or lab_fixed.numel() != D * H * W:
        raise RuntimeError(f"label_warp_counts: lab_fixed {tuple(lab_fixed.shape)} does not match lab_moving {tuple(lab_moving.shape)}")
    _same_shape("label_warp_counts", "flow_cl", flow_cl, (1, D, H, W, 3), f"lab_moving {tuple(lab_moving.shape)}: one sample")
    for name, t in (("lab_moving", lab_moving), ("lab_fixed", lab_fixed)):
        if t.device != flow_cl.device:
            raise RuntimeError(f"label_warp_counts: {name} lives on {t.device}, flow_cl on {flow_cl.device}")
    if int(nlabels) < 1:
        raise RuntimeError(f"label_warp_counts: nlabels {nlabels} is not positive")
    lm, lf = lab_moving.contiguous(), lab_fixed.contiguous()
    warped = torch.empty((D, H, W), dtype=torch.int16, device=lm.device) if want_warped else None
    counts = torch.empty((3, nlabels + 1), dtype=torch.int64, device=lm.device)
    with _Guard(flow_cl):
        _call(_L().modet_label_warp_counts, _p(lm), _p(flow_cl), _p(lf), _p(warped), _p(counts), D, H, W, nlabels, _stream())
    return warped, counts


def jacdet_nonpos_count(flow_cl, want_det=False):
    """number of voxels per sample whose Jacobian determinant of (identity + flow) is <= 0, on the GPU, in the
    reference's fp64 operation order (utils.py:108-150, infer.py:89-90).  flow_cl (B,D,H,W,3) channels-last fp32.
    Returns (counts int64 (B,), det float64 (B,D,H,W) or None)."""
    _chk(flow_cl)
    if flow_cl.dim() != 5:
        raise RuntimeError(f"jacdet_nonpos_count: expects a (B,D,H,W,3) channels-last flow, got {tuple(flow_cl.shape)}")
    B, D, H, W, C = flow_cl.shape
    if C != 3:
        raise RuntimeError("jacdet_nonpos_count: expects a (B,D,H,W,3) channels-last flow")
    counts = torch.empty(B, dtype=torch.int64, device=flow_cl.device)
    det = torch.empty((B, D, H, W), dtype=torch.float64, device=flow_cl.device) if want_det else None
    with _Guard(flow_cl, "jacdet", 60.0 * flow_cl.numel() / 3, 4.0 * flow_cl.numel()):
        _call(_L().modet_jacdet_nonpos_count, _p(flow_cl), _p(counts), _p(det), B, D, H, W, _stream())
    return counts, det


SURFACE_MAX_DIM, SURFACE_MAX_LABELS = 512, 32767     # include/modet_hip_surface.h


def surface_distances(lab_a, lab_b, nlabels=54, percentile=95.0):
    """per-label surface distances of two (D,H,W) int16 label maps on the GPU, unit spacing, connectivity 1 (medpy's metric.hd,
    hd95 and assd, which the reference's Baseline methods/RDN/utils.py:94-116 runs per label on the CPU).  Returns device tensors
    (metrics float64 (nlabels, 5): hd, hd-percentile, assd, asd_ab, asd_ba; counts int64 (nlabels, 7): n_a, n_b, nborder_a,
    nborder_b and the integer squares hd2, q_lo2, q_hi2).  A label empty in either map has NaN metrics and -1 squares."""
    op = "surface_distances"
    if isinstance(nlabels, bool) or not isinstance(nlabels, int) or not 1 <= nlabels <= SURFACE_MAX_LABELS:
        raise RuntimeError(f"{op}: nlabels must be an integer in 1..{SURFACE_MAX_LABELS}, got {nlabels!r}")
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float)) or not 0.0 <= float(percentile) <= 100.0:
        raise RuntimeError(f"{op}: percentile must be a number in [0, 100], got {percentile!r}")
    for name, t in (("lab_a", lab_a), ("lab_b", lab_b)):
        if not t.is_cuda:
            raise RuntimeError(f"{op}: {name} must live on the GPU (the HIP path has no CPU fallback)")
        if t.dtype != torch.int16:
            raise RuntimeError(f"{op}: {name} must be int16, got {t.dtype}")
        if t.dim() != 3:
            raise RuntimeError(f"{op}: {name} must be one (D,H,W) label map, got {tuple(t.shape)} (2-D maps and batches, B > 1, "
                               "are not supported)")
        if not t.is_contiguous():
            raise RuntimeError(f"{op}: {name} must be contiguous")
    _same_shape(op, "lab_b", lab_b, lab_a.shape, f"lab_a {tuple(lab_a.shape)}")
    if lab_b.device != lab_a.device:
        raise RuntimeError(f"{op}: lab_a lives on {lab_a.device}, lab_b on {lab_b.device}")
    D, H, W = lab_a.shape
    if min(D, H, W) < 1 or max(D, H, W) > SURFACE_MAX_DIM:
        raise RuntimeError(f"{op}: every dimension of {tuple(lab_a.shape)} must be in 1..{SURFACE_MAX_DIM}")
    L = _L()
    nb = L.modet_surface_ws_bytes(D, H, W, nlabels)
    if not nb:
        raise RuntimeError(f"{op}: maps {tuple(lab_a.shape)} with {nlabels} labels are out of the kernels' range")
    metrics = torch.empty((nlabels, 5), dtype=torch.float64, device=lab_a.device)
    counts = torch.empty((nlabels, 7), dtype=torch.int64, device=lab_a.device)
    ws = _ws(nb, lab_a)
    n = float(D) * H * W
    with _Guard(lab_a, f"surface[{nlabels}]", 0.0, 16.0 * n):
        _call(L.modet_surface_distances, _p(lab_a), _p(lab_b), _p(metrics), _p(counts), _p(ws), nb, D, H, W, nlabels,
              float(percentile), _stream())
    return metrics, counts


# ------------------------------------------------------------------------------------------------ bf16 storage (cfg 5)
# BASELINE.json configs[4] "bf16 storage / fp32 accumulate": the ConvInsBlock chains (94 % of the step's FLOPs, half of its
# bytes) keep their activations in bf16 and run on the bf16 matrix pipe; everything that crosses a chain's boundary (level
# inputs / outputs, all parameters, statistics, weight gradients) stays fp32.  csrc/conv3d_bf16.hip, norm_act.hip.
def _chk16(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("smilecode_amd: tensor must live on the GPU (the HIP path has no CPU fallback)")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"smilecode_amd: expected float32 or bfloat16, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError("smilecode_amd: tensor must be contiguous")


def _isbf(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def cast_bf16(x, to_bf16):
    """fp32 <-> bf16 copy (round to nearest even) by the library's own kernel"""
    _chk16(x)
    y = torch.empty(x.shape, dtype=torch.bfloat16 if to_bf16 else torch.float32, device=x.device)
    with _Guard(x, "cast_bf16", 0.0, 6.0 * x.numel()):
        _call(_L().modet_cast_bf16, _p(x), _p(y), x.numel(), int(to_bf16), _stream())
    return y


def conv3d_bf16_forward(x, w, b, want_stats=True, step=None):
    """y (bf16) = conv3d(x (fp32 | bf16), w) + b on the bf16 matrix pipe, fp32 accumulate; (y, stats | None)"""
    _chk16(x)
    _chk(w, b)
    _rank5("conv3d_bf16", "the input", x)
    step = step if step is not None else current_step()
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, Cin, 3, 3, 3):
        raise RuntimeError(f"conv3d_bf16: weight {tuple(w.shape)} does not match input channels {Cin}")
    _same_shape("conv3d_bf16", "bias", b, (Cout,), f"weight {tuple(w.shape)}")
    L = _L()
    y = torch.empty((B, D, H, W, Cout), dtype=torch.bfloat16, device=x.device)
    nb = L.modet_conv3d_bf16_ws_bytes(Cin, Cout)
    ws = _ws(nb, x)
    sb = L.modet_conv3d_bf16_stats_bytes(B, D, H, W, Cin, Cout) if want_stats else 0
    stats = torch.empty(sb // 4, dtype=torch.float32, device=x.device) if sb > 0 else None
    n = float(B) * D * H * W
    with _Guard(x, _conv16_tag("fwd", x.shape, Cin, Cout, _isbf(x)), 54.0 * Cin * Cout * n, n * ((2.0 if _isbf(x) else 4.0) * Cin + 2.0 * Cout)):
        _call(L.modet_conv3d_bf16_fwd, _p(x), _isbf(x), _p(w), _p(b), _p(y), _p(ws), nb, _p(stats), sb, B, D, H, W, Cin, Cout,
              _stream(), _h(step))
    return y, stats


def conv3d_bf16_backward_data(dy, w, Cin, dx_bf16, step=None):
    _chk16(dy)
    _chk(w)
    step = step if step is not None else current_step()
    if dy.dim() != 5:
        raise RuntimeError(f"conv3d_bf16_backward_data: expects a channels-last (B,D,H,W,Cout) gradient, got {tuple(dy.shape)}")
    B, D, H, W, Cout = dy.shape
    _same_shape("conv3d_bf16_backward_data", "weight", w, (Cout, Cin, 3, 3, 3), f"gradient {tuple(dy.shape)}, Cin {Cin}")
    dx = torch.empty((B, D, H, W, Cin), dtype=torch.bfloat16 if dx_bf16 else torch.float32, device=dy.device)
    L = _L()
    nb = L.modet_conv3d_bf16_ws_bytes(Cin, Cout)
    ws = _ws(nb, dy)
    n = float(B) * D * H * W
    with _Guard(dy, _conv16_tag("dgrad", dy.shape, Cin, Cout, True), 54.0 * Cin * Cout * n, n * (2.0 * Cout + (2.0 if dx_bf16 else 4.0) * Cin)):
        _call(L.modet_conv3d_bf16_bwd_data, _p(dy), _p(w), _p(dx), int(dx_bf16), _p(ws), nb, B, D, H, W, Cin, Cout, _stream(), _h(step))
    return dx


def conv3d_bf16_backward_weight(x, dy, w=None, b=None, step=None):
    """d_w, d_bias (fp32) from x (fp32 | bf16) and d_y (bf16); with a StepContext whose ``deferred()`` scope has
    destinations for the parameters ``w`` / ``b`` the gradients go there at the flush and (None, None) is returned"""
    _chk16(x, dy)
    if x.dim() != 5 or dy.dim() != 5 or tuple(dy.shape[:4]) != tuple(x.shape[:4]):
        raise RuntimeError(f"conv3d_bf16_backward_weight: gradient {tuple(dy.shape)} does not match input {tuple(x.shape)}")
    if dy.dtype != torch.bfloat16:
        raise RuntimeError(f"conv3d_bf16_backward_weight: the gradient must be bfloat16, got {dy.dtype}")
    L = _L()
    if not hasattr(L, "modet_conv3d_bf16_bwd_weight"):      # (an older library loaded through MODET_HIP_LIB for A/B timing)
        x32 = x if x.dtype == torch.float32 else cast_bf16(x, False)
        return conv3d_backward_weight(x32, cast_bf16(dy, False), True)
    B, D, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    nb = L.modet_conv3d_bf16_bwd_weight_ws_bytes(B, D, H, W, Cin, Cout)
    ws = _ws(nb, x)
    n = float(B) * D * H * W

    def launch(fn, dw, db, *handle):
        """the one library call: with a step-context handle the partial tiles are reduced at its flush, else now"""
        with _Guard(x, _conv16_tag("wgrad", x.shape, Cin, Cout, _isbf(x)), 54.0 * Cin * Cout * n, n * ((2.0 if _isbf(x) else 4.0) * Cin + 2.0 * Cout)):
            _call(fn, _p(x), _isbf(x), _p(dy), _p(dw), _p(db), _p(ws), nb, B, D, H, W, Cin, Cout, _stream(), *handle)

    scope = step if step is not None else current_step()
    dst = scope.destinations(w, b, True) if (scope is not None and hasattr(L, "modet_conv3d_bf16_bwd_weight_defer")) else None
    if dst is None:
        dw = torch.empty((Cout, Cin, 3, 3, 3), dtype=torch.float32, device=x.device)
        db = torch.empty((Cout,), dtype=torch.float32, device=x.device)
        launch(L.modet_conv3d_bf16_bwd_weight, dw, db)
        return dw, db
    launch(L.modet_conv3d_bf16_bwd_weight_defer, *dst, _h(scope))
    scope._keep.append(ws)
    scope.written.add(w.data_ptr())
    scope.written.add(b.data_ptr())
    return None, None


class _Conv3dBF16(Function):
    """conv3d with bf16 output (+ InstanceNorm partial statistics from the fp32 accumulators, not differentiable)"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.step = current_step()
        y, stats = conv3d_bf16_forward(x, w, b, True, ctx.step)
        ctx.save_for_backward(x, w, b)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)        # no zeros_like(stats) fill launch for the statistics output's "gradient"
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        if dy is None:
            return None, None, None
        x, w, b = ctx.saved_tensors
        dy = dy.contiguous()
        dx = conv3d_bf16_backward_data(dy, w, x.shape[-1], x.dtype == torch.bfloat16, ctx.step) if ctx.needs_input_grad[0] else None
        dw, db = conv3d_bf16_backward_weight(x, dy, w, b, ctx.step)
        return dx, dw, db


def _in16_args(x, stats):
    """a bf16 raw conv output and the partial statistics of the conv's epilogue (the bf16 chain has no one-pass form)"""
    _chk16(x)
    if x.dtype != torch.bfloat16:
        raise RuntimeError("instnorm bf16: the raw conv output must be bfloat16")
    if stats is None:
        raise RuntimeError("instnorm bf16: needs the conv epilogue's partial statistics")
    _chk(stats)


def _in16_fwd(x, stats, eps, out_bf16):
    """THE bf16 InstanceNorm + LeakyReLU forward launch -> (y bf16 | fp32, mean, rstd)"""
    B, V, C, mean, rstd = _in_dims(x)
    y = torch.empty(x.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    nel = float(x.numel())
    with _Guard(x, "instnorm_bf16_fwd", 8.0 * nel, nel * (4.0 if out_bf16 else 6.0)):
        _call(_L().modet_instnorm_lrelu_fwd_stats_bf16, _p(x), _p(y), int(out_bf16), _p(mean), _p(rstd), _p(stats), stats.numel() * 4,
              B, V, C, eps, _stream())
    return y, mean, rstd


def _in16_bwd(dy, x, mean, rstd):
    """THE bf16 InstanceNorm + LeakyReLU backward launch: d_y fp32 or bf16 -> d_x bf16"""
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // (B * C)
    dx = torch.empty_like(x)
    L = _L()
    nb = L.modet_instnorm_bf16_ws_bytes(B, V, C)
    ws = _ws(nb, x)
    nel = float(x.numel())
    with _Guard(x, "instnorm_bf16_bwd", 14.0 * nel, nel * (6.0 + 2.0 * (2.0 if _isbf(dy) else 4.0))):
        _call(L.modet_instnorm_lrelu_bwd_bf16, _p(dy), _isbf(dy), _p(x), _p(mean), _p(rstd), _p(dx), _p(ws), nb, B, V, C, _stream())
    return dx


class _InstNormLReLUBF16(Function):
    """InstanceNorm3d + LeakyReLU(0.1) of a bf16 raw conv output; y is bf16 (inside a chain) or fp32 (a level's output)"""

    @staticmethod
    def forward(ctx, x, stats, eps, out_bf16):
        _in16_args(x, stats)
        y, mean, rstd = _in16_fwd(x, stats, eps, out_bf16)
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        return _in16_bwd(dy.contiguous(), x, mean, rstd), None, None, None


class _InstNormLReLUBF16PoolSplit(Function):
    """_InstNormLReLUBF16 (fp32 output) followed by _PoolTeeSplit as ONE node, bf16 chain: x_raw bf16 (2B,...) ->
    (avgpool2(y), y[:B], y[B:]) with y = LeakyReLU(InstanceNorm(x_raw)) in fp32.  Forward: the two kernels unchanged (a fused
    apply + pool was measured and bought nothing for the bf16 chain); backward: d_y = unpool(g_pooled) / 8 + [g_a ; g_b] is
    formed inside the two InstanceNorm backward passes (modet_instnorm_lrelu_bwd_pool_bf16) instead of written by the pool
    backward and read back twice: same arithmetic, same order of the sums -- bit-identical to the two-node form."""

    @staticmethod
    def forward(ctx, x, stats, eps, Bh, features16=False):
        _in16_args(x, stats)
        _rank5("instnorm bf16", "the raw conv output", x)
        B, D, H, W, C = x.shape
        if not 0 < Bh < B:
            raise RuntimeError(f"instnorm bf16: split {Bh} is not inside the batch of {tuple(x.shape)}")
        if features16:
            # one pass: bf16 features + the pooled tensor from their fp32 values (pooling the ROUNDED features costs the gradient)
            y = torch.empty_like(x)
            *_, mean, rstd = _in_dims(x)
            pooled = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
            nel = float(x.numel())
            with _Guard(x, "instnorm_bf16_fwd", 9.0 * nel, nel * 4.5):
                _call(_L().modet_instnorm_lrelu_fwd_stats_pool_bf16, _p(x), _p(y), _p(pooled), _p(mean), _p(rstd), _p(stats),
                      stats.numel() * 4, B, D, H, W, C, eps, _stream())
        else:
            y, mean, rstd = _in16_fwd(x, stats, eps, False)
            pooled = _pool_fwd(y)
        ctx.save_for_backward(x, mean, rstd)
        ctx.Bh = Bh
        ctx.set_materialize_grads(False)
        if not features16:
            return pooled, y[:Bh], y[Bh:]
        # bf16 level features: the two halves leave as fp32 HANDLES -- allocated, never written, never read -- that carry the
        # bf16 tensor as ``.data16``.  Autograd sees fp32 tensors of the right shape, so the consumers' fp32 gradients arrive
        # here uncast (a bf16 tensor on the edge would have them rounded to bf16, with a cast pass each); the consumers
        # (level_attention_bf16) read ``.data16`` only.
        # (one element of storage expanded to the shape -- autograd checks sizes only -- not a full fp32 allocation
        # beside the bf16 data; and only ModeT.forward ever asks for handles: Encoder.forward_pair(handles=True))
        hm = torch.empty(1, dtype=torch.float32, device=x.device).expand((Bh,) + tuple(x.shape[1:]))
        hf = torch.empty(1, dtype=torch.float32, device=x.device).expand((B - Bh,) + tuple(x.shape[1:]))
        hm.data16, hf.data16 = y[:Bh], y[Bh:]
        return pooled, hm, hf

    @staticmethod
    def backward(ctx, gy, ga, gb):
        if not ctx.needs_input_grad[0] or (gy is None and ga is None and gb is None):
            return None, None, None, None, None
        x, mean, rstd = ctx.saved_tensors
        B, D, H, W, C = x.shape
        Bh = ctx.Bh
        if gy is None:
            return _in16_bwd(_halves(ga, gb, Bh, x.shape), x, mean, rstd), None, None, None, None
        gy = gy.contiguous()
        ga = None if ga is None else ga.contiguous()
        gb = None if gb is None else gb.contiguous()
        dx = torch.empty_like(x)
        L = _L()
        nb = L.modet_instnorm_bf16_ws_bytes(B, D * H * W, C)
        ws = _ws(nb, x)
        nel = float(x.numel())
        with _Guard(x, "instnorm_bf16_bwd", 15.0 * nel, nel * 14.5):
            _call(L.modet_instnorm_lrelu_bwd_pool_bf16, _p(gy), _p(ga), _p(gb), Bh, _p(x), _p(mean), _p(rstd), _p(dx), _p(ws), nb,
                  B, D, H, W, C, _stream())
        return dx, None, None, None, None


def _conv_ins_head_bf16(inp, w1, b1, w2, b2, eps):
    """ConvInsBlock -> conv with bf16 storage: the nodes the two pair forms share -> (raw bf16 output of the second conv, its statistics)"""
    raw1, st1 = _Conv3dBF16.apply(inp, w1, b1)
    y1 = _InstNormLReLUBF16.apply(raw1, st1, eps, True)
    return _Conv3dBF16.apply(y1, w2, b2)


def conv_ins_pair_bf16_pool_split(inp, w1, b1, w2, b2, Bh, eps=1e-5, features16=False):
    """conv_ins_pair_bf16 whose output goes to AvgPool3d(2) and, split into its two batch halves, to the level's consumers:
    (pooled, y[:Bh], y[Bh:]); see _InstNormLReLUBF16PoolSplit.  features16: the two halves are stored as bf16 and handed out as
    fp32 handles with ``.data16`` (only level_attention_bf16 understands those)."""
    raw2, st2 = _conv_ins_head_bf16(inp, w1, b1, w2, b2, eps)
    return _InstNormLReLUBF16PoolSplit.apply(raw2, st2, eps, Bh, features16)


def feature_handle_like(new, old):
    """``new`` (a detached copy / leaf of the fp32 handle ``old``) carries the same bf16 level features"""
    d16 = getattr(old, "data16", None)
    if d16 is not None:
        new.data16 = d16
    return new


def conv_ins_pair_bf16(inp, w1, b1, w2, b2, eps=1e-5):
    """ConvInsBlock -> ConvInsBlock with bf16 storage inside the chain: fp32 (or bf16) in, fp32 out"""
    raw2, st2 = _conv_ins_head_bf16(inp, w1, b1, w2, b2, eps)
    return _InstNormLReLUBF16.apply(raw2, st2, eps, False)
