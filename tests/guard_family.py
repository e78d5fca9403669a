"""What the tests of the ABI families beside the core share (_lib.FAMILIES: mind, mi, ssim, reg, vecint, convs2, deconv).

-m gpu: the guard-band harness of tests/test_gpu_<family>_guard.py.  Every caller-supplied tensor sits between guard bands
(tests/guard.py), outputs and workspaces are poisoned, and the library is reached through a recording proxy over the family's
table.  Per case: no band is damaged, every result is finite, the results equal an unguarded run bit for bit, and a second guarded
run with 0x00 instead of 0xFF bands and poison gives the same bits.  The files themselves hold cases and expectations only.

Without a GPU: the family's header against its ctypes table and the library's exports, and the header as C99."""
import contextlib
import os
import subprocess

import pytest
import torch

from tests import guard


class Maker:
    """puts a case's tensors on the GPU: plain (mode None), or between bands of 0xFF / 0x00 bytes"""

    def __init__(self, mode):
        self.mode = mode

    def __call__(self, t):
        return t.cuda() if self.mode is None else guard.guarded(t.cuda(), canary=self.mode)

    def empty(self, shape, dtype=torch.float32):
        """an output buffer (poisoned when guarded)"""
        if self.mode is None:
            return torch.empty(shape, dtype=dtype, device="cuda")
        return guard.guarded_empty(shape, dtype, "cuda", canary=self.mode)

    def ws(self, nbytes):
        """a workspace of exactly nbytes (guarded: poisoned, and every byte behind it is band; plain: rounded up to 4)"""
        if self.mode is None:
            return torch.empty(-(-int(nbytes) // 4) * 4, dtype=torch.uint8, device="cuda")
        return guard.guarded_bytes(nbytes, "cuda", canary=self.mode)


def stream():
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), "%s: %s differs (%s): max |diff| %.3e" % (
            tag, k, what, float((a[k].double() - b[k].double()).abs().max()))


class Harness:
    """one family's guard session: its ``px`` fixture, the proxies' (entry point, [class of each pointer argument]) records of the
    0xFF runs (``seen``) and the cases that ran (``ran``, filled by the test file)"""

    def __init__(self, family):
        self.family, self.seen, self.ran = family, [], set()

    def fixture(self):
        @pytest.fixture
        def px(monkeypatch):
            from smilecode_amd import _lib
            p = guard.LibProxy(_lib.load(), signatures=_lib.FAMILIES[self.family][1])
            monkeypatch.setattr(_lib, "_lib", p)
            guard.release()
            yield p
            guard.release()
            torch.cuda.empty_cache()
        return px

    def run(self, case, mode, px):
        g, ctx = Maker(mode), (contextlib.nullcontext() if mode is None else guard.GuardedAlloc(canary=mode))
        n0, outs = len(px.records), {}
        with ctx:
            named = case(g)
            torch.cuda.synchronize()
            if mode is not None:
                bands = guard.check()
                assert not bands, guard.describe(bands)
            for k, v in named.items():
                outs[k] = v.detach().clone()
        if mode == 0xFF:
            self.seen.extend(px.records[n0:])
        del px.records[n0:]
        guard.release()
        return outs

    def run_guarded(self, case, px, tag):
        plain = self.run(case, None, px)
        first = self.run(case, 0xFF, px)
        for k, v in first.items():
            assert bool(torch.isfinite(v).all()), "%s: %s is not finite in the guarded run (a read of a band or of poison)" % (tag, k)
        _same(first, plain, "guarded vs unguarded", tag)
        second = self.run(case, 0x00, px)
        _same(second, first, "0x00 vs 0xFF bands and poison", tag)

    def check_coverage(self, px, cases, expect):
        """the coverage condition of tests/test_gpu_guard.py over the family's table: every launching name of it was called at
        least once with every device pointer inside a guarded buffer, and no case handed the library a device pointer outside
        one.  Cases deselected from this session are run here, guarded once.  ``expect``: launching name -> (positions among
        its pointer arguments seen both present and absent, positions always inside a guarded buffer)."""
        from smilecode_amd import _lib
        for tag in sorted(cases):
            if tag not in self.ran:
                self.run(cases[tag], 0xFF, px)
        need = sorted(n for n in _lib.FAMILIES[self.family][1] if guard.is_launching(n))
        assert need == sorted(expect)
        clean = {n for n, cs in self.seen if "torch" not in cs}
        missing = [n for n in need if n not in clean]
        loose = sorted({n for n, cs in self.seen if "torch" in cs})
        assert not missing, "entry points never called with all device pointers guarded: " + ", ".join(missing)
        assert not loose, "cases handed the library pointers outside every guarded buffer: " + ", ".join(loose)
        for n, (either, always) in expect.items():
            for at in either:
                seen = {cs[at] for m, cs in self.seen if m == n}
                assert seen == {"guarded", "null"}, (n, at, seen)
            if always:
                assert {cs[i] for m, cs in self.seen if m == n for i in always} == {"guarded"}, n


NULL, DIM, UNSUP, WS = -1, -2, -3, -4          # MODET_ERR_NULL, _DIM, _UNSUPPORTED, _WORKSPACE


class StridedLayer:
    """What the guard files of the two stride-2 layer families share (test_gpu_convs2_guard.py, test_gpu_deconv_guard.py): the
    cases over the family's oracle (``orc``: tests/rdn_oracle.py, tests/rcn_oracle.py) and the refusals every entry point of
    either makes.  ``prefix``: the entry points are modet_<prefix>_fwd, _bwd_data, _bwd_weight and _ws_bytes; ``wrapper``: the name
    of the package's function in smilecode_amd.ops; ``has_bias(n)``: whether case n of the oracle has a bias of its own (a case
    given one without gets 0.25 per channel); ``seed``: the wrapper cases draw their tensors with seed + n."""

    def __init__(self, orc, prefix, wrapper, has_bias, seed):
        self.orc, self.prefix, self.wrapper, self.has_bias, self.seed = orc, prefix, wrapper, has_bias, seed

    def entry(self, L, name):
        return getattr(L, "modet_%s_%s" % (self.prefix, name))

    def _tensors(self, g, n, bias, seed=None):
        Cout = self.orc.OP_CASES[n][3]
        use_bias = self.has_bias(n) if bias is None else bias
        x, w, b, gy = self.orc.case_tensors(n, seed=seed)
        b = g(b if b is not None else torch.full((Cout,), 0.25)) if use_bias else None
        return g(x), g(w), b, g(gy)

    def abi_case(self, n, bias=None):
        """the C ABI directly, exact workspaces: forward, data gradient, weight gradient"""
        def case(g):
            from smilecode_amd import _lib
            L = _lib.load()
            (B, (D_, H_, W_), Cin, Cout), slope = self.orc.OP_CASES[n][:4], self.orc.OP_CASES[n][-1]
            x, w, b, gy = self._tensors(g, n, bias)
            act, sl = int(slope is not None), float(slope or 0.0)
            dims = (B, D_, H_, W_, Cin, Cout)
            y, dx, dw = g.empty(gy.shape), g.empty(x.shape), g.empty(w.shape)
            db = g.empty((Cout,)) if b is not None else None
            p = lambda v: None if v is None else v.data_ptr()      # noqa: E731
            nbs = [self.entry(L, "ws_bytes")(*dims, k) for k in range(3)]
            assert min(nbs) > 0
            ws = [g.ws(nb) for nb in nbs]
            _lib.check(self.entry(L, "fwd")(p(x), p(w), p(b), p(y), p(ws[0]), nbs[0], *dims, act, sl, stream()), self.prefix + " fwd")
            ya = y if act else None
            _lib.check(self.entry(L, "bwd_data")(p(gy), p(ya), p(w), p(dx), p(ws[1]), nbs[1], *dims, act, sl, stream()),
                       self.prefix + " bwd data")
            _lib.check(self.entry(L, "bwd_weight")(p(x), p(gy), p(ya), p(dw), p(db), p(ws[2]), nbs[2], *dims, act, sl, stream()),
                       self.prefix + " bwd weight")
            out = {"y": y, "d_x": dx, "d_w": dw}
            if b is not None:
                out["d_b"] = db
            return out
        return case

    def ops_case(self, n, bias=None):
        """the package's own wrapper under GuardedAlloc: outputs, gradients and workspaces are guarded allocations"""
        def case(g):
            from smilecode_amd import ops
            x, w, b, gy = self._tensors(g, n, bias, seed=self.seed + n)
            leaves = [t.requires_grad_(True) for t in (x, w, b) if t is not None]
            y = getattr(ops, self.wrapper)(x, w, b, self.orc.OP_CASES[n][-1])
            grads = torch.autograd.grad(y, leaves, gy)
            out = {"y": y}
            out.update({"g%d" % i: v for i, v in enumerate(grads)})
            return out
        return case

    def refusals(self, dims, w_shape, slope):
        return _Refusals(self, dims, w_shape, slope)


class _Refusals:
    """a valid call of each entry point of a stride-2 layer at ``dims`` with an activation, on outputs filled with 7: fwd(),
    bwd_data() and bwd_weight() make it with the arguments given by keyword replaced (a pointer by None or an address; nb, dims,
    act, slope) and return the library's code"""

    def __init__(self, layer, dims, w_shape, slope):
        from smilecode_amd import _lib
        self.layer, self.L, self.dims, self.slope = layer, _lib.load(), dims, slope
        B, D, H, W, Cin, Cout = dims
        out = (B,) + tuple(layer.orc.out_shape(D, H, W)) + (Cout,)
        self.x, self.w, self.b = (torch.zeros(s, device="cuda") for s in ((B, D, H, W, Cin), w_shape, (Cout,)))
        self.y, self.gy = torch.full(out, 7.0, device="cuda"), torch.ones(out, device="cuda")
        self.dx, self.dw, self.db = (torch.full_like(t, 7.0) for t in (self.x, self.w, self.b))
        self.nb = [layer.entry(self.L, "ws_bytes")(*dims, k) for k in range(3)]
        self.ws = torch.empty(max(self.nb) + 32, dtype=torch.uint8, device="cuda")

    def _call(self, name, ptrs, k, kw):
        a = {p: getattr(self, p).data_ptr() for p in ptrs}
        a.update(nb=self.nb[k], dims=self.dims, act=1, slope=self.slope)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return self.layer.entry(self.L, name)(*(a[p] for p in ptrs), a["nb"], *a["dims"], a["act"], a["slope"], stream())

    def fwd(self, **kw):
        return self._call("fwd", ("x", "w", "b", "y", "ws"), 0, kw)

    def bwd_data(self, **kw):
        return self._call("bwd_data", ("gy", "y", "w", "dx", "ws"), 1, kw)

    def bwd_weight(self, **kw):
        return self._call("bwd_weight", ("x", "gy", "y", "dw", "db", "ws"), 2, kw)

    def check(self):
        """NULL pointers, an empty axis, a negative slope, an activation code of 2, a misaligned tensor and a short or misaligned
        workspace are answered with the library's error codes before any launch: the outputs keep their fill (after the
        file's own refusals too: call this last)"""
        fwd, bd, bw, nb = self.fwd, self.bwd_data, self.bwd_weight, self.nb
        x, ws = self.x.data_ptr(), self.ws.data_ptr()
        assert fwd(x=None) == NULL and fwd(y=None) == NULL and fwd(ws=None) == NULL
        assert fwd(nb=nb[0] - 1) == WS and fwd(ws=ws + 4) == WS
        assert fwd(x=x + 4) == UNSUP
        assert fwd(dims=self.dims[:2] + (0,) + self.dims[3:]) == DIM
        assert fwd(slope=-0.5) == UNSUP and fwd(act=2) == UNSUP
        assert bd(y=None) == NULL                                           # act == 1 needs y
        assert bd(dx=None) == NULL and bd(nb=nb[1] - 4) == WS
        assert bw(y=None) == NULL and bw(dw=None) == NULL
        assert bw(nb=nb[2] - 4) == WS and bw(ws=ws + 8) == WS
        torch.cuda.synchronize()
        for t in (self.y, self.dx, self.dw, self.db):
            assert bool((t == 7.0).all())                                   # nothing was launched


def check_family_table(family, declared, launching):
    """every name the family's header declares (``declared``) has a signature in its table and is exported by the library with
    that signature, the table holds nothing else, its launching names are ``launching``, and neither the table nor the header
    shares a name with any other family's"""
    from smilecode_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    path, table = _lib.FAMILIES[family]
    names = _lib.header_symbols(path)
    assert set(names) == set(declared)
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/{os.path.basename(path)} but not exported"
        assert name in table, f"{name} has no ctypes signature"
        fn = getattr(lib, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == table[name][1]
    assert set(table) == set(names)
    for other, (opath, otable) in _lib.FAMILIES.items():
        if other != family:
            assert not set(table) & set(otable), other
            assert not set(names) & set(_lib.header_symbols(opath)), other
    assert sorted(n for n in table if guard.is_launching(n)) == sorted(launching)
    return lib


def check_header_is_c99(family, tmp_path, main_body):
    """a C99 translation unit that includes the family's header and uses it as ``main_body`` compiles without a warning"""
    from smilecode_amd import _lib
    path = _lib.FAMILIES[family][0]
    src = tmp_path / ("use_%s.c" % family)
    src.write_text('#include "%s"\nint main(void) { %s }\n' % (os.path.basename(path), main_body))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(path), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
