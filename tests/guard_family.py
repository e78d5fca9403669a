"""What the tests of the ABI families beside the core share (_lib.FAMILIES: mind, mi, ssim, reg, vecint).

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
