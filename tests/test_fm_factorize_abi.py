"""CPU-only: factorize / unfactorize are part of the C ABI -- the four entry points are declared in include/textcomp.h,
exported by libtextcomp.so and typed by the Python binding with the header's arity, and the upper layers expose them."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tc_fm_factorize", "tc_fm_factorize_dev", "tc_fm_unfactorize", "tc_fm_unfactorize_dev")


def _header():
    return open(os.path.join(ROOT, "include", "textcomp.h")).read()


def _arity(name):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, src, flags=re.S)
    assert m, "include/textcomp.h does not declare " + name
    return m.group(1).count(",") + 1


def test_header_declares_the_calls():
    assert [_arity(n) for n in NAMES] == [9, 9, 9, 9]


def test_binding_types_the_calls_with_the_headers_arity():
    from textcomp import _lib
    typed = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for n in NAMES:
        assert n in typed, "textcomp._lib.SYMBOLS lacks " + n
        res, args = typed[n]
        assert res is ctypes.c_int and len(args) == _arity(n)
        assert args[5 if "unfactorize" in n else 4] is ctypes.c_uint64      # npat
        assert args[-1] is ctypes.POINTER(ctypes.c_uint64)                  # the capacity word


def test_library_exports_the_calls():
    import __graft_entry__
    __graft_entry__.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "text-compression_amd", "libtextcomp.so"))
    for n in NAMES:
        assert hasattr(lib, n), "libtextcomp.so lacks " + n


def test_upper_layers_expose_the_operations():
    import textcomp
    from textcomp import fmindex
    for m in ("factorize", "factorize_dev", "unfactorize", "unfactorize_dev"):
        assert callable(getattr(textcomp.FMIndexHandle, m))
    for kind in ("bytestring", "text"):
        for sp in "SP":
            assert callable(getattr(fmindex, "%sFMIndexFactorize%s" % (kind, sp)))
