"""CPU-only: the palindromes are part of the C ABI -- the four entry points are declared in include/textcomp.h, exported by
libtextcomp.so and typed by the Python binding with the header's arity (tests/test_abi_exports.py holds SYMBOLS to textcomp.h
exactly), and textcomp.Context exposes them; textcomp.DNA_COMPLEMENT is the involution the header describes."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"tc_palindromes": 10, "tc_palindromes_dev": 10, "tc_longest_palindrome": 8, "tc_longest_palindrome_dev": 8}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "textcomp.h")).read(), flags=re.S)


def _arity(name):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, "include/textcomp.h does not declare " + name
    return m.group(1).count(",") + 1


def test_header_declares_the_calls_and_the_definition():
    assert {n: _arity(n) for n in ARITY} == ARITY
    assert re.search(r"#define\s+TC_PAL_MAX_MISMATCH\s+16\b", _header())
    doc = " ".join(open(os.path.join(ROOT, "include", "textcomp.h")).read().replace("\n *", " ").split())
    for phrase in ("is a SIGMA-PALINDROME with mm mismatches", "c = 2s + len - 1", "its outermost pair matches",
                   "The middle byte of an odd length counts as a pair with itself", "comp is a HOST pointer",
                   "(1,4,0) issi, (1,7,0) ississi, (4,4,0) issi, (7,4,0) ippi", '"ACGT" under the DNA complement: (0,4,0)',
                   "nothing at m = 0; (0,5,1) and (2,3,1) at m = 1", "capacity 2n - 1 is always enough",
                   "of equal lengths the one with the smallest centre"):
        assert phrase in doc, phrase


def test_header_examples_are_the_definitions():
    import pal_ref as R
    assert R.brute(b"mississippi", None, 0, 3) == [(1, 4, 0), (1, 7, 0), (4, 4, 0), (7, 4, 0)]
    assert len(R.brute(b"mississippi")) == 14
    assert R.brute(b"ACGT", R.DNA) == [(0, 4, 0)]
    assert R.brute(b"ACAGT", R.DNA) == [] and R.brute(b"ACAGT", R.DNA, 1) == [(0, 5, 1), (2, 3, 1)]


def test_binding_types_the_calls_with_the_headers_arity():
    from textcomp import _lib
    typed = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for n, k in ARITY.items():
        assert n in typed, "textcomp._lib.SYMBOLS lacks " + n
        res, args = typed[n]
        assert res is ctypes.c_int and len(args) == k
        assert all(a is ctypes.c_void_p for a in (args[0], args[1], args[3]))       # the context, the text, comp
        assert args[2] is ctypes.c_uint64                                           # n
        assert args[4] is ctypes.c_uint32                                           # max_mismatch
    for n in ("tc_palindromes", "tc_palindromes_dev"):
        args = typed[n][1]
        assert args[5] is ctypes.c_uint32                                           # min_len
        assert all(a is ctypes.c_void_p for a in args[6:9])                         # the three arrays
        assert args[-1] is ctypes.POINTER(ctypes.c_uint64)                          # the capacity word
    for n in ("tc_longest_palindrome", "tc_longest_palindrome_dev"):
        assert all(a is ctypes.POINTER(ctypes.c_uint32) for a in typed[n][1][5:])   # three host words
    assert _lib.TC_PAL_MAX_MISMATCH == 16


def test_library_exports_the_calls():
    import __graft_entry__
    __graft_entry__.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "text-compression_amd", "libtextcomp.so"))
    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    for n, k in ARITY.items():
        assert hasattr(lib, n), "libtextcomp.so lacks " + n
        fn = getattr(lib, n)
        if k == 10:
            fn.argtypes = [P, P, ctypes.c_uint64, P, U32, U32, P, P, P, P]
            assert fn(None, None, 0, None, 0, 1, None, None, None, None) == -1      # a null context, before anything else
        else:
            fn.argtypes = [P, P, ctypes.c_uint64, P, U32, P, P, P]
            assert fn(None, None, 0, None, 0, None, None, None) == -1


def test_context_exposes_the_operations():
    import textcomp
    for m in ("palindromes", "palindrome_count", "palindromes_dev", "longest_palindrome", "longest_palindrome_dev"):
        assert callable(getattr(textcomp.Context, m)), m


def test_dna_complement_is_an_involution():
    import textcomp
    t = np.asarray(textcomp.DNA_COMPLEMENT)
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert np.array_equal(t[t], np.arange(256, dtype=np.uint8))
    assert bytes(t[list(b"ACGTacgt")]) == b"TGCAtgca"
    assert sorted(np.nonzero(t != np.arange(256))[0].tolist()) == sorted(b"ACGTacgt")
    import pal_ref
    assert np.array_equal(t, pal_ref.DNA)
