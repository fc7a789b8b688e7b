"""CPU-only: the unique-substring calls are part of the C ABI -- the six entry points are declared in include/textcomp.h, exported
by libtextcomp.so and typed by the Python binding with the header's arity (tests/test_abi_exports.py holds SYMBOLS to textcomp.h
exactly), textcomp.Context exposes them, and the header's worked examples are what brute force over all substrings says."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"tc_unique_prefixes": 4, "tc_unique_prefixes_dev": 4, "tc_unique_substrings": 8, "tc_unique_substrings_dev": 8,
         "tc_shortest_unique": 5, "tc_shortest_unique_dev": 5}
# the table of include/textcomp.h: text -> (up, MUS, point SUS), as the header prints them
TABLE = {
    "mississippi": ("1 5 4 3 5 4 3 2 2 2 0", "(0,1) (3,3) (7,2) (8,2) (9,2)",
                    "(0,1) (0,2) (0,3) (3,3) (3,3) (3,3) (6,3) (7,2) (7,2) (8,2) (9,2)"),
    "abaab": ("3 2 2 0 0", "(1,2) (2,2)", "(0,3) (1,2) (1,2) (2,2) (2,3)"),
    "banana": ("1 4 3 0 0 0", "(0,1) (2,3)", "(0,1) (0,2) (0,3) (2,3) (2,3) (2,4)"),
    "abcabc": ("4 3 2 0 0 0", "(2,2)", "(0,4) (1,3) (2,2) (2,2) (2,3) (2,4)"),
    "aaaa": ("4 0 0 0", "(0,4)", "(0,4) (0,4) (0,4) (0,4)"),
    "a": ("1", "(0,1)", "(0,1)"),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "textcomp.h")).read(), flags=re.S)


def _arity(name):
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, "include/textcomp.h does not declare " + name
    return m.group(1).count(",") + 1


def test_header_declares_the_calls_and_the_definition():
    assert {n: _arity(n) for n in ARITY} == ARITY
    doc = " ".join(open(os.path.join(ROOT, "include", "textcomp.h")).read().replace("\n *", " ").split())
    for phrase in ("(not part of the reference's surface)", "A substring is UNIQUE when it occurs exactly once", "Occurrences may overlap",
                   "the empty string is never unique", "SHORTEST UNIQUE PREFIX", "up[i] = m + 1 if i + m < n, else 0",
                   "MINIMAL UNIQUE SUBSTRING (MUS)", "The empty string counts as occurring twice",
                   "up[s] != 0 and (s = n - 1, or up[s+1] = 0, or up[s+1] >= up[s])", "No MUS contains another",
                   "capacity n is always enough", "a non-empty text has at least one", "of equal lengths, the one with the smallest s",
                   "(s_k, p - s_k + 1)", "(p, e_k - p + 1)", "sus_start alone may be NULL", "The filters of the list do not apply",
                   "min_len = 0, or a max_len that is neither 0 nor >= min_len: TC_ERR_ARG", "nothing read or written, 0 MUS"):
        assert phrase in doc, phrase
    for text, cols in TABLE.items():                # every row of the table, as printed
        assert " ".join((text,) + cols) in doc, text


def _pairs(s):
    return [tuple(int(x) for x in p.strip("()").split(",")) for p in s.split()]


def test_header_examples_are_the_definitions():
    import sus_ref as S
    for text, (up, mus, point) in TABLE.items():
        assert S.brute(text.encode()) == ([int(x) for x in up.split()], _pairs(mus), _pairs(point)), text
    for text, words in (("mississippi", "m sis ip pp pi"), ("abaab", "ba aa"), ("banana", "b nan"), ("abcabc", "ca")):
        assert [text[s:s + l] for s, l in _pairs(TABLE[text][1])] == words.split()


def test_binding_types_the_calls_with_the_headers_arity():
    from textcomp import _lib
    typed = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for n, k in ARITY.items():
        assert n in typed, "textcomp._lib.SYMBOLS lacks " + n
        res, args = typed[n]
        assert res is ctypes.c_int and len(args) == k
        assert args[0] is ctypes.c_void_p and args[1] is ctypes.c_void_p           # the context, the text
        assert args[2] is ctypes.c_uint64                                           # n
    for n in ("tc_unique_substrings", "tc_unique_substrings_dev"):
        args = typed[n][1]
        assert args[3] is ctypes.c_uint32 and args[4] is ctypes.c_uint32            # min_len, max_len
        assert all(a is ctypes.c_void_p for a in args[5:7])                         # the two arrays
        assert args[7] is ctypes.POINTER(ctypes.c_uint64)                           # the capacity word
    for n in ("tc_unique_prefixes", "tc_unique_prefixes_dev", "tc_shortest_unique", "tc_shortest_unique_dev"):
        assert all(a is ctypes.c_void_p for a in typed[n][1][3:])


def test_library_exports_the_calls():
    import __graft_entry__
    __graft_entry__.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "text-compression_amd", "libtextcomp.so"))
    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    for n, k in ARITY.items():
        assert hasattr(lib, n), "libtextcomp.so lacks " + n
        fn = getattr(lib, n)
        if k == 8:
            fn.argtypes = [P, P, ctypes.c_uint64, U32, U32, P, P, P]
            assert fn(None, None, 0, 1, 0, None, None, None) == -1                  # a null context, before anything else
        else:
            fn.argtypes = [P, P, ctypes.c_uint64] + [P] * (k - 3)
            assert fn(None, None, 0, *([None] * (k - 3))) == -1


def test_context_exposes_the_operations():
    import textcomp
    for m in ("unique_prefixes", "unique_prefixes_dev", "unique_substring_count", "unique_substrings", "unique_substrings_dev",
              "shortest_unique", "shortest_unique_dev"):
        assert callable(getattr(textcomp.Context, m)), m
    for m in ("unique_prefixes", "shortest_unique"):
        assert list(inspect.signature(getattr(textcomp.Context, m)).parameters) == ["self", "text"]
    for m in ("unique_prefixes_dev", "shortest_unique_dev"):
        assert list(inspect.signature(getattr(textcomp.Context, m)).parameters) == ["self", "d_text"]
    for m in ("unique_substring_count", "unique_substrings"):
        sig = inspect.signature(getattr(textcomp.Context, m))
        assert list(sig.parameters) == ["self", "text", "min_len", "max_len"]
        assert (sig.parameters["min_len"].default, sig.parameters["max_len"].default) == (1, 0)
    sig = inspect.signature(textcomp.Context.unique_substrings_dev)
    assert list(sig.parameters) == ["self", "d_text", "min_len", "max_len", "cap"]
    assert (sig.parameters["min_len"].default, sig.parameters["max_len"].default, sig.parameters["cap"].default) == (1, 0, None)
