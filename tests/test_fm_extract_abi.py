"""CPU-only: the text samples and extract exist at every layer that can be looked at without a GPU -- the header declares
them, libtextcomp.so exports them, the ctypes table types them, the Python wrappers take text_rate, the C++ mirror and
the Haskell FFI name them."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tc_fm_build_self", "tc_fm_build_self_dev", "tc_fm_text_rate", "tc_fm_extract", "tc_fm_extract_dev")


def _header():
    src = open(os.path.join(ROOT, "include", "textcomp.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(tc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}
    for name in NEW:
        assert name in protos, name
    for name in ("tc_fm_build_self", "tc_fm_build_self_dev"):
        assert "uint32_t sa_rate" in protos[name] and "uint32_t text_rate" in protos[name] and protos[name].count(",") == 5
    assert protos["tc_fm_extract"].count(",") == protos["tc_fm_extract_dev"].count(",") == 7
    assert re.search(r"uint32_t\s+tc_fm_text_rate", src)


def test_library_exports_them():
    import __graft_entry__
    __graft_entry__.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "text-compression_amd", "libtextcomp.so"))
    for name in NEW:
        assert hasattr(lib, name), "libtextcomp.so lacks %s" % name
    # the two that need no context answer for a null index
    lib.tc_fm_text_rate.restype = ctypes.c_uint32
    lib.tc_fm_text_rate.argtypes = [ctypes.c_void_p]
    lib.tc_fm_device_bytes.restype = ctypes.c_uint64
    lib.tc_fm_device_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.tc_fm_text_rate(None) == 0
    assert lib.tc_fm_device_bytes(None, 2) == 0


def test_python_binding_and_wrappers():
    import textcomp
    from textcomp import _lib
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in NEW:
        assert name in table, name
    assert len(table["tc_fm_build_self"][1]) == 6 and len(table["tc_fm_build_self_dev"][1]) == 6
    assert len(table["tc_fm_extract"][1]) == 8 and len(table["tc_fm_extract_dev"][1]) == 8
    assert table["tc_fm_text_rate"][0] is ctypes.c_uint32
    assert inspect.signature(textcomp.Context.fm_build).parameters["text_rate"].default == 0
    assert inspect.signature(textcomp.Context.fm_build).parameters["sa_rate"].default == 1
    assert inspect.signature(textcomp.Context.fm_build_dev).parameters["text_rate"].default == 0
    assert isinstance(inspect.getattr_static(textcomp.FMIndexHandle, "text_rate"), property)
    assert list(inspect.signature(textcomp.FMIndexHandle.extract).parameters) == ["self", "starts", "lens"]
    assert list(inspect.signature(textcomp.FMIndexHandle.extract_dev).parameters)[:4] == ["self", "d_starts", "d_lens", "nq"]


def test_mirrors_name_them():
    hpp = open(os.path.join(ROOT, "text-compression_amd", "host", "Data", "TextCompression.hpp")).read()
    ffi = open(os.path.join(ROOT, "text-compression_amd", "hs", "Data", "TextCompression", "FFI.hs")).read()
    for name in NEW:
        assert name in hpp, "host/Data/TextCompression.hpp does not use %s" % name
        assert 'foreign import ccall' in ffi and ('"%s"' % name) in ffi, "FFI.hs does not import %s" % name
