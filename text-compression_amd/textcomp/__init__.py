"""textcomp -- host-side mirror of the reference's Data.BWT / Data.MTF / Data.RLE /
Data.FMIndex surface over libtextcomp.so (HIP, gfx950).

Two levels:
  * `Context`: array-level calls (numpy in / numpy out) straight onto the C ABI.
  * `textcomp.bwt / .mtf / .rle / .fmindex`: functions with the reference's names
    and value shapes (`Seq (Maybe Word8)` = list of int|None, `RLE ByteString` =
    alternating [b"count", symbol] list, ...), for callers and parity tests.

There is no CPU path: without the built library and a usable GPU everything raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Block, Stats, TcError, TcMalformed  # noqa: F401


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


CODINGS = {"packed": _lib.TC_CODING_PACKED, "huffman": _lib.TC_CODING_HUFFMAN}
_CODING_NAMES = {v: k for k, v in CODINGS.items()}


def _coding_id(coding):
    if coding in CODINGS:
        return CODINGS[coding]
    if coding in _CODING_NAMES:
        return coding
    raise ValueError("container coding must be 'packed' or 'huffman', not %r" % (coding,))


def _u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _dna_complement():
    t = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"CG", b"at", b"cg"):
        t[a], t[b] = b, a
    t.setflags(write=False)
    return t


# the comp of the palindrome calls under which they find inverted repeats: A<->T, C<->G, a<->t, c<->g, everything else fixed
DNA_COMPLEMENT = _dna_complement()


# the kinds of the repeat cover: every occurrence of repeated content, or every occurrence but the leftmost
COVER_ALL, COVER_LATER = _lib.TC_COVER_ALL, _lib.TC_COVER_LATER
DOC_OTHER, DOC_EARLIER = _lib.TC_DOC_OTHER, _lib.TC_DOC_EARLIER
ESA_NO_POS = _lib.TC_ESA_NO_POS


def _soft_mask():
    t = np.arange(256, dtype=np.uint8)
    t[ord("A"):ord("Z") + 1] += 32
    t.setflags(write=False)
    return t


# maps of the mask calls: SOFT_MASK lower-cases ASCII letters, hard_mask(b) turns every covered byte into b
SOFT_MASK = _soft_mask()


def hard_mask(byte=b"N"):
    """the 256-byte map that turns every byte into `byte` (an integer or a one-byte string)"""
    b = byte if isinstance(byte, int) else bytes(byte)[0] if len(bytes(byte)) == 1 else None
    if b is None or not 0 <= b <= 255:
        raise ValueError("hard_mask takes one byte")
    return np.full(256, b, dtype=np.uint8)


def _comp(comp):
    """a byte involution as the 256-byte host table the palindrome calls take (None: the identity, a null pointer)"""
    if comp is None:
        return None
    t = _u8(comp)
    if len(t) != 256:
        raise ValueError("comp holds 256 bytes, not %d" % len(t))
    return t


class Context:
    """One device + stream + workspace (`tc_ctx`)."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.tc_ctx_create(device, C.byref(h))
        if rc != 0:
            raise TcError(rc, "tc_ctx_create(device=%d): no usable HIP device" % device)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.tc_last_error(self._h).decode(errors="replace")
            raise (TcMalformed if rc == _lib.TC_ERR_MALFORMED else TcError)(rc, msg)

    @property
    def handle(self):
        return self._h

    @property
    def lib(self):
        return self._lib

    def place_workspace(self, d_text_ptr, n, blk, tries=5):
        """tc_ctx_place_workspace: encode the record at device address d_text_ptr on up to `tries` workspace
        placements, keep the fastest; returns (ms per placement tried, chosen index)."""
        ms = (C.c_double * 8)()
        ch = C.c_int(-1)
        self._check(self._lib.tc_ctx_place_workspace(self._h, C.c_void_p(d_text_ptr), n, C.byref(blk), tries, ms, C.byref(ch)))
        return [x for x in ms if x > 0], ch.value

    # ------------------------------------------------ container coding
    def set_container_coding(self, coding):
        """what the container writers of this context put behind the header: "packed" (the fixed-width
        packings, the default) or "huffman" (run format id 3; textcomp.h).  Readers go by the header."""
        self._check(self._lib.tc_ctx_set_container_coding(self._h, _coding_id(coding)))

    @property
    def container_coding(self):
        return _CODING_NAMES[self._lib.tc_ctx_get_container_coding(self._h)]

    def _with_coding(self, coding):
        """context manager: `coding` (None: leave it) for the duration, the previous value afterwards"""
        import contextlib

        @contextlib.contextmanager
        def cm():
            if coding is None:
                yield
                return
            before = self._lib.tc_ctx_get_container_coding(self._h)
            self.set_container_coding(coding)
            try:
                yield
            finally:
                self._lib.tc_ctx_set_container_coding(self._h, before)
        return cm()

    def stats(self):
        s = Stats()
        self._check(self._lib.tc_get_stats(self._h, C.byref(s)))
        return s

    # ---------------------------------------------------------------- BWT
    def bwt_encode(self, text):
        """-> (L uint8[n+1], primary); empty input -> (empty, None)."""
        t = _u8(text)
        n = len(t)
        if n == 0:
            return np.empty(0, np.uint8), None
        L = np.empty(n + 1, np.uint8)
        prim = C.c_uint64()
        self._check(self._lib.tc_bwt_encode(self._h, _ptr(t), n, _ptr(L), C.byref(prim)))
        return L, int(prim.value)

    def suffix_array(self, text):
        t = _u8(text)
        sa = np.empty(len(t) + 1, np.uint32)
        self._check(self._lib.tc_suffix_array(self._h, _ptr(t) if len(t) else None, len(t), _ptr(sa)))
        return sa

    # ------------------------------------- suffix array + LCP array (the enhanced suffix array)
    def suffix_array_dev(self, d_text):
        """text resident in HBM (a torch uint8 tensor on this context's device) -> its suffix array as an int32 tensor
        of n + 1 entries on the device (the values are < 2^31): tc_suffix_array_dev"""
        import torch
        n = d_text.numel()
        d_sa = torch.empty(n + 1, dtype=torch.int32, device=d_text.device)
        torch.cuda.synchronize()
        self._check(self._lib.tc_suffix_array_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n,
                                                  C.c_void_p(d_sa.data_ptr())))
        return d_sa

    def lcp_array_dev(self, d_text, d_sa):
        """text and its suffix array resident in HBM -> the LCP array, an int32 tensor of n + 1 entries on the device:
        tc_lcp_array_dev.  TcMalformed when d_sa is no permutation of 0 .. n."""
        import torch
        n = d_text.numel()
        if d_sa.numel() != n + 1 or d_sa.element_size() != 4:
            raise ValueError("d_sa must hold n + 1 32-bit entries")
        d_lcp = torch.empty(n + 1, dtype=torch.int32, device=d_text.device)
        torch.cuda.synchronize()
        self._check(self._lib.tc_lcp_array_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n,
                                               C.c_void_p(d_sa.data_ptr()), C.c_void_p(d_lcp.data_ptr())))
        return d_lcp

    def lcp_summary_dev(self, d_lcp):
        """an LCP array resident in HBM -> (largest entry, smallest row holding it, sum of all entries):
        tc_lcp_summary_dev"""
        import torch
        mx, row, tot = C.c_uint32(), C.c_uint64(), C.c_uint64()
        torch.cuda.synchronize()
        self._check(self._lib.tc_lcp_summary_dev(self._h, C.c_void_p(d_lcp.data_ptr()), d_lcp.numel(), C.byref(mx),
                                                 C.byref(row), C.byref(tot)))
        return int(mx.value), int(row.value), int(tot.value)

    def lcp_array(self, text):
        """-> (sa, lcp), two uint32 arrays of n + 1 entries: lcp[0] = 0, lcp[j] = longest common prefix of the suffixes
        at sa[j - 1] and sa[j] (tc_lcp_array)."""
        t = _u8(text)
        sa = np.empty(len(t) + 1, np.uint32)
        lcp = np.empty(len(t) + 1, np.uint32)
        self._check(self._lib.tc_lcp_array(self._h, _ptr(t) if len(t) else None, len(t), _ptr(sa), _ptr(lcp)))
        return sa, lcp

    def _esa_dev(self, text):
        import torch
        t = _u8(text)
        d_text = torch.from_numpy(t.copy()).to("cuda:%d" % self.device)
        d_sa = self.suffix_array_dev(d_text)
        return d_sa, self.lcp_array_dev(d_text, d_sa)

    def longest_repeat(self, text):
        """-> (pos_a, pos_b, length), 0-based: text[pos_a : pos_a + length] == text[pos_b : pos_b + length] is a longest
        substring that occurs twice (the two may overlap); of several the one first in suffix-array order: rows
        row - 1 and row of the suffix array, row from tc_lcp_summary_dev.  No byte occurs twice: (0, 0, 0)."""
        d_sa, d_lcp = self._esa_dev(text)
        length, row, _ = self.lcp_summary_dev(d_lcp)
        if length == 0:
            return 0, 0, 0
        pair = d_sa[row - 1:row + 1].cpu().tolist()
        return int(pair[0]), int(pair[1]), length

    def distinct_substrings(self, text):
        """number of distinct non-empty substrings of text: n (n + 1) / 2 - sum(lcp)"""
        n = len(_u8(text))
        _, d_lcp = self._esa_dev(text)
        return n * (n + 1) // 2 - self.lcp_summary_dev(d_lcp)[2]

    # ------------------------------------- LPF array, LZ77 parse of a text against itself, and its inverse
    def lpf_array(self, text):
        """-> (lpf, src), two uint32 arrays of n entries, 0-based: lpf[i] = the longest prefix of text[i:] that also starts
        at some j < i (the source may overlap), src[i] = such a j (0 where lpf[i] = 0): tc_lpf_array"""
        t = _u8(text)
        lpf = np.empty(len(t), np.uint32)
        src = np.empty(len(t), np.uint32)
        if len(t) == 0:
            return lpf, src
        self._check(self._lib.tc_lpf_array(self._h, _ptr(t) if len(t) else None, len(t), _ptr(lpf), _ptr(src)))
        return lpf, src

    def lz_phrase_count(self, text):
        """the number z of phrases of the LZ77 parse of text (the sizes-only form of tc_lz_parse)"""
        t = _u8(text)
        nph = C.c_uint64(0)
        self._check(self._lib.tc_lz_parse(self._h, _ptr(t) if len(t) else None, len(t), None, None, C.byref(nph)))
        return int(nph.value)

    def lz_parse(self, text):
        """the greedy left-to-right LZ77 parse of text against itself -> (ph_src, ph_len), two uint32 arrays of z entries:
        a copy is (0-based source position, length >= 1), a literal (byte value, 0): tc_lz_parse"""
        t = _u8(text)
        cap = max(self.lz_phrase_count(t), 1)
        ph_src = np.empty(cap, np.uint32)
        ph_len = np.empty(cap, np.uint32)
        nph = C.c_uint64(cap)
        self._check(self._lib.tc_lz_parse(self._h, _ptr(t) if len(t) else None, len(t), _ptr(ph_src), _ptr(ph_len), C.byref(nph)))
        return ph_src[:int(nph.value)].copy(), ph_len[:int(nph.value)].copy()

    def lz_unparse(self, ph_src, ph_len):
        """the inverse of lz_parse -> bytes: tc_lz_unparse.  TcError (TC_ERR_ARG) for a list no parse is."""
        ps = np.ascontiguousarray(ph_src, dtype=np.uint32)
        pl = np.ascontiguousarray(ph_len, dtype=np.uint32)
        if ps.ndim != 1 or ps.shape != pl.shape:
            raise ValueError("ph_src and ph_len of one length")
        nph = len(ps)
        if nph == 0:
            return b""
        nb = C.c_uint64(0)
        self._check(self._lib.tc_lz_unparse(self._h, _ptr(ps), _ptr(pl), nph, None, C.byref(nb)))
        out = np.empty(int(nb.value), np.uint8)
        self._check(self._lib.tc_lz_unparse(self._h, _ptr(ps), _ptr(pl), nph, _ptr(out), C.byref(nb)))
        return out[:int(nb.value)].tobytes()

    def lpf_array_dev(self, d_text, src=True):
        """text resident in HBM (a torch uint8 tensor on this context's device) -> (lpf, src), two int32 tensors of n
        entries on the device (src None when not asked for): tc_lpf_array_dev"""
        import torch
        n = d_text.numel()
        d_lpf = torch.empty(n, dtype=torch.int32, device=d_text.device)
        d_src = torch.empty(n, dtype=torch.int32, device=d_text.device) if src else None
        if n == 0:
            return d_lpf, d_src
        torch.cuda.synchronize()
        self._check(self._lib.tc_lpf_array_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n,
                                               C.c_void_p(d_lpf.data_ptr()), C.c_void_p(d_src.data_ptr()) if src else None))
        return d_lpf, d_src

    def lz_parse_dev(self, d_text, cap=None):
        """text resident in HBM -> (ph_src, ph_len), two int32 tensors of z entries on the device: tc_lz_parse_dev.  cap:
        the phrase slots to try first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        torch.cuda.synchronize()
        if cap is None:
            nph = C.c_uint64(0)
            self._check(self._lib.tc_lz_parse_dev(self._h, pt, n, None, None, C.byref(nph)))
            cap = int(nph.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            ph_src = torch.empty(cap, dtype=torch.int32, device=d_text.device)
            ph_len = torch.empty(cap, dtype=torch.int32, device=d_text.device)
            torch.cuda.synchronize()
            nph = C.c_uint64(cap)
            rc = self._lib.tc_lz_parse_dev(self._h, pt, n, C.c_void_p(ph_src.data_ptr()), C.c_void_p(ph_len.data_ptr()), C.byref(nph))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nph.value), 1)
        self._check(rc)
        return ph_src[:int(nph.value)], ph_len[:int(nph.value)]

    def lz_unparse_dev(self, d_ph_src, d_ph_len, cap=None):
        """a phrase list resident in HBM (two 32-bit tensors of one length) -> the text, a uint8 tensor on the device:
        tc_lz_unparse_dev.  cap: the bytes to try first (None: the sizes-only form runs first)"""
        import torch
        if d_ph_src.numel() != d_ph_len.numel() or d_ph_src.element_size() != 4 or d_ph_len.element_size() != 4:
            raise ValueError("d_ph_src and d_ph_len must hold the same number of 32-bit entries")
        nph = d_ph_src.numel()
        dev = d_ph_src.device
        if nph == 0:
            return torch.zeros(0, dtype=torch.uint8, device=dev)
        ps, pl = C.c_void_p(d_ph_src.data_ptr()), C.c_void_p(d_ph_len.data_ptr())
        torch.cuda.synchronize()
        if cap is None:
            nb = C.c_uint64(0)
            self._check(self._lib.tc_lz_unparse_dev(self._h, ps, pl, nph, None, C.byref(nb)))
            cap = int(nb.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            nb = C.c_uint64(cap)
            rc = self._lib.tc_lz_unparse_dev(self._h, ps, pl, nph, C.c_void_p(out.data_ptr()), C.byref(nb))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nb.value), 1)
        self._check(rc)
        return out[:int(nb.value)]

    # ------------------------------------- maximal and supermaximal repeats of a text
    def repeat_count(self, text, min_len=1, min_occ=2, supermaximal=False):
        """the number of (super)maximal repeats of text with len >= min_len and occ >= min_occ (the sizes-only form of
        tc_repeats)"""
        t = _u8(text)
        nrep = C.c_uint64(0)
        self._check(self._lib.tc_repeats(self._h, _ptr(t) if len(t) else None, len(t), int(bool(supermaximal)), min_len, min_occ,
                                         None, None, None, None, None, C.byref(nrep)))
        return int(nrep.value)

    def repeats(self, text, min_len=1, min_occ=2, supermaximal=False, with_sa=False):
        """the maximal (or supermaximal) repeats of text -> (pos, len, occ, row[, sa]), uint32 arrays: repeat k is
        text[pos[k] : pos[k] + len[k]], it occurs occ[k] times, at sa[row[k] : row[k] + occ[k]]; listed by representative
        row (include/textcomp.h), which is not the order of row: tc_repeats"""
        t = _u8(text)
        kind = int(bool(supermaximal))
        cap = max(self.repeat_count(t, min_len, min_occ, supermaximal), 1)
        pos, ln, occ, row = (np.empty(cap, np.uint32) for _ in range(4))
        sa = np.empty(len(t) + 1, np.uint32) if with_sa else None
        nrep = C.c_uint64(cap)
        self._check(self._lib.tc_repeats(self._h, _ptr(t) if len(t) else None, len(t), kind, min_len, min_occ,
                                         _ptr(sa) if with_sa else None, _ptr(pos), _ptr(ln), _ptr(occ), _ptr(row), C.byref(nrep)))
        k = int(nrep.value)
        out = (pos[:k].copy(), ln[:k].copy(), occ[:k].copy(), row[:k].copy())
        return out + (sa,) if with_sa else out

    def repeats_dev(self, d_text, min_len=1, min_occ=2, supermaximal=False, with_sa=False, cap=None):
        """text resident in HBM -> (pos, len, occ, row[, sa]), int32 tensors on the device: tc_repeats_dev.  cap: the
        repeat slots to try first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        kind = int(bool(supermaximal))
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        d_sa = torch.empty(n + 1, dtype=torch.int32, device=d_text.device) if with_sa else None
        psa = C.c_void_p(d_sa.data_ptr()) if with_sa else None
        torch.cuda.synchronize()
        if cap is None:
            nrep = C.c_uint64(0)
            self._check(self._lib.tc_repeats_dev(self._h, pt, n, kind, min_len, min_occ, None, None, None, None, None, C.byref(nrep)))
            cap = int(nrep.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=d_text.device) for _ in range(4)]
            torch.cuda.synchronize()
            nrep = C.c_uint64(cap)
            rc = self._lib.tc_repeats_dev(self._h, pt, n, kind, min_len, min_occ, psa, *(C.c_void_p(o.data_ptr()) for o in out),
                                          C.byref(nrep))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nrep.value), 1)
        self._check(rc)
        res = tuple(o[:int(nrep.value)] for o in out)
        return res + (d_sa,) if with_sa else res

    # ------------------------------------- tandem repeats: the runs (maximal repetitions) of a text
    def tandem_repeat_count(self, text, min_period=1, max_period=0, min_copies=2, min_len=1):
        """the number of runs of text that pass the four filters (the sizes-only form of tc_tandem_repeats)"""
        t = _u8(text)
        nrun = C.c_uint64(0)
        self._check(self._lib.tc_tandem_repeats(self._h, _ptr(t) if len(t) else None, len(t), min_period, max_period, min_copies,
                                                min_len, None, None, None, C.byref(nrun)))
        return int(nrun.value)

    def tandem_repeats(self, text, min_period=1, max_period=0, min_copies=2, min_len=1):
        """the runs of text -> (start, len, period), uint32 arrays: run k is text[start[k] : start[k] + len[k]], whose
        smallest period is period[k] and which extends neither way; by increasing start, then period.  max_period = 0: no
        limit; a run passes with len // period >= min_copies: tc_tandem_repeats"""
        t = _u8(text)
        cap = max(self.tandem_repeat_count(t, min_period, max_period, min_copies, min_len), 1)
        start, ln, period = (np.empty(cap, np.uint32) for _ in range(3))
        nrun = C.c_uint64(cap)
        self._check(self._lib.tc_tandem_repeats(self._h, _ptr(t) if len(t) else None, len(t), min_period, max_period, min_copies,
                                                min_len, _ptr(start), _ptr(ln), _ptr(period), C.byref(nrun)))
        k = int(nrun.value)
        return start[:k].copy(), ln[:k].copy(), period[:k].copy()

    def tandem_repeats_dev(self, d_text, min_period=1, max_period=0, min_copies=2, min_len=1, cap=None):
        """text resident in HBM -> (start, len, period), int32 tensors on the device: tc_tandem_repeats_dev.  cap: the run
        slots to try first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        torch.cuda.synchronize()
        if cap is None:
            nrun = C.c_uint64(0)
            self._check(self._lib.tc_tandem_repeats_dev(self._h, pt, n, min_period, max_period, min_copies, min_len, None, None, None,
                                                        C.byref(nrun)))
            cap = int(nrun.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=d_text.device) for _ in range(3)]
            torch.cuda.synchronize()
            nrun = C.c_uint64(cap)
            rc = self._lib.tc_tandem_repeats_dev(self._h, pt, n, min_period, max_period, min_copies, min_len,
                                                 *(C.c_void_p(o.data_ptr()) for o in out), C.byref(nrun))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nrun.value), 1)
        self._check(rc)
        return tuple(o[:int(nrun.value)] for o in out)

    # ------------------------------------- palindromes and inverted repeats of a text, with mismatches
    def palindrome_count(self, text, comp=None, max_mismatch=0, min_len=1):
        """the number of palindromes of text under comp that tc_palindromes reports (its sizes-only form)"""
        t, c = _u8(text), _comp(comp)
        npal = C.c_uint64(0)
        self._check(self._lib.tc_palindromes(self._h, _ptr(t) if len(t) else None, len(t), _ptr(c), max_mismatch, min_len, None, None,
                                             None, C.byref(npal)))
        return int(npal.value)

    def palindromes(self, text, comp=None, max_mismatch=0, min_len=1):
        """for every centre the longest palindrome of text under the byte involution comp (None: the identity;
        DNA_COMPLEMENT: inverted repeats) with at most max_mismatch mismatching pairs, a matching outermost pair and at least
        min_len bytes -> (start, len, mm), uint32 arrays by increasing centre 2 start + len - 1: tc_palindromes"""
        t, c = _u8(text), _comp(comp)
        cap = max(self.palindrome_count(t, c, max_mismatch, min_len), 1)
        start, ln, mm = (np.empty(cap, np.uint32) for _ in range(3))
        npal = C.c_uint64(cap)
        self._check(self._lib.tc_palindromes(self._h, _ptr(t) if len(t) else None, len(t), _ptr(c), max_mismatch, min_len, _ptr(start),
                                             _ptr(ln), _ptr(mm), C.byref(npal)))
        k = int(npal.value)
        return start[:k].copy(), ln[:k].copy(), mm[:k].copy()

    def palindromes_dev(self, d_text, comp=None, max_mismatch=0, min_len=1, cap=None):
        """text resident in HBM -> (start, len, mm), int32 tensors on the device: tc_palindromes_dev.  comp stays a host
        table; cap: the slots to try first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        c = _comp(comp)
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        torch.cuda.synchronize()
        if cap is None:
            npal = C.c_uint64(0)
            self._check(self._lib.tc_palindromes_dev(self._h, pt, n, _ptr(c), max_mismatch, min_len, None, None, None, C.byref(npal)))
            cap = int(npal.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=d_text.device) for _ in range(3)]
            torch.cuda.synchronize()
            npal = C.c_uint64(cap)
            rc = self._lib.tc_palindromes_dev(self._h, pt, n, _ptr(c), max_mismatch, min_len, *(C.c_void_p(o.data_ptr()) for o in out),
                                              C.byref(npal))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(npal.value), 1)
        self._check(rc)
        return tuple(o[:int(npal.value)] for o in out)

    def longest_palindrome(self, text, comp=None, max_mismatch=0):
        """(start, len, mm) of the longest palindrome of text under comp, of equal lengths the one with the smallest centre;
        len = 0 when there is none: tc_longest_palindrome"""
        t, c = _u8(text), _comp(comp)
        start, ln, mm = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.tc_longest_palindrome(self._h, _ptr(t) if len(t) else None, len(t), _ptr(c), max_mismatch,
                                                    C.byref(start), C.byref(ln), C.byref(mm)))
        return int(start.value), int(ln.value), int(mm.value)

    def longest_palindrome_dev(self, d_text, comp=None, max_mismatch=0):
        """text resident in HBM -> (start, len, mm), host integers: tc_longest_palindrome_dev"""
        import torch
        n = d_text.numel()
        c = _comp(comp)
        torch.cuda.synchronize()
        start, ln, mm = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.tc_longest_palindrome_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n, _ptr(c), max_mismatch,
                                                        C.byref(start), C.byref(ln), C.byref(mm)))
        return int(start.value), int(ln.value), int(mm.value)

    # ------------------------------------- the minimal absent words of a text
    def absent_word_count(self, text, min_len=2, max_len=0):
        """the number of minimal absent words of text with min_len <= len (<= max_len unless that is 0): the sizes-only form
        of tc_absent_words"""
        t = _u8(text)
        nmaw = C.c_uint64(0)
        self._check(self._lib.tc_absent_words(self._h, _ptr(t) if len(t) else None, len(t), min_len, max_len, None, None, None,
                                              C.byref(nmaw)))
        return int(nmaw.value)

    def absent_words(self, text, min_len=2, max_len=0):
        """the minimal absent words of text -> (left uint8, pos uint32, len uint32): word k is the byte left[k] followed by
        text[pos[k] : pos[k] + len[k] - 1]; it does not occur in text, while it does without its first and without its last
        byte.  In the row order of include/textcomp.h, not sorted by word; max_len = 0: no limit: tc_absent_words"""
        t = _u8(text)
        cap = max(self.absent_word_count(t, min_len, max_len), 1)
        left, pos, ln = np.empty(cap, np.uint8), np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        nmaw = C.c_uint64(cap)
        self._check(self._lib.tc_absent_words(self._h, _ptr(t) if len(t) else None, len(t), min_len, max_len, _ptr(left), _ptr(pos),
                                              _ptr(ln), C.byref(nmaw)))
        k = int(nmaw.value)
        return left[:k].copy(), pos[:k].copy(), ln[:k].copy()

    def absent_words_dev(self, d_text, min_len=2, max_len=0, cap=None):
        """text resident in HBM -> (left uint8, pos int32, len int32), tensors on the device: tc_absent_words_dev.  cap: the
        word slots to try first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        torch.cuda.synchronize()
        if cap is None:
            nmaw = C.c_uint64(0)
            self._check(self._lib.tc_absent_words_dev(self._h, pt, n, min_len, max_len, None, None, None, C.byref(nmaw)))
            cap = int(nmaw.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=dt, device=d_text.device) for dt in (torch.uint8, torch.int32, torch.int32)]
            torch.cuda.synchronize()
            nmaw = C.c_uint64(cap)
            rc = self._lib.tc_absent_words_dev(self._h, pt, n, min_len, max_len, *(C.c_void_p(o.data_ptr()) for o in out),
                                               C.byref(nmaw))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nmaw.value), 1)
        self._check(rc)
        return tuple(o[:int(nmaw.value)] for o in out)

    def absent_word_profile(self, text, kmax):
        """-> (hist, total): hist[l] = the number of minimal absent words of length l <= kmax (a uint64 array of kmax + 1
        entries), total = those of every length: tc_absent_word_profile"""
        t = _u8(text)
        hist = np.zeros(max(int(kmax), 0) + 1, np.uint64)
        total = C.c_uint64(0)
        self._check(self._lib.tc_absent_word_profile(self._h, _ptr(t) if len(t) else None, len(t), kmax, _ptr(hist), C.byref(total)))
        return hist, int(total.value)

    def absent_word_profile_dev(self, d_text, kmax):
        """text resident in HBM -> (hist, an int64 tensor of kmax + 1 entries on the device, total): tc_absent_word_profile_dev"""
        import torch
        n = d_text.numel()
        hist = torch.zeros(max(int(kmax), 0) + 1, dtype=torch.int64, device=d_text.device)
        torch.cuda.synchronize()
        total = C.c_uint64(0)
        self._check(self._lib.tc_absent_word_profile_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n, kmax,
                                                         C.c_void_p(hist.data_ptr()), C.byref(total)))
        return hist, int(total.value)

    # ------------------------------------- what is unique in a text: prefixes, minimal unique substrings, point SUS
    def unique_prefixes(self, text):
        """up, a uint32 array: up[i] = the length of the shortest substring that starts at i and occurs once in text, 0 where
        even the whole suffix occurs again: tc_unique_prefixes"""
        t = _u8(text)
        up = np.empty(len(t), np.uint32)
        self._check(self._lib.tc_unique_prefixes(self._h, _ptr(t) if len(t) else None, len(t), _ptr(up) if len(t) else None))
        return up

    def unique_prefixes_dev(self, d_text):
        """text resident in HBM -> up, an int32 tensor on the device: tc_unique_prefixes_dev"""
        import torch
        n = d_text.numel()
        up = torch.empty(n, dtype=torch.int32, device=d_text.device)
        torch.cuda.synchronize()
        self._check(self._lib.tc_unique_prefixes_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n,
                                                     C.c_void_p(up.data_ptr()) if n else None))
        return up

    def unique_substring_count(self, text, min_len=1, max_len=0):
        """the number of minimal unique substrings of text with min_len <= len (<= max_len unless that is 0): the sizes-only
        form of tc_unique_substrings"""
        t = _u8(text)
        nmus = C.c_uint64(0)
        self._check(self._lib.tc_unique_substrings(self._h, _ptr(t) if len(t) else None, len(t), min_len, max_len, None, None,
                                                   C.byref(nmus)))
        return int(nmus.value)

    def unique_substrings(self, text, min_len=1, max_len=0):
        """the minimal unique substrings of text -> (start, len), uint32 arrays: text[start[k] : start[k] + len[k]] occurs
        once, while it occurs again without its first and without its last byte; by increasing start (and end).  max_len = 0:
        no limit: tc_unique_substrings"""
        t = _u8(text)
        cap = max(self.unique_substring_count(t, min_len, max_len), 1)
        start, ln = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        nmus = C.c_uint64(cap)
        self._check(self._lib.tc_unique_substrings(self._h, _ptr(t) if len(t) else None, len(t), min_len, max_len, _ptr(start),
                                                   _ptr(ln), C.byref(nmus)))
        k = int(nmus.value)
        return start[:k].copy(), ln[:k].copy()

    def unique_substrings_dev(self, d_text, min_len=1, max_len=0, cap=None):
        """text resident in HBM -> (start, len), int32 tensors on the device: tc_unique_substrings_dev.  cap: the slots to try
        first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        torch.cuda.synchronize()
        if cap is None:
            nmus = C.c_uint64(0)
            self._check(self._lib.tc_unique_substrings_dev(self._h, pt, n, min_len, max_len, None, None, C.byref(nmus)))
            cap = int(nmus.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=d_text.device) for _ in range(2)]
            torch.cuda.synchronize()
            nmus = C.c_uint64(cap)
            rc = self._lib.tc_unique_substrings_dev(self._h, pt, n, min_len, max_len, *(C.c_void_p(o.data_ptr()) for o in out),
                                                    C.byref(nmus))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nmus.value), 1)
        self._check(rc)
        return tuple(o[:int(nmus.value)] for o in out)

    def shortest_unique(self, text):
        """for every position p the shortest substring of text that covers p and occurs once, of equal lengths the leftmost
        -> (start, len), uint32 arrays of len(text) entries: tc_shortest_unique"""
        t = _u8(text)
        start, ln = np.empty(len(t), np.uint32), np.empty(len(t), np.uint32)
        self._check(self._lib.tc_shortest_unique(self._h, _ptr(t) if len(t) else None, len(t), _ptr(start) if len(t) else None,
                                                 _ptr(ln) if len(t) else None))
        return start, ln

    def shortest_unique_dev(self, d_text):
        """text resident in HBM -> (start, len), int32 tensors on the device: tc_shortest_unique_dev"""
        import torch
        n = d_text.numel()
        start, ln = (torch.empty(n, dtype=torch.int32, device=d_text.device) for _ in range(2))
        torch.cuda.synchronize()
        self._check(self._lib.tc_shortest_unique_dev(self._h, C.c_void_p(d_text.data_ptr()) if n else None, n,
                                                     C.c_void_p(start.data_ptr()) if n else None, C.c_void_p(ln.data_ptr()) if n else None))
        return start, ln

    # ------------------------------------- the repeat cover of a text: spans, mask, dedup; the same over an array of lengths
    @staticmethod
    def _cover_map(map):
        if map is None:
            return None
        m = np.ascontiguousarray(np.frombuffer(bytes(map), np.uint8) if isinstance(map, (bytes, bytearray)) else map, dtype=np.uint8)
        if m.shape != (256,):
            raise ValueError("map must hold 256 bytes")
        return m

    def repeat_cover_count(self, text, min_len, min_occ=2, kind=COVER_ALL):
        """(spans, covered): how many maximal runs of repeated content text has, and how many bytes they hold -- a byte is
        covered when it lies in a stretch of min_len bytes that occurs min_occ times (COVER_LATER: and has occurred before):
        the sizes-only form of tc_repeat_spans"""
        t = _u8(text)
        ns, cov = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.tc_repeat_spans(self._h, _ptr(t) if len(t) else None, len(t), min_len, min_occ, kind, None, None,
                                              C.byref(ns), C.byref(cov)))
        return int(ns.value), int(cov.value)

    def repeat_spans(self, text, min_len, min_occ=2, kind=COVER_ALL):
        """the maximal runs of covered bytes -> (start, len, covered): uint32 arrays in increasing start and the sum of len:
        tc_repeat_spans"""
        t = _u8(text)
        cap = max(self.repeat_cover_count(t, min_len, min_occ, kind)[0], 1)
        start, ln = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        ns, cov = C.c_uint64(cap), C.c_uint64(0)
        self._check(self._lib.tc_repeat_spans(self._h, _ptr(t) if len(t) else None, len(t), min_len, min_occ, kind, _ptr(start),
                                              _ptr(ln), C.byref(ns), C.byref(cov)))
        k = int(ns.value)
        return start[:k].copy(), ln[:k].copy(), int(cov.value)

    def repeat_mask(self, text, min_len, min_occ=2, kind=COVER_ALL, map=None):
        """-> (out, covered): out[p] = map[text[p]] where p is covered and text[p] elsewhere (map: 256 bytes, such as SOFT_MASK
        or hard_mask(b"N")); map None: out[p] = 1 / 0, the cover itself: tc_repeat_mask"""
        t, m = _u8(text), self._cover_map(map)
        out = np.empty(len(t), np.uint8)
        cov = C.c_uint64(0)
        self._check(self._lib.tc_repeat_mask(self._h, _ptr(t) if len(t) else None, len(t), min_len, min_occ, kind,
                                             _ptr(m) if m is not None else None, _ptr(out) if len(t) else None, C.byref(cov)))
        return out, int(cov.value)

    def repeat_dedup(self, text, min_len, min_occ=2, kind=COVER_LATER):
        """-> (out, covered): the text without its covered bytes, a uint8 array of len(text) - covered entries.  COVER_LATER
        keeps the first copy of everything; the result may hold new repeats across the cuts: tc_repeat_dedup"""
        t = _u8(text)
        out = np.empty(max(len(t), 1), np.uint8)
        nout, cov = C.c_uint64(len(t)), C.c_uint64(0)
        self._check(self._lib.tc_repeat_dedup(self._h, _ptr(t) if len(t) else None, len(t), min_len, min_occ, kind, _ptr(out),
                                              C.byref(nout), C.byref(cov)))
        return out[:int(nout.value)].copy(), int(cov.value)

    def _spans_retry(self, call, device, cap):
        """the capacity protocol of the device span lists: call(start, len, nspans, covered) -> rc; cap None: sizes first"""
        import torch
        torch.cuda.synchronize()
        cov = C.c_uint64(0)
        if cap is None:
            ns = C.c_uint64(0)
            self._check(call(None, None, C.byref(ns), C.byref(cov)))
            cap = int(ns.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=device) for _ in range(2)]
            torch.cuda.synchronize()
            ns = C.c_uint64(cap)
            rc = call(*(C.c_void_p(o.data_ptr()) for o in out), C.byref(ns), C.byref(cov))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(ns.value), 1)
        self._check(rc)
        return out[0][:int(ns.value)], out[1][:int(ns.value)], int(cov.value)

    def repeat_spans_dev(self, d_text, min_len, min_occ=2, kind=COVER_ALL, cap=None):
        """text resident in HBM -> (start, len, covered), int32 tensors on the device and a host integer: tc_repeat_spans_dev.
        cap: the slots to try first (None: the sizes-only form runs first)"""
        n, pt = d_text.numel(), self._dev_ptr(d_text)
        return self._spans_retry(lambda s, l, ns, cv: self._lib.tc_repeat_spans_dev(self._h, pt, n, min_len, min_occ, kind, s, l, ns, cv),
                                 d_text.device, cap)

    def repeat_cover_count_dev(self, d_text, min_len, min_occ=2, kind=COVER_ALL):
        """text resident in HBM -> (spans, covered): the sizes-only form of tc_repeat_spans_dev"""
        import torch
        ns, cov = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize()
        self._check(self._lib.tc_repeat_spans_dev(self._h, self._dev_ptr(d_text), d_text.numel(), min_len, min_occ, kind, None, None,
                                                  C.byref(ns), C.byref(cov)))
        return int(ns.value), int(cov.value)

    def repeat_mask_dev(self, d_text, min_len, min_occ=2, kind=COVER_ALL, map=None):
        """text resident in HBM -> (out, covered), a uint8 tensor on the device and a host integer: tc_repeat_mask_dev"""
        import torch
        n, m = d_text.numel(), self._cover_map(map)
        out = torch.empty(n, dtype=torch.uint8, device=d_text.device)
        cov = C.c_uint64(0)
        torch.cuda.synchronize()
        self._check(self._lib.tc_repeat_mask_dev(self._h, self._dev_ptr(d_text), n, min_len, min_occ, kind,
                                                 _ptr(m) if m is not None else None, self._dev_ptr(out), C.byref(cov)))
        return out, int(cov.value)

    def _dedup_retry(self, call, device, cap):
        """the capacity protocol of the device dedups: call(out, nout, covered) -> rc; cap None: sizes first"""
        import torch
        torch.cuda.synchronize()
        cov = C.c_uint64(0)
        if cap is None:
            nout = C.c_uint64(0)
            self._check(call(None, C.byref(nout), C.byref(cov)))
            cap = int(nout.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = torch.empty(cap, dtype=torch.uint8, device=device)
            torch.cuda.synchronize()
            nout = C.c_uint64(cap)
            rc = call(C.c_void_p(out.data_ptr()), C.byref(nout), C.byref(cov))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nout.value), 1)
        self._check(rc)
        return out[:int(nout.value)], int(cov.value)

    def repeat_dedup_dev(self, d_text, min_len, min_occ=2, kind=COVER_LATER, cap=None):
        """text resident in HBM -> (out, covered), a uint8 tensor on the device and a host integer: tc_repeat_dedup_dev.  cap: the
        bytes to try first (None: the sizes-only form runs first; d_text.numel() is always enough)"""
        n, pt = d_text.numel(), self._dev_ptr(d_text)
        return self._dedup_retry(lambda o, no, cv: self._lib.tc_repeat_dedup_dev(self._h, pt, n, min_len, min_occ, kind, o, no, cv),
                                 d_text.device, cap)

    @staticmethod
    def _len_words(d_len):
        if d_len.element_size() != 4:
            raise ValueError("d_len must hold 32-bit entries")
        return d_len.numel()

    def cover_spans_dev(self, d_len, min_len, cap=None):
        """an array of lengths resident in HBM (a 32-bit tensor: lpf_array_dev's, text_match_stats_dev's ms_len, or any other)
        -> (start, len, covered): position i counts iff len[i] >= min_len and covers [i, i + len[i]): tc_cover_spans_dev"""
        n, pl = self._len_words(d_len), self._dev_ptr(d_len)
        return self._spans_retry(lambda s, l, ns, cv: self._lib.tc_cover_spans_dev(self._h, pl, n, min_len, s, l, ns, cv), d_len.device, cap)

    def cover_mask_dev(self, d_len, d_text, min_len, map=None):
        """-> (out, covered): the mask of d_text (a uint8 tensor of d_len.numel() bytes; may be None without a map) under the
        cover of d_len: tc_cover_mask_dev"""
        import torch
        n, m = self._len_words(d_len), self._cover_map(map)
        if d_text is not None and d_text.numel() != n:
            raise ValueError("d_text and d_len must have one length")
        out = torch.empty(n, dtype=torch.uint8, device=d_len.device)
        cov = C.c_uint64(0)
        torch.cuda.synchronize()
        self._check(self._lib.tc_cover_mask_dev(self._h, self._dev_ptr(d_len), self._dev_ptr(d_text) if d_text is not None else None, n,
                                                min_len, _ptr(m) if m is not None else None, self._dev_ptr(out), C.byref(cov)))
        return out, int(cov.value)

    def cover_dedup_dev(self, d_len, d_text, min_len, cap=None):
        """-> (out, covered): d_text without the bytes the cover of d_len holds: tc_cover_dedup_dev"""
        n = self._len_words(d_len)
        if d_text.numel() != n:
            raise ValueError("d_text and d_len must have one length")
        pl, pt = self._dev_ptr(d_len), self._dev_ptr(d_text)
        return self._dedup_retry(lambda o, no, cv: self._lib.tc_cover_dedup_dev(self._h, pl, pt, n, min_len, o, no, cv), d_len.device, cap)

    def text_cover_dev(self, d_query, d_target, min_len):
        """the two texts resident in HBM -> (start, len, covered): the maximal stretches of d_query made of substrings of at
        least min_len bytes that occur in d_target: text_match_stats_dev(pos=False, occ=False), then cover_spans_dev"""
        ms_len = self.text_match_stats_dev(d_query, d_target, pos=False, occ=False)[0]
        return self.cover_spans_dev(ms_len, min_len)

    # ------------------------------------- the k-mers of a text: list, abundance spectrum, all-k profile
    def kmer_count(self, text, k, min_occ=1, max_occ=0):
        """how many distinct k-mers of text occur at least min_occ and (max_occ > 0) at most max_occ times: the
        sizes-only form of tc_kmers"""
        t = _u8(text)
        nk = C.c_uint64(0)
        self._check(self._lib.tc_kmers(self._h, _ptr(t) if len(t) else None, len(t), k, min_occ, max_occ, None, None, None, None,
                                       C.byref(nk)))
        return int(nk.value)

    def kmers(self, text, k, min_occ=1, max_occ=0, with_sa=False):
        """the k-mers of text -> (pos, occ, row[, sa]), uint32 arrays in lexicographic order: k-mer i is
        text[pos[i] : pos[i] + k], it occurs occ[i] times, at sa[row[i] : row[i] + occ[i]]: tc_kmers"""
        t = _u8(text)
        cap = max(self.kmer_count(t, k, min_occ, max_occ), 1)
        pos, occ, row = (np.empty(cap, np.uint32) for _ in range(3))
        sa = np.empty(len(t) + 1, np.uint32) if with_sa else None
        nk = C.c_uint64(cap)
        self._check(self._lib.tc_kmers(self._h, _ptr(t) if len(t) else None, len(t), k, min_occ, max_occ,
                                       _ptr(sa) if with_sa else None, _ptr(pos), _ptr(occ), _ptr(row), C.byref(nk)))
        m = int(nk.value)
        out = (pos[:m].copy(), occ[:m].copy(), row[:m].copy())
        return out + (sa,) if with_sa else out

    def _kmers_retry(self, call, device, cap):
        """the capacity protocol of the two device lists: call(pos, occ, row, nk) -> rc; cap None: sizes first"""
        import torch
        torch.cuda.synchronize()
        if cap is None:
            nk = C.c_uint64(0)
            self._check(call(None, None, None, C.byref(nk)))
            cap = int(nk.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=device) for _ in range(3)]
            torch.cuda.synchronize()
            nk = C.c_uint64(cap)
            rc = call(*(C.c_void_p(o.data_ptr()) for o in out), C.byref(nk))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nk.value), 1)
        self._check(rc)
        return tuple(o[:int(nk.value)] for o in out)

    def kmers_dev(self, d_text, k, min_occ=1, max_occ=0, with_sa=False, cap=None):
        """text resident in HBM -> (pos, occ, row[, sa]), int32 tensors on the device: tc_kmers_dev.  cap: the k-mer
        slots to try first (None: the sizes-only form runs first)"""
        import torch
        n = d_text.numel()
        pt = C.c_void_p(d_text.data_ptr()) if n else None
        d_sa = torch.empty(n + 1, dtype=torch.int32, device=d_text.device) if with_sa else None
        psa = C.c_void_p(d_sa.data_ptr()) if with_sa else None
        res = self._kmers_retry(lambda p, o, r, nk: self._lib.tc_kmers_dev(self._h, pt, n, k, min_occ, max_occ, psa, p, o, r, nk),
                                d_text.device, cap)
        return res + (d_sa,) if with_sa else res

    def kmers_esa_dev(self, d_sa, d_lcp, k, min_occ=1, max_occ=0, cap=None):
        """a suffix array and its LCP array resident in HBM (suffix_array_dev, lcp_array_dev: the sort is paid once for
        any number of k) -> (pos, occ, row), int32 tensors on the device: tc_kmers_esa_dev"""
        N = d_lcp.numel()
        if d_sa.numel() != N or d_sa.element_size() != 4 or d_lcp.element_size() != 4:
            raise ValueError("d_sa and d_lcp must hold the same number of 32-bit entries")
        psa, pl = C.c_void_p(d_sa.data_ptr()), C.c_void_p(d_lcp.data_ptr())
        return self._kmers_retry(lambda p, o, r, nk: self._lib.tc_kmers_esa_dev(self._h, psa, pl, N, k, min_occ, max_occ, p, o, r, nk),
                                 d_lcp.device, cap)

    def kmer_spectrum(self, text, k, bins=256):
        """-> (hist uint64[bins], distinct, total): hist[i] = the distinct k-mers that occur i + 1 times, the last bin
        those that occur at least `bins` times; total = max(0, n - k + 1): tc_kmer_spectrum"""
        t = _u8(text)
        hist = np.empty(max(bins, 1), np.uint64)
        distinct, total = C.c_uint64(), C.c_uint64()
        self._check(self._lib.tc_kmer_spectrum(self._h, _ptr(t) if len(t) else None, len(t), k, bins, _ptr(hist),
                                               C.byref(distinct), C.byref(total)))
        return hist, int(distinct.value), int(total.value)

    def kmer_spectrum_esa_dev(self, d_sa, d_lcp, k, bins=256):
        """the same from an enhanced suffix array resident in HBM -> (hist, an int64 tensor of `bins` entries on the
        device, distinct, total): tc_kmer_spectrum_esa_dev"""
        import torch
        N = d_lcp.numel()
        if d_sa.numel() != N or d_sa.element_size() != 4 or d_lcp.element_size() != 4:
            raise ValueError("d_sa and d_lcp must hold the same number of 32-bit entries")
        d_hist = torch.empty(max(bins, 1), dtype=torch.int64, device=d_lcp.device)
        distinct, total = C.c_uint64(), C.c_uint64()
        torch.cuda.synchronize()
        self._check(self._lib.tc_kmer_spectrum_esa_dev(self._h, C.c_void_p(d_sa.data_ptr()), C.c_void_p(d_lcp.data_ptr()), N, k,
                                                       bins, C.c_void_p(d_hist.data_ptr()), C.byref(distinct), C.byref(total)))
        return d_hist, int(distinct.value), int(total.value)

    def kmer_profile(self, text, kmax, unique=True):
        """-> (distinct, unique), uint64 arrays of kmax entries: the number of distinct k-mers and of k-mers that occur
        once, for every k = 1 .. kmax (unique=False: the second is None): tc_kmer_profile"""
        t = _u8(text)
        d = np.empty(max(kmax, 1), np.uint64)
        u = np.empty(max(kmax, 1), np.uint64) if unique else None
        self._check(self._lib.tc_kmer_profile(self._h, _ptr(t) if len(t) else None, len(t), kmax, _ptr(d), _ptr(u) if unique else None))
        return d[:kmax], (u[:kmax] if unique else None)

    def kmer_profile_esa_dev(self, d_lcp, kmax, unique=True):
        """the same from an LCP array resident in HBM (the suffix array is not read): tc_kmer_profile_esa_dev; the two
        results are host arrays"""
        import torch
        if d_lcp.element_size() != 4:
            raise ValueError("d_lcp must hold 32-bit entries")
        d = np.empty(max(kmax, 1), np.uint64)
        u = np.empty(max(kmax, 1), np.uint64) if unique else None
        torch.cuda.synchronize()
        self._check(self._lib.tc_kmer_profile_esa_dev(self._h, C.c_void_p(d_lcp.data_ptr()), d_lcp.numel(), kmax, _ptr(d),
                                                      _ptr(u) if unique else None))
        return d[:kmax], (u[:kmax] if unique else None)

    # ------------------------------------- one text against another: matching statistics, MEMs, LCS
    def text_match_stats(self, query, target, pos=True, occ=True):
        """-> (ms_len, ms_pos, ms_occ), uint32 arrays of len(query) entries, 0-based: ms_len[i] = the longest prefix of
        query[i:] that occurs in target, ms_pos[i] = where the smallest suffix of target with that prefix starts,
        ms_occ[i] = its occurrences in target (pos / occ False: None in their place): tc_text_match_stats"""
        q, t = _u8(query), _u8(target)
        a = len(q)
        ms_len = np.empty(a, np.uint32)
        ms_pos = np.empty(a, np.uint32) if pos else None
        ms_occ = np.empty(a, np.uint32) if occ else None
        if a == 0:
            return ms_len, ms_pos, ms_occ
        self._check(self._lib.tc_text_match_stats(self._h, _ptr(q) if a else None, a, _ptr(t) if len(t) else None, len(t),
                                                  _ptr(ms_len), _ptr(ms_pos), _ptr(ms_occ)))
        return ms_len, ms_pos, ms_occ

    def text_mem_count(self, query, target, min_len=1):
        """the number of maximal exact matches of query in target that are at least min_len long (the sizes-only form of
        tc_text_mems)"""
        q, t = _u8(query), _u8(target)
        nmem = C.c_uint64(0)
        self._check(self._lib.tc_text_mems(self._h, _ptr(q) if len(q) else None, len(q), _ptr(t) if len(t) else None, len(t),
                                           min_len, None, None, None, C.byref(nmem)))
        return int(nmem.value)

    def text_mems(self, query, target, min_len=1):
        """the maximal exact matches of query in target -> (start, pos, len), uint32 arrays in increasing start:
        query[start : start + len] == target[pos : pos + len]: tc_text_mems"""
        q, t = _u8(query), _u8(target)
        cap = max(self.text_mem_count(q, t, min_len), 1)
        start, pos, ln = (np.empty(cap, np.uint32) for _ in range(3))
        nmem = C.c_uint64(cap)
        self._check(self._lib.tc_text_mems(self._h, _ptr(q) if len(q) else None, len(q), _ptr(t) if len(t) else None, len(t),
                                           min_len, _ptr(start), _ptr(pos), _ptr(ln), C.byref(nmem)))
        k = int(nmem.value)
        return start[:k].copy(), pos[:k].copy(), ln[:k].copy()

    def text_lcs(self, query, target):
        """-> (len, qpos, tpos, sum): query[qpos : qpos + len] == target[tpos : tpos + len] is a longest common substring
        (the first in query; (0, 0, 0) when no byte is common), sum = the sum of ms_len: tc_text_lcs"""
        q, t = _u8(query), _u8(target)
        ln, qpos, tpos, tot = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.tc_text_lcs(self._h, _ptr(q) if len(q) else None, len(q), _ptr(t) if len(t) else None, len(t),
                                          C.byref(ln), C.byref(qpos), C.byref(tpos), C.byref(tot)))
        return int(ln.value), int(qpos.value), int(tpos.value), int(tot.value)

    @staticmethod
    def _dev_ptr(d):
        return C.c_void_p(d.data_ptr()) if d.numel() else None

    def text_match_stats_dev(self, d_query, d_target, pos=True, occ=True):
        """the two texts resident in HBM (torch uint8 tensors on this context's device; they may be one tensor) ->
        (ms_len, ms_pos, ms_occ), int32 tensors of a entries on the device (None where not asked for):
        tc_text_match_stats_dev"""
        import torch
        a = d_query.numel()
        out = [torch.empty(a, dtype=torch.int32, device=d_query.device) if want else None for want in (True, pos, occ)]
        if a == 0:
            return tuple(out)
        torch.cuda.synchronize()
        self._check(self._lib.tc_text_match_stats_dev(self._h, self._dev_ptr(d_query), a, self._dev_ptr(d_target),
                                                      d_target.numel(), *(C.c_void_p(o.data_ptr()) if o is not None else None for o in out)))
        return tuple(out)

    def _mems_retry(self, call, device, cap):
        """the capacity protocol of the two device MEM lists: call(start, pos, len, nmem) -> rc; cap None: sizes first"""
        import torch
        torch.cuda.synchronize()
        if cap is None:
            nmem = C.c_uint64(0)
            self._check(call(None, None, None, C.byref(nmem)))
            cap = int(nmem.value)
        cap = max(int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device=device) for _ in range(3)]
            torch.cuda.synchronize()
            nmem = C.c_uint64(cap)
            rc = call(*(C.c_void_p(o.data_ptr()) for o in out), C.byref(nmem))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nmem.value), 1)
        self._check(rc)
        return tuple(o[:int(nmem.value)] for o in out)

    def text_mems_dev(self, d_query, d_target, min_len=1, cap=None):
        """the two texts resident in HBM -> (start, pos, len), int32 tensors on the device: tc_text_mems_dev.  cap: the
        MEM slots to try first (None: the sizes-only form runs first)"""
        pq, pt = self._dev_ptr(d_query), self._dev_ptr(d_target)
        a, b = d_query.numel(), d_target.numel()
        return self._mems_retry(lambda s, p, l, nm: self._lib.tc_text_mems_dev(self._h, pq, a, pt, b, min_len, s, p, l, nm),
                                d_query.device, cap)

    def mems_from_stats_dev(self, d_ms_len, d_ms_pos, min_len=1, cap=None):
        """matching statistics resident in HBM (two 32-bit tensors of one length: text_match_stats_dev's, kept for any
        number of min_len) -> (start, pos, len), int32 tensors on the device: tc_mems_from_stats_dev"""
        a = d_ms_len.numel()
        if d_ms_pos.numel() != a or d_ms_len.element_size() != 4 or d_ms_pos.element_size() != 4:
            raise ValueError("d_ms_len and d_ms_pos must hold the same number of 32-bit entries")
        pl, pp = self._dev_ptr(d_ms_len), self._dev_ptr(d_ms_pos)
        return self._mems_retry(lambda s, p, l, nm: self._lib.tc_mems_from_stats_dev(self._h, pl, pp, a, min_len, s, p, l, nm),
                                d_ms_len.device, cap)

    def text_lcs_dev(self, d_query, d_target):
        """the two texts resident in HBM -> (len, qpos, tpos, sum), host integers: tc_text_lcs_dev"""
        import torch
        ln, qpos, tpos, tot = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        torch.cuda.synchronize()
        self._check(self._lib.tc_text_lcs_dev(self._h, self._dev_ptr(d_query), d_query.numel(), self._dev_ptr(d_target),
                                              d_target.numel(), C.byref(ln), C.byref(qpos), C.byref(tpos), C.byref(tot)))
        return int(ln.value), int(qpos.value), int(tpos.value), int(tot.value)

    def bwt_decode(self, L, primary):
        L = _u8(L)
        N = len(L)
        if N == 0:
            return b""
        out = np.empty(max(N - 1, 1), np.uint8)
        self._check(self._lib.tc_bwt_decode(self._h, _ptr(L), N, primary, _ptr(out)))
        return out[:N - 1].tobytes()

    def bwt_decode_sym(self, sym):
        sym = np.ascontiguousarray(sym, dtype=np.int16)
        N = len(sym)
        if N == 0:
            return b""
        out = np.empty(N, np.uint8)
        n_out = C.c_uint64()
        self._check(self._lib.tc_bwt_decode_sym(self._h, _ptr(sym), N, _ptr(out), C.byref(n_out)))
        return out[:n_out.value].tobytes()

    # ---------------------------------------------------------------- MTF
    def mtf_encode(self, L, primary):
        """(L, primary|None) -> (idx uint16[N], final_list int16[sigma])."""
        L = _u8(L)
        N = len(L)
        if N == 0:
            return np.empty(0, np.uint16), np.empty(0, np.int16)
        idx = np.empty(N, np.uint16)
        fl = np.empty(_lib.TC_MAX_SIGMA, np.int16)
        sig = C.c_uint32()
        self._check(self._lib.tc_mtf_encode(self._h, _ptr(L), N, -1 if primary is None else primary,
                                            _ptr(idx), _ptr(fl), C.byref(sig)))
        return idx, fl[:sig.value].copy()

    def mtf_encode_sym(self, sym):
        sym = np.ascontiguousarray(sym, dtype=np.int16)
        N = len(sym)
        if N == 0:
            return np.empty(0, np.uint16), np.empty(0, np.int16)
        idx = np.empty(N, np.uint16)
        fl = np.empty(_lib.TC_MAX_SIGMA, np.int16)
        sig = C.c_uint32()
        self._check(self._lib.tc_mtf_encode_sym(self._h, _ptr(sym), N, _ptr(idx), _ptr(fl),
                                                C.byref(sig)))
        return idx, fl[:sig.value].copy()

    def mtf_decode(self, idx, flist):
        idx = np.ascontiguousarray(idx, dtype=np.uint16)
        fl = np.ascontiguousarray(flist, dtype=np.int16)
        if len(idx) == 0 or len(fl) == 0:
            return np.empty(0, np.int16)
        out = np.empty(len(idx), np.int16)
        self._check(self._lib.tc_mtf_decode(self._h, _ptr(idx), len(idx), _ptr(fl), len(fl), _ptr(out)))
        return out

    # ---------------------------------------------------------------- RLE
    def _rle_call(self, fn, args_before, N, sym_dtype, cap=None):
        cap = (2 * N + 2) if cap is None else cap
        counts = np.empty(max(cap, 1), np.uint32)
        syms = np.empty(max(cap, 1), sym_dtype)
        nr = C.c_uint64(cap)
        self._check(fn(self._h, *args_before, _ptr(counts), _ptr(syms), C.byref(nr)))
        return counts[:nr.value].copy(), syms[:nr.value].copy()

    def rle_encode(self, L, primary, cap=None):
        L = _u8(L)
        if len(L) == 0:
            return np.empty(0, np.uint32), np.empty(0, np.int16)
        return self._rle_call(self._lib.tc_rle_encode,
                              (_ptr(L), len(L), -1 if primary is None else primary), len(L),
                              np.int16, cap)

    def rle_encode_sym(self, sym, cap=None):
        sym = np.ascontiguousarray(sym, dtype=np.int16)
        if len(sym) == 0:
            return np.empty(0, np.uint32), np.empty(0, np.int16)
        return self._rle_call(self._lib.tc_rle_encode_sym, (_ptr(sym), len(sym)), len(sym), np.int16,
                              cap)

    def rle_encode_u16(self, vals, cap=None):
        vals = np.ascontiguousarray(vals, dtype=np.uint16)
        if len(vals) == 0:
            return np.empty(0, np.uint32), np.empty(0, np.uint16)
        return self._rle_call(self._lib.tc_rle_encode_u16, (_ptr(vals), len(vals)), len(vals),
                              np.uint16, cap)

    def _rle_decode(self, fn, counts, syms, dtype):
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        syms = np.ascontiguousarray(syms, dtype=dtype)
        if len(counts) == 0:
            return np.empty(0, dtype)
        cap = int(counts.astype(np.uint64).sum()) + len(counts) + 1
        out = np.empty(cap, dtype)
        N = C.c_uint64(cap)
        self._check(fn(self._h, _ptr(counts), _ptr(syms), len(counts), _ptr(out), C.byref(N)))
        return out[:N.value].copy()

    def rle_decode(self, counts, syms):
        return self._rle_decode(self._lib.tc_rle_decode, counts, syms, np.int16)

    def rle_decode_u16(self, counts, vals):
        return self._rle_decode(self._lib.tc_rle_decode_u16, counts, vals, np.uint16)

    # ------------------------------------------------------------- fused
    def encode(self, text, cap=None):
        """Fused BWT->MTF->RLE.  -> dict(n, primary, sigma, final_list, run_count, run_value)."""
        t = _u8(text)
        n = len(t)
        cap = (n + 2) if cap is None else cap
        rc_ = np.empty(max(cap, 1), np.uint32)
        rv_ = np.empty(max(cap, 1), np.uint16)
        b = Block()
        b.nruns = cap
        b.run_count = rc_.ctypes.data
        b.run_value = rv_.ctypes.data
        self._check(self._lib.tc_encode(self._h, _ptr(t) if n else None, n, C.byref(b)))
        k = int(b.nruns)
        return dict(n=int(b.n), primary=int(b.primary) if n else None, sigma=int(b.sigma),
                    final_list=np.array(b.final_list[:b.sigma], dtype=np.int16),
                    run_count=rc_[:k].copy(), run_value=rv_[:k].copy())

    def decode(self, blk):
        n = int(blk["n"])
        if n == 0:
            return b""
        rc_ = np.ascontiguousarray(blk["run_count"], dtype=np.uint32)
        rv_ = np.ascontiguousarray(blk["run_value"], dtype=np.uint16)
        b = Block()
        b.n = n
        b.primary = int(blk["primary"])
        b.sigma = int(blk["sigma"])
        for i, v in enumerate(blk["final_list"]):
            b.final_list[i] = int(v)
        b.nruns = len(rc_)
        b.run_count = rc_.ctypes.data
        b.run_value = rv_.ctypes.data
        out = np.empty(n, np.uint8)
        self._check(self._lib.tc_decode(self._h, C.byref(b), _ptr(out)))
        return out.tobytes()

    # --------------------------------------------------------- container
    def encode_container(self, text, cap=None, coding=None):
        """text -> one self-describing byte string (header + packed runs); see textcomp.h.
        coding: "packed" / "huffman" for this call (the context's setting is restored afterwards)."""
        t = _u8(text)
        n = len(t)
        cap = int(self._lib.tc_container_bound(n + 2, 257 if n else 0)) if cap is None else int(cap)
        out = np.empty(max(cap, 1), np.uint8)
        used = C.c_uint64(cap)
        with self._with_coding(coding):
            self._check(self._lib.tc_encode_container(self._h, _ptr(t), n, _ptr(out), C.byref(used)))
        return out[:used.value].tobytes()

    def encode_container_dev(self, d_text_ptr, n, d_out_ptr, cap):
        """device text -> device container (tc_encode_container_dev: for sigma <= 6 the RLE stage writes the
        container's nibble stream itself).  Returns the bytes used."""
        used = C.c_uint64(int(cap))
        self._check(self._lib.tc_encode_container_dev(self._h, C.c_void_p(d_text_ptr), int(n), C.c_void_p(d_out_ptr),
                                                      C.byref(used)))
        return int(used.value)

    def decode_container(self, blob):
        b = np.frombuffer(bytes(blob), np.uint8)
        n, nruns = C.c_uint64(), C.c_uint64()
        self._check(self._lib.tc_container_info(self._h, _ptr(b), len(b), C.byref(n), C.byref(nruns)))
        out = np.empty(max(n.value, 1), np.uint8)
        got = C.c_uint64()
        self._check(self._lib.tc_decode_container(self._h, _ptr(b), len(b), _ptr(out), C.byref(got)))
        return out[:got.value].tobytes()

    # ------------------------------------------------------ chunked stream
    def encode_stream(self, text, block_bytes=0, cap=None, coding=None):
        """coding: "packed" / "huffman" for this call (the context's setting is restored afterwards).
        text of any length -> containers of independent records of block_bytes, back to back
        (copies overlap the encode); see textcomp.h.  Without `cap` the output buffer starts at
        2 bytes per input byte and falls back to tc_stream_bound when that is too small."""
        t = _u8(text)
        n = len(t)
        bound = int(self._lib.tc_stream_bound(n, block_bytes))
        caps = [int(cap)] if cap is not None else sorted({min(bound, 2 * n + 4096 * (1 + n // max(int(block_bytes) or (1 << 30), 1))), bound})
        for i, c in enumerate(caps):
            out = np.empty(max(c, 1), np.uint8)
            used = C.c_uint64(c)
            with self._with_coding(coding):
                rc = self._lib.tc_encode_stream(self._h, _ptr(t), n, int(block_bytes), _ptr(out), C.byref(used))
            if rc == _lib.TC_ERR_CAPACITY and i + 1 < len(caps):
                continue
            self._check(rc)
            return out[:used.value].tobytes()

    def stream_info(self, blob):
        """(total text bytes, number of records) of a stream."""
        b = np.frombuffer(bytes(blob), np.uint8)
        n, nb = C.c_uint64(), C.c_uint64()
        self._check(self._lib.tc_stream_info(self._h, _ptr(b), len(b), C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def decode_stream(self, blob):
        b = np.frombuffer(bytes(blob), np.uint8)
        n, _ = self.stream_info(b)
        out = np.empty(max(n, 1), np.uint8)
        got = C.c_uint64(n)
        self._check(self._lib.tc_decode_stream(self._h, _ptr(b), len(b), _ptr(out), C.byref(got)))
        return out[:got.value].tobytes()

    # ----------------------------------------------------------- FM-index
    def fm_build(self, text, sa_rate=1, text_rate=0, lcp=False):
        """sa_rate > 1 (a power of two up to TC_FM_MAX_SA_RATE): keep every sa_rate-th suffix-array entry only
        (tc_fm_build_sampled); locate answers the same hits by walking the LF mapping.  text_rate > 0 (a power of two
        up to TC_FM_MAX_SA_RATE): also keep the row of every text_rate-th text position (tc_fm_build_self), so that
        extract can read text ranges back from the index.  lcp: also keep the LCP array and its min tree
        (tc_fm_build_lcp), so that match_stats and mems work"""
        return FMIndexHandle(self, text, sa_rate=sa_rate, text_rate=text_rate, lcp=lcp)

    def fm_build_dev(self, d_text, sa_rate=1, text_rate=0, lcp=False):
        """index of a text that already lies in HBM (a torch uint8 tensor on this context's device): tc_fm_build_dev /
        tc_fm_build_sampled_dev / tc_fm_build_self_dev / tc_fm_build_lcp_dev"""
        h = C.c_void_p()
        p = C.c_void_p(d_text.data_ptr()) if d_text.numel() else None
        if lcp:
            self._check(self.lib.tc_fm_build_lcp_dev(self.handle, p, d_text.numel(), int(sa_rate), int(text_rate), C.byref(h)))
        elif text_rate:
            self._check(self.lib.tc_fm_build_self_dev(self.handle, p, d_text.numel(), int(sa_rate), int(text_rate), C.byref(h)))
        elif sa_rate == 1:
            self._check(self.lib.tc_fm_build_dev(self.handle, p, d_text.numel(), C.byref(h)))
        else:
            self._check(self.lib.tc_fm_build_sampled_dev(self.handle, p, d_text.numel(), int(sa_rate), C.byref(h)))
        return FMIndexHandle(self, None, _handle=h, _n=d_text.numel())

    # ----------------------------------------------------------- the kept enhanced suffix array
    def esa_build(self, text):
        """the enhanced suffix array of text, kept on the device for any number of queries and analyses: tc_esa_build"""
        return ESAHandle(self, text)

    def esa_build_dev(self, d_text):
        """the same of a text that already lies in HBM (a torch uint8 tensor on this context's device; the handle keeps its
        own copy): tc_esa_build_dev"""
        import torch
        torch.cuda.synchronize()
        h = C.c_void_p()
        p = C.c_void_p(d_text.data_ptr()) if d_text.numel() else None
        self._check(self.lib.tc_esa_build_dev(self.handle, p, d_text.numel(), C.byref(h)))
        return ESAHandle(self, None, _handle=h)

    def esa_build_docs(self, text, docs):
        """the same of a collection: text is the concatenation of the documents, docs their boundaries doc_start[0 .. ndocs]
        (textcomp.concat_docs makes both); the handle also answers document frequency and listing: tc_esa_build_docs"""
        return ESAHandle(self, text, docs=docs)

    def esa_build_docs_dev(self, d_text, docs):
        """the same of a text that already lies in HBM (docs is a host array): tc_esa_build_docs_dev"""
        import torch
        torch.cuda.synchronize()
        ds = np.ascontiguousarray(docs, dtype=np.uint32).ravel()
        h = C.c_void_p()
        p = C.c_void_p(d_text.data_ptr()) if d_text.numel() else None
        self._check(self.lib.tc_esa_build_docs_dev(self.handle, p, d_text.numel(), _ptr(ds) if len(ds) else None, max(len(ds), 1) - 1,
                                                   C.byref(h)))
        return ESAHandle(self, None, _handle=h)


class FMIndexHandle:
    """`tc_fm`: the device-resident FM-index of one text."""

    def __init__(self, ctx, text, _handle=None, _n=0, sa_rate=1, text_rate=0, lcp=False):
        self._ctx = ctx
        if _handle is not None:      # an index that arrived from another GPU (textcomp.fmshard)
            self._h, self.n = _handle, _n
            return
        t = _u8(text)
        h = C.c_void_p()
        if lcp:
            ctx._check(ctx.lib.tc_fm_build_lcp(ctx.handle, _ptr(t) if len(t) else None, len(t), int(sa_rate), int(text_rate), C.byref(h)))
        elif text_rate:
            ctx._check(ctx.lib.tc_fm_build_self(ctx.handle, _ptr(t) if len(t) else None, len(t), int(sa_rate), int(text_rate), C.byref(h)))
        elif sa_rate == 1:
            ctx._check(ctx.lib.tc_fm_build(ctx.handle, _ptr(t) if len(t) else None, len(t), C.byref(h)))
        else:
            ctx._check(ctx.lib.tc_fm_build_sampled(ctx.handle, _ptr(t) if len(t) else None, len(t), int(sa_rate), C.byref(h)))
        self._h = h
        self.n = len(t)

    @property
    def sa_rate(self):
        """1: full suffix array; k > 1: every k-th entry kept; 0: no locate part (count-only import, empty index)"""
        return int(self._ctx.lib.tc_fm_sa_rate(self._h))

    @property
    def text_rate(self):
        """k >= 1: the row of every k-th text position is kept (extract works); 0: no text samples"""
        return int(self._ctx.lib.tc_fm_text_rate(self._h))

    @property
    def has_lcp(self):
        """True: the index holds the LCP part (built with lcp=True), match_stats and mems work"""
        return bool(self._ctx.lib.tc_fm_has_lcp(self._h))

    def device_bytes(self, part=0):
        """device bytes the index holds: part 0 = everything, 1 = the locate part alone, 2 = the extract part alone,
        3 = the LCP part alone"""
        return int(self._ctx.lib.tc_fm_device_bytes(self._h, int(part)))

    def extract(self, starts, lens):
        """text ranges read back from the index: starts are 1-based (what locate answers), -> list of bytes, one per
        query, equal to text[start - 1 : start - 1 + len]: tc_fm_extract"""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint64)
        if st.shape != ln.shape or st.ndim != 1:
            raise ValueError("starts and lens must be two sequences of one length")
        nq = len(st)
        if nq == 0:
            return []
        ctx = self._ctx
        offs = np.empty(nq + 1, np.uint64)
        cap = 1 << 16
        while True:
            out = np.empty(max(cap, 1), np.uint8)
            nb = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_extract(ctx.handle, self._h, _ptr(st), _ptr(ln), nq, _ptr(offs), _ptr(out), C.byref(nb))
            if rc == _lib.TC_ERR_CAPACITY and int(nb.value) > cap:
                cap = int(nb.value)
                continue
            ctx._check(rc)
            break
        blob = out[:int(nb.value)].tobytes()
        return [blob[int(offs[i]):int(offs[i + 1])] for i in range(nq)]

    def extract_dev(self, d_starts, d_lens, nq, cap=None):
        """queries resident on the device (two uint64/int64 tensors [nq], starts 1-based) -> (offs int64 tensor
        [nq + 1], bytes uint8 tensor [total]), both on the device: tc_fm_extract_dev"""
        import torch
        ctx = self._ctx
        dev = d_starts.device
        offs = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        if nq == 0:
            return offs, torch.zeros(0, dtype=torch.uint8, device=dev)
        cap = max(int(cap) if cap is not None else 128 * nq, 1)
        for _ in range(2):
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            nb = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_extract_dev(ctx.handle, self._h, C.c_void_p(d_starts.data_ptr()), C.c_void_p(d_lens.data_ptr()),
                                           nq, C.c_void_p(offs.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(nb))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nb.value), 1)
        ctx._check(rc)
        return offs, out[:int(nb.value)]

    def locate_dev(self, d_pats, d_offs, npat, cap=None):
        """patterns resident on the device (as count_dev) -> (hit_offs uint64-as-int64 tensor [npat + 1], hits tensor
        [total], 1-based positions in SA order), both on the device: tc_fm_locate_dev"""
        import torch
        ctx = self._ctx
        hoffs = torch.zeros(npat + 1, dtype=torch.int64, device=d_pats.device)
        if npat == 0:
            return hoffs, torch.zeros(0, dtype=torch.int64, device=d_pats.device)
        cap = max(int(cap) if cap is not None else 2 * npat, 1)
        for _ in range(2):
            hits = torch.empty(cap, dtype=torch.int64, device=d_pats.device)
            torch.cuda.synchronize()
            nh = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_locate_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                          npat, C.c_void_p(hoffs.data_ptr()), C.c_void_p(hits.data_ptr()), C.byref(nh))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nh.value), 1)
        ctx._check(rc)
        return hoffs, hits[:int(nh.value)]

    def export_dev(self, with_locate=False):
        """The index as one device byte string (torch uint8 tensor) -- what a broadcast moves."""
        import torch
        ctx = self._ctx
        nb = int(ctx.lib.tc_fm_export_bound(self._h, int(with_locate)))
        buf = torch.empty(nb, dtype=torch.uint8, device="cuda:%d" % ctx.device)
        torch.cuda.synchronize()
        used = C.c_uint64(nb)
        ctx._check(ctx.lib.tc_fm_export_dev(ctx.handle, self._h, int(with_locate), C.c_void_p(buf.data_ptr()), C.byref(used)))
        return buf[:used.value]

    @classmethod
    def import_dev(cls, ctx, buf, n=0):
        """Inverse of export_dev on this rank's device; `buf` may be released afterwards."""
        import torch
        torch.cuda.synchronize()
        h = C.c_void_p()
        ctx._check(ctx.lib.tc_fm_import_dev(ctx.handle, C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(h)))
        return cls(ctx, None, _handle=h, _n=n)

    def count_dev(self, d_pats, d_offs, npat):
        """patterns resident on the device (flat uint8 tensor, uint64/int64 offsets [npat + 1]) -> int64 tensor"""
        import torch
        ctx = self._ctx
        out = torch.zeros(max(npat, 1), dtype=torch.int64, device=d_pats.device)[:npat]
        torch.cuda.synchronize()
        if npat:
            ctx._check(ctx.lib.tc_fm_count_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()),
                                               C.c_void_p(d_offs.data_ptr()), npat, C.c_void_p(out.data_ptr())))
        return out

    def count_mm_dev(self, d_pats, d_offs, npat, k):
        """count_dev within Hamming distance k (0 .. TC_FM_MAX_MISMATCH; substitutions only) -> int64 tensor:
        tc_fm_count_mm_dev"""
        import torch
        ctx = self._ctx
        out = torch.zeros(max(npat, 1), dtype=torch.int64, device=d_pats.device)[:npat]
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_fm_count_mm_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                              npat, int(k), C.c_void_p(out.data_ptr())))
        return out

    def locate_mm_dev(self, d_pats, d_offs, npat, k, cap=None):
        """locate_dev within Hamming distance k -> (hit_offs int64 tensor [npat + 1], hits int64 tensor [total], 1-based
        positions in the kernel's enumeration order, mismatches uint8 tensor [total]), all on the device:
        tc_fm_locate_mm_dev"""
        import torch
        ctx = self._ctx
        dev = d_pats.device
        hoffs = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
        cap = max(int(cap) if cap is not None else 2 * npat, 1)
        for _ in range(2):
            hits = torch.empty(cap, dtype=torch.int64, device=dev)
            mm = torch.empty(cap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            nh = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_locate_mm_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                             npat, int(k), C.c_void_p(hoffs.data_ptr()), C.c_void_p(hits.data_ptr()),
                                             C.c_void_p(mm.data_ptr()), C.byref(nh))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nh.value), 1)
        ctx._check(rc)
        return hoffs, hits[:int(nh.value)], mm[:int(nh.value)]

    def close(self):
        if getattr(self, "_h", None):
            self._ctx.lib.tc_fm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _pack(pats):
        offs = np.zeros(len(pats) + 1, np.uint64)
        for i, p in enumerate(pats):
            offs[i + 1] = offs[i] + len(p)
        flat = np.frombuffer(b"".join(bytes(p) for p in pats) + b"\0", dtype=np.uint8).copy()
        return flat, offs

    def count(self, pats):
        """-> int64[npat]; 0 stands for Nothing."""
        if len(pats) == 0:
            return np.empty(0, np.int64)
        flat, offs = self._pack(pats)
        out = np.empty(len(pats), np.int64)
        ctx = self._ctx
        ctx._check(ctx.lib.tc_fm_count(ctx.handle, self._h, _ptr(flat), _ptr(offs), len(pats), _ptr(out)))
        return out

    def locate(self, pats):
        """-> list of uint64 arrays (1-based positions, SA order)."""
        if len(pats) == 0:
            return []
        flat, offs = self._pack(pats)
        ctx = self._ctx
        hoffs = np.empty(len(pats) + 1, np.uint64)
        cap = 1 << 16
        while True:
            hits = np.empty(cap, np.uint64)
            nh = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_locate(ctx.handle, self._h, _ptr(flat), _ptr(offs), len(pats),
                                      _ptr(hoffs), _ptr(hits), C.byref(nh))
            if rc == _lib.TC_ERR_CAPACITY:
                cap = int(nh.value)
                continue
            ctx._check(rc)
            break
        return [hits[int(hoffs[i]):int(hoffs[i + 1])].copy() for i in range(len(pats))]

    def count_mm(self, pats, k):
        """-> int64[npat]: the text positions within Hamming distance k (0 .. TC_FM_MAX_MISMATCH; substitutions only) of
        each pattern.  A pattern byte that does not occur in the text can only be a mismatch (unlike count, which stops
        at it): tc_fm_count_mm"""
        ctx = self._ctx
        flat, offs = self._pack(pats)
        out = np.empty(len(pats), np.int64)
        ctx._check(ctx.lib.tc_fm_count_mm(ctx.handle, self._h, _ptr(flat), _ptr(offs), len(pats), int(k), _ptr(out)))
        return out

    def locate_mm(self, pats, k):
        """-> list of (positions uint64 array, mismatches uint8 array) pairs, one per pattern: 1-based positions within
        Hamming distance k, each once, in the kernel's enumeration order (deterministic, not sorted): tc_fm_locate_mm"""
        ctx = self._ctx
        flat, offs = self._pack(pats)
        hoffs = np.zeros(len(pats) + 1, np.uint64)
        cap = 1 << 16
        while True:
            hits = np.empty(cap, np.uint64)
            mm = np.empty(cap, np.uint8)
            nh = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_locate_mm(ctx.handle, self._h, _ptr(flat), _ptr(offs), len(pats), int(k),
                                         _ptr(hoffs), _ptr(hits), _ptr(mm), C.byref(nh))
            if rc == _lib.TC_ERR_CAPACITY and int(nh.value) > cap:
                cap = int(nh.value)
                continue
            ctx._check(rc)
            break
        return [(hits[int(hoffs[i]):int(hoffs[i + 1])].copy(), mm[int(hoffs[i]):int(hoffs[i + 1])].copy())
                for i in range(len(pats))]

    def factorize(self, pats):
        """the greedy right-to-left longest-match parse of each pattern against the text -> (fac_offs uint64 [npat + 1],
        fac_pos uint64 [total], fac_len uint32 [total]): pattern i's factors are [fac_offs[i], fac_offs[i + 1]), in
        pattern order; a match is (1-based position, length >= 1), a literal (byte value, 0): tc_fm_factorize"""
        ctx = self._ctx
        npat = len(pats)
        foffs = np.zeros(npat + 1, np.uint64)
        if npat == 0:
            return foffs, np.empty(0, np.uint64), np.empty(0, np.uint32)
        flat, offs = self._pack(pats)
        cap = 1 << 16
        while True:
            fpos = np.empty(cap, np.uint64)
            flen = np.empty(cap, np.uint32)
            nf = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_factorize(ctx.handle, self._h, _ptr(flat), _ptr(offs), npat, _ptr(foffs), _ptr(fpos), _ptr(flen),
                                         C.byref(nf))
            if rc == _lib.TC_ERR_CAPACITY and int(nf.value) > cap:
                cap = int(nf.value)
                continue
            ctx._check(rc)
            break
        return foffs, fpos[:int(nf.value)].copy(), flen[:int(nf.value)].copy()

    def factor_counts(self, pats):
        """-> uint64[npat]: the number of factors of each pattern (the sizes-only form of tc_fm_factorize)"""
        ctx = self._ctx
        npat = len(pats)
        if npat == 0:
            return np.empty(0, np.uint64)
        flat, offs = self._pack(pats)
        foffs = np.zeros(npat + 1, np.uint64)
        nf = C.c_uint64(0)
        ctx._check(ctx.lib.tc_fm_factorize(ctx.handle, self._h, _ptr(flat), _ptr(offs), npat, _ptr(foffs), None, None, C.byref(nf)))
        return np.diff(foffs)

    def unfactorize(self, fac_offs, fac_pos, fac_len):
        """the inverse of factorize on an index with text samples (text_rate > 0) -> list of bytes, one per pattern:
        tc_fm_unfactorize"""
        fo = np.ascontiguousarray(fac_offs, dtype=np.uint64)
        fp = np.ascontiguousarray(fac_pos, dtype=np.uint64)
        fl = np.ascontiguousarray(fac_len, dtype=np.uint32)
        if fo.ndim != 1 or len(fo) == 0 or fp.shape != fl.shape or fp.ndim != 1:
            raise ValueError("fac_offs [npat + 1], and fac_pos and fac_len of one length")
        npat = len(fo) - 1
        if npat == 0:
            return []
        if int(fo[-1]) > len(fp):
            raise ValueError("fac_offs names %d factors, %d given" % (int(fo[-1]), len(fp)))
        ctx = self._ctx
        offs = np.empty(npat + 1, np.uint64)
        cap = 1 << 16
        while True:
            out = np.empty(max(cap, 1), np.uint8)
            nb = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_unfactorize(ctx.handle, self._h, _ptr(fo), _ptr(fp) if len(fp) else None,
                                           _ptr(fl) if len(fl) else None, npat, _ptr(offs), _ptr(out), C.byref(nb))
            if rc == _lib.TC_ERR_CAPACITY and int(nb.value) > cap:
                cap = int(nb.value)
                continue
            ctx._check(rc)
            break
        blob = out[:int(nb.value)].tobytes()
        return [blob[int(offs[i]):int(offs[i + 1])] for i in range(npat)]

    def factorize_dev(self, d_pats, d_offs, npat, cap=None):
        """patterns resident on the device (as count_dev) -> (fac_offs int64 tensor [npat + 1], fac_pos int64 tensor
        [total], fac_len int32 tensor [total]), all on the device: tc_fm_factorize_dev"""
        import torch
        ctx = self._ctx
        dev = d_pats.device
        foffs = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
        if npat == 0:
            return foffs, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
        cap = max(int(cap) if cap is not None else 4 * npat, 1)
        for _ in range(2):
            fpos = torch.empty(cap, dtype=torch.int64, device=dev)
            flen = torch.empty(cap, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            nf = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_factorize_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                             npat, C.c_void_p(foffs.data_ptr()), C.c_void_p(fpos.data_ptr()),
                                             C.c_void_p(flen.data_ptr()), C.byref(nf))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nf.value), 1)
        ctx._check(rc)
        return foffs, fpos[:int(nf.value)], flen[:int(nf.value)]

    def unfactorize_dev(self, d_fac_offs, d_fac_pos, d_fac_len, npat, cap=None):
        """a factor list resident on the device (what factorize_dev returns) -> (offs int64 tensor [npat + 1], bytes uint8
        tensor [total]), both on the device: tc_fm_unfactorize_dev"""
        import torch
        ctx = self._ctx
        dev = d_fac_offs.device
        offs = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
        if npat == 0:
            return offs, torch.zeros(0, dtype=torch.uint8, device=dev)
        cap = max(int(cap) if cap is not None else 128 * npat, 1)
        for _ in range(2):
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            nb = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_unfactorize_dev(ctx.handle, self._h, C.c_void_p(d_fac_offs.data_ptr()),
                                               C.c_void_p(d_fac_pos.data_ptr()), C.c_void_p(d_fac_len.data_ptr()), npat,
                                               C.c_void_p(offs.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(nb))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nb.value), 1)
        ctx._check(rc)
        return offs, out[:int(nb.value)]

    def match_stats(self, pats, pos=True, occ=True):
        """matching statistics of each pattern on an index with the LCP part -> (ms_len uint32, ms_pos uint64 or None,
        ms_occ uint32 or None), each [total pattern bytes]: entry offs[j] + i is, for position i of pattern j, the length
        of the longest match that starts there, the 1-based text position of its occurrence in the first suffix-array
        row, and the number of its occurrences (0, 0, 0: the byte does not occur): tc_fm_match_stats"""
        ctx = self._ctx
        flat, offs = self._pack(pats)
        total = int(offs[-1])
        ms_len = np.zeros(total, np.uint32)
        ms_pos = np.zeros(total, np.uint64) if pos else None
        ms_occ = np.zeros(total, np.uint32) if occ else None
        if len(pats):
            ctx._check(ctx.lib.tc_fm_match_stats(ctx.handle, self._h, _ptr(flat), _ptr(offs), len(pats), _ptr(ms_len),
                                                 _ptr(ms_pos) if pos else None, _ptr(ms_occ) if occ else None))
        return ms_len, ms_pos, ms_occ

    def match_stats_dev(self, d_pats, d_offs, npat, total, pos=True, occ=True):
        """patterns resident on the device (as count_dev; total = offs[npat], the pattern bytes) -> (ms_len int32 tensor,
        ms_pos int64 tensor or None, ms_occ int32 tensor or None), each [total], on the device: tc_fm_match_stats_dev"""
        import torch
        ctx = self._ctx
        dev = d_pats.device
        ms_len = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)[:total]
        ms_pos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)[:total] if pos else None
        ms_occ = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)[:total] if occ else None
        torch.cuda.synchronize()
        if npat:
            ctx._check(ctx.lib.tc_fm_match_stats_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                                     npat, C.c_void_p(ms_len.data_ptr()),
                                                     C.c_void_p(ms_pos.data_ptr()) if pos else None,
                                                     C.c_void_p(ms_occ.data_ptr()) if occ else None))
        return ms_len, ms_pos, ms_occ

    def mems(self, pats, min_len=1):
        """the maximal exact matches of at least min_len bytes of each pattern on an index with the LCP part ->
        (mem_offs uint64 [npat + 1], mem_start uint64 [total], mem_pos uint64 [total], mem_len uint32 [total]): pattern
        j's MEMs are [mem_offs[j], mem_offs[j + 1]), in increasing start (0-based in the pattern); mem_pos is the 1-based
        text position of the occurrence in the first suffix-array row: tc_fm_mems"""
        ctx = self._ctx
        npat = len(pats)
        moffs = np.zeros(npat + 1, np.uint64)
        if npat == 0:
            return moffs, np.empty(0, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32)
        flat, offs = self._pack(pats)
        cap = 1 << 16
        while True:
            mstart, mpos, mlen = np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint32)
            nm = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_mems(ctx.handle, self._h, _ptr(flat), _ptr(offs), npat, int(min_len), _ptr(moffs), _ptr(mstart),
                                    _ptr(mpos), _ptr(mlen), C.byref(nm))
            if rc == _lib.TC_ERR_CAPACITY and int(nm.value) > cap:
                cap = int(nm.value)
                continue
            ctx._check(rc)
            break
        k = int(nm.value)
        return moffs, mstart[:k].copy(), mpos[:k].copy(), mlen[:k].copy()

    def mems_dev(self, d_pats, d_offs, npat, min_len=1, cap=None):
        """patterns resident on the device (as count_dev) -> (mem_offs int64 tensor [npat + 1], mem_start int64 tensor
        [total], mem_pos int64 tensor [total], mem_len int32 tensor [total]), all on the device: tc_fm_mems_dev"""
        import torch
        ctx = self._ctx
        dev = d_pats.device
        moffs = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
        if npat == 0:
            z = torch.zeros(0, dtype=torch.int64, device=dev)
            return moffs, z, z.clone(), torch.zeros(0, dtype=torch.int32, device=dev)
        cap = max(int(cap) if cap is not None else 4 * npat, 1)
        for _ in range(2):
            mstart = torch.empty(cap, dtype=torch.int64, device=dev)
            mpos = torch.empty(cap, dtype=torch.int64, device=dev)
            mlen = torch.empty(cap, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            nm = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_mems_dev(ctx.handle, self._h, C.c_void_p(d_pats.data_ptr()), C.c_void_p(d_offs.data_ptr()), npat,
                                        int(min_len), C.c_void_p(moffs.data_ptr()), C.c_void_p(mstart.data_ptr()),
                                        C.c_void_p(mpos.data_ptr()), C.c_void_p(mlen.data_ptr()), C.byref(nm))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nm.value), 1)
        ctx._check(rc)
        k = int(nm.value)
        return moffs, mstart[:k], mpos[:k], mlen[:k]

    def info(self):
        ctx = self._ctx
        N, sig, prim = C.c_uint64(), C.c_uint32(), C.c_uint64()
        cs = np.empty(_lib.TC_MAX_SIGMA, np.int16)
        cv = np.empty(_lib.TC_MAX_SIGMA, np.uint64)
        rc = ctx.lib.tc_fm_info(self._h, C.byref(N), C.byref(sig), _ptr(cs), _ptr(cv), C.byref(prim))
        if rc != 0:
            raise TcError(rc, "tc_fm_info")
        return dict(N=int(N.value), sigma=int(sig.value), c_sym=cs[:sig.value].copy(),
                    c_val=cv[:sig.value].copy(), primary=int(prim.value))


class ESAHandle:
    """`tc_esa`: the device-resident enhanced suffix array of one text -- the text, sa, isa, lcp and two min trees -- built
    once.  Queries may come from any Context on the handle's device (ctx=...); by default from the one that built it."""

    WHAT = {"text": _lib.TC_ESA_TEXT, "sa": _lib.TC_ESA_SA, "isa": _lib.TC_ESA_ISA, "lcp": _lib.TC_ESA_LCP,
            "da": _lib.TC_ESA_DA, "pv": _lib.TC_ESA_PV, "doc_start": _lib.TC_ESA_DOC_START}

    def __init__(self, ctx, text, _handle=None, docs=None):
        self._ctx = ctx
        if _handle is None:
            t = _u8(text)
            _handle = C.c_void_p()
            if docs is None:
                ctx._check(ctx.lib.tc_esa_build(ctx.handle, _ptr(t) if len(t) else None, len(t), C.byref(_handle)))
            else:
                ds = np.ascontiguousarray(docs, dtype=np.uint32).ravel()
                ctx._check(ctx.lib.tc_esa_build_docs(ctx.handle, _ptr(t) if len(t) else None, len(t), _ptr(ds) if len(ds) else None,
                                                     max(len(ds), 1) - 1, C.byref(_handle)))
        self._h = _handle
        self.n = int(ctx.lib.tc_esa_n(self._h))
        self.ndocs = int(ctx.lib.tc_esa_ndocs(self._h))     # 0: a plain handle

    def close(self):
        if getattr(self, "_h", None):
            self._ctx.lib.tc_esa_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device_bytes(self, part=0):
        """device bytes the handle holds: part 0 = everything, 1 = the text, 2 = sa, 3 = isa, 4 = lcp and its min tree,
        5 = the min tree of sa, 6 = da and doc_start, 7 = pv and its min tree (6 and 7: 0 on a plain handle)"""
        return int(self._ctx.lib.tc_esa_device_bytes(self._h, int(part)))

    def _what(self, what):
        w = self.WHAT.get(what, what)
        if w not in self.WHAT.values():
            raise ValueError("what is 'text', 'sa', 'isa', 'lcp', 'da', 'pv' or 'doc_start', not %r" % (what,))
        return w

    def _range(self, w, first, count):
        have = self.n if w == _lib.TC_ESA_TEXT else self.ndocs + 1 if w == _lib.TC_ESA_DOC_START else self.n + 1
        return int(first), int(have - first if count is None else count)

    def read(self, what, first=0, count=None, ctx=None):
        """entries [first, first + count) of 'text' (uint8) or 'sa', 'isa', 'lcp' and, on a handle with documents, 'da', 'pv',
        'doc_start' (uint32) -> numpy array: tc_esa_read"""
        ctx = ctx or self._ctx
        w = self._what(what)
        first, count = self._range(w, first, count)
        out = np.empty(max(count, 0), np.uint8 if w == _lib.TC_ESA_TEXT else np.uint32)
        ctx._check(ctx.lib.tc_esa_read(ctx.handle, self._h, w, first, count & (2 ** 64 - 1), _ptr(out) if len(out) else None, 0))
        return out

    def read_dev(self, what, first=0, count=None, ctx=None):
        """the same to a fresh tensor on the device (uint8, or int32 holding the 32-bit entries)"""
        import torch
        ctx = ctx or self._ctx
        w = self._what(what)
        first, count = self._range(w, first, count)
        out = torch.empty(max(count, 0), dtype=torch.uint8 if w == _lib.TC_ESA_TEXT else torch.int32, device="cuda:%d" % ctx.device)
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_read(ctx.handle, self._h, w, first, count & (2 ** 64 - 1),
                                       C.c_void_p(out.data_ptr()) if out.numel() else None, 1))
        return out

    @staticmethod
    def _u32s(*arrays):
        out = [np.ascontiguousarray(a, dtype=np.uint32).ravel() for a in arrays]
        if any(len(a) != len(out[0]) for a in out):
            raise ValueError("the query arrays must have one length")
        return out

    @staticmethod
    def _i32s(*tensors):
        import torch
        for t in tensors:
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != tensors[0].numel():
                raise ValueError("the query tensors must be contiguous int32 tensors of one length")
        return [C.c_void_p(t.data_ptr()) if t.numel() else None for t in tensors]

    def lce(self, a, b, max_mismatch=0, mm=False, ctx=None):
        """len[q] = how far the positions a[q] and b[q] (0 .. n) agree with at most max_mismatch mismatches -> uint32 array, or
        (len, mismatches) with mm=True: tc_esa_lce"""
        ctx = ctx or self._ctx
        a, b = self._u32s(a, b)
        ln = np.zeros(len(a), np.uint32)
        m = np.zeros(len(a), np.uint32) if mm else None
        ctx._check(ctx.lib.tc_esa_lce(ctx.handle, self._h, _ptr(a), _ptr(b), len(a), int(max_mismatch), _ptr(ln), _ptr(m)))
        return (ln, m) if mm else ln

    def lce_dev(self, d_a, d_b, max_mismatch=0, mm=False, ctx=None):
        """the same on int32 tensors resident on the device -> int32 tensor(s): tc_esa_lce_dev"""
        import torch
        ctx = ctx or self._ctx
        pa, pb = self._i32s(d_a, d_b)
        nq = d_a.numel()
        ln = torch.zeros(nq, dtype=torch.int32, device=d_a.device)
        m = torch.zeros(nq, dtype=torch.int32, device=d_a.device) if mm else None
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_lce_dev(ctx.handle, self._h, pa, pb, nq, int(max_mismatch),
                                          C.c_void_p(ln.data_ptr()) if nq else None, C.c_void_p(m.data_ptr()) if mm and nq else None))
        return (ln, m) if mm else ln

    def find(self, start, length, first_pos=True, ctx=None):
        """the substrings text[start[q] : start[q] + length[q]] -> (first_row, occ[, first_pos]), uint32 arrays: the suffix-array
        interval [first_row, first_row + occ) and the earliest occurrence: tc_esa_find"""
        ctx = ctx or self._ctx
        s, l = self._u32s(start, length)
        out = [np.zeros(len(s), np.uint32) for _ in range(3 if first_pos else 2)]
        ctx._check(ctx.lib.tc_esa_find(ctx.handle, self._h, _ptr(s), _ptr(l), len(s), _ptr(out[0]), _ptr(out[1]),
                                       _ptr(out[2]) if first_pos else None))
        return tuple(out)

    def find_dev(self, d_start, d_length, first_pos=True, ctx=None):
        """the same on int32 tensors resident on the device -> int32 tensors: tc_esa_find_dev"""
        import torch
        ctx = ctx or self._ctx
        ps, pl = self._i32s(d_start, d_length)
        nq = d_start.numel()
        out = [torch.zeros(nq, dtype=torch.int32, device=d_start.device) for _ in range(3 if first_pos else 2)]
        po = [C.c_void_p(o.data_ptr()) if nq else None for o in out] + ([] if first_pos else [None])
        torch.cuda.synchronize()
        if nq:
            ctx._check(ctx.lib.tc_esa_find_dev(ctx.handle, self._h, ps, pl, nq, *po))
        return tuple(out)

    def compare(self, a_start, a_len, b_start, b_len, common=False, ctx=None):
        """order[q] = -1, 0, 1 as text[a_start : a_start + a_len] sorts before, equals, sorts behind text[b_start : b_start + b_len]
        -> int8 array, or (order, common prefix lengths) with common=True: tc_esa_compare"""
        ctx = ctx or self._ctx
        a, la, b, lb = self._u32s(a_start, a_len, b_start, b_len)
        order = np.zeros(len(a), np.int8)
        c = np.zeros(len(a), np.uint32) if common else None
        ctx._check(ctx.lib.tc_esa_compare(ctx.handle, self._h, _ptr(a), _ptr(la), _ptr(b), _ptr(lb), len(a), _ptr(order), _ptr(c)))
        return (order, c) if common else order

    def compare_dev(self, d_a_start, d_a_len, d_b_start, d_b_len, common=False, ctx=None):
        """the same on int32 tensors resident on the device -> int8 tensor (and int32 tensor): tc_esa_compare_dev"""
        import torch
        ctx = ctx or self._ctx
        ps = self._i32s(d_a_start, d_a_len, d_b_start, d_b_len)
        nq = d_a_start.numel()
        order = torch.zeros(nq, dtype=torch.int8, device=d_a_start.device)
        c = torch.zeros(nq, dtype=torch.int32, device=d_a_start.device) if common else None
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_compare_dev(ctx.handle, self._h, *ps, nq, C.c_void_p(order.data_ptr()) if nq else None,
                                              C.c_void_p(c.data_ptr()) if common and nq else None))
        return (order, c) if common else order

    # ---- document collections (a handle of esa_build_docs): in how many documents, and in which, does a substring occur
    def doc_arrays(self):
        """-> (d_doc_start, d_da, d_pv): the device addresses of the document arrays, valid until close: tc_esa_doc_arrays"""
        p = [C.c_void_p() for _ in range(3)]
        rc = self._ctx.lib.tc_esa_doc_arrays(self._h, *(C.byref(x) for x in p))
        if rc != 0:
            raise TcError(rc, "tc_esa_doc_arrays")
        return tuple(x.value for x in p)

    def doc_count(self, start, length, limit=0, occ=False, ctx=None):
        """df[q] = the number of distinct documents in which text[start[q] : start[q] + length[q]] occurs, saturating at limit
        where limit > 0 -> uint32 array, or (df, occ) with occ=True: tc_esa_doc_count"""
        ctx = ctx or self._ctx
        s, l = self._u32s(start, length)
        df = np.zeros(len(s), np.uint32)
        oc = np.zeros(len(s), np.uint32) if occ else None
        ctx._check(ctx.lib.tc_esa_doc_count(ctx.handle, self._h, _ptr(s), _ptr(l), len(s), int(limit), _ptr(df), _ptr(oc)))
        return (df, oc) if occ else df

    def doc_count_dev(self, d_start, d_length, limit=0, occ=False, ctx=None):
        """the same on int32 tensors resident on the device -> int32 tensor(s): tc_esa_doc_count_dev"""
        import torch
        ctx = ctx or self._ctx
        ps, pl = self._i32s(d_start, d_length)
        nq = d_start.numel()
        df = torch.zeros(nq, dtype=torch.int32, device=d_start.device)
        oc = torch.zeros(nq, dtype=torch.int32, device=d_start.device) if occ else None
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_doc_count_dev(ctx.handle, self._h, ps, pl, nq, int(limit), C.c_void_p(df.data_ptr()) if nq else None,
                                                C.c_void_p(oc.data_ptr()) if occ and nq else None))
        return (df, oc) if occ else df

    def doc_list(self, start, length, limit=0, hit_pos=False, ctx=None):
        """the documents in which text[start[q] : start[q] + length[q]] occurs -> (list_offs, docs[, hit_pos]): query q's documents
        are docs[list_offs[q] : list_offs[q + 1]], in the order of their first row in the interval; hit_pos is one occurrence in
        each.  uint64 / uint32 arrays: tc_esa_doc_list (the sizes first, then the lists)"""
        ctx = ctx or self._ctx
        s, l = self._u32s(start, length)
        offs = np.zeros(len(s) + 1, np.uint64)
        total = C.c_uint64(0)
        rc = ctx.lib.tc_esa_doc_list(ctx.handle, self._h, _ptr(s), _ptr(l), len(s), int(limit), _ptr(offs), None, None, C.byref(total))
        if rc != _lib.TC_ERR_CAPACITY:
            ctx._check(rc)
        docs = np.zeros(total.value, np.uint32)
        hits = np.zeros(total.value, np.uint32) if hit_pos else None
        if total.value:
            ctx._check(ctx.lib.tc_esa_doc_list(ctx.handle, self._h, _ptr(s), _ptr(l), len(s), int(limit), _ptr(offs), _ptr(docs), _ptr(hits),
                                               C.byref(total)))
        return (offs, docs, hits) if hit_pos else (offs, docs)

    def doc_list_dev(self, d_start, d_length, limit=0, hit_pos=False, ctx=None):
        """the same on int32 tensors resident on the device -> (list_offs, an int64 tensor, docs[, hit_pos], int32 tensors):
        tc_esa_doc_list_dev"""
        import torch
        ctx = ctx or self._ctx
        ps, pl = self._i32s(d_start, d_length)
        nq = d_start.numel()
        offs = torch.zeros(nq + 1, dtype=torch.int64, device=d_start.device)
        total = C.c_uint64(0)
        torch.cuda.synchronize()
        rc = ctx.lib.tc_esa_doc_list_dev(ctx.handle, self._h, ps, pl, nq, int(limit), C.c_void_p(offs.data_ptr()), None, None, C.byref(total))
        if rc != _lib.TC_ERR_CAPACITY:
            ctx._check(rc)
        docs = torch.zeros(total.value, dtype=torch.int32, device=d_start.device)
        hits = torch.zeros(total.value, dtype=torch.int32, device=d_start.device) if hit_pos else None
        torch.cuda.synchronize()
        if total.value:
            ctx._check(ctx.lib.tc_esa_doc_list_dev(ctx.handle, self._h, ps, pl, nq, int(limit), C.c_void_p(offs.data_ptr()),
                                                   C.c_void_p(docs.data_ptr()), C.c_void_p(hits.data_ptr()) if hit_pos else None,
                                                   C.byref(total)))
        return (offs, docs, hits) if hit_pos else (offs, docs)

    def kmer_doc_count(self, k, min_df=1, max_df=0, ctx=None):
        """the number of distinct k-mers that occur in min_df .. max_df documents (max_df 0: no upper bound): the sizes-only form
        of tc_esa_kmer_docs_dev"""
        ctx = ctx or self._ctx
        nk = C.c_uint64(0)
        ctx._check(ctx.lib.tc_esa_kmer_docs_dev(ctx.handle, self._h, int(k), int(min_df), int(max_df), None, None, None, None, C.byref(nk)))
        return int(nk.value)

    def kmer_docs(self, k, min_df=1, max_df=0, ctx=None):
        """the k-mers of the text with their document frequency -> (pos, occ, df, row), uint32 arrays: the k-mers of kmers(k) in the
        same order, filtered to min_df <= df <= max_df (max_df 0: no upper bound): tc_esa_kmer_docs"""
        ctx = ctx or self._ctx
        need = self.kmer_doc_count(k, min_df, max_df, ctx=ctx)
        out = [np.zeros(need, np.uint32) for _ in range(4)]
        nk = C.c_uint64(need)
        if need:
            ctx._check(ctx.lib.tc_esa_kmer_docs(ctx.handle, self._h, int(k), int(min_df), int(max_df), *(_ptr(o) for o in out), C.byref(nk)))
        return tuple(out)

    def kmer_docs_dev(self, k, min_df=1, max_df=0, cap=None, ctx=None):
        """the same -> int32 tensors on the device: tc_esa_kmer_docs_dev.  cap: the k-mer slots to try first (None: the sizes first)"""
        import torch
        ctx = ctx or self._ctx
        cap = max(self.kmer_doc_count(k, min_df, max_df, ctx=ctx) if cap is None else int(cap), 1)
        for _ in range(2):
            out = [torch.empty(cap, dtype=torch.int32, device="cuda:%d" % ctx.device) for _ in range(4)]
            torch.cuda.synchronize()
            nk = C.c_uint64(cap)
            rc = ctx.lib.tc_esa_kmer_docs_dev(ctx.handle, self._h, int(k), int(min_df), int(max_df), *(C.c_void_p(o.data_ptr()) for o in out),
                                              C.byref(nk))
            if rc != _lib.TC_ERR_CAPACITY:
                break
            cap = max(int(nk.value), 1)
        ctx._check(rc)
        return tuple(o[:int(nk.value)] for o in out)

    def kmer_doc_spectrum(self, k, ctx=None):
        """-> (hist, distinct): hist[d], d = 0 .. ndocs, the number of distinct k-mers that occur in exactly d documents, a uint64
        array: tc_esa_kmer_doc_spectrum"""
        ctx = ctx or self._ctx
        hist = np.zeros(self.ndocs + 1, np.uint64)
        distinct = C.c_uint64()
        ctx._check(ctx.lib.tc_esa_kmer_doc_spectrum(ctx.handle, self._h, int(k), _ptr(hist), C.byref(distinct)))
        return hist, int(distinct.value)

    def kmer_doc_spectrum_dev(self, k, ctx=None):
        """the same -> (hist, an int64 tensor on the device, distinct): tc_esa_kmer_doc_spectrum_dev"""
        import torch
        ctx = ctx or self._ctx
        d_hist = torch.empty(self.ndocs + 1, dtype=torch.int64, device="cuda:%d" % ctx.device)
        distinct = C.c_uint64()
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_kmer_doc_spectrum_dev(ctx.handle, self._h, int(k), C.c_void_p(d_hist.data_ptr()), C.byref(distinct)))
        return d_hist, int(distinct.value)

    # ---- cross-document matches: which parts of each document also occur in another (or an earlier) one, and where
    def doc_match(self, kind=DOC_OTHER, clamp=True, src=False, doc=False, ctx=None):
        """xl[i] = the length of the longest match of position i that starts in another document (DOC_OTHER) or in an earlier one
        (DOC_EARLIER), clamped to the end of i's own document unless clamp=False -> uint32 array of n entries, or (xl[, src][,
        doc]) with the partner's position (ESA_NO_POS: none) and document (TC_ESA_NO_DOC: none): tc_esa_doc_match"""
        ctx = ctx or self._ctx
        out = [np.zeros(self.n, np.uint32) for _ in range(1 + bool(src) + bool(doc))]
        ps = _ptr(out[1]) if src else None
        pd = _ptr(out[-1]) if doc else None
        ctx._check(ctx.lib.tc_esa_doc_match(ctx.handle, self._h, int(kind), int(bool(clamp)), _ptr(out[0]), ps, pd))
        return tuple(out) if src or doc else out[0]

    def doc_match_dev(self, kind=DOC_OTHER, clamp=True, src=False, doc=False, ctx=None):
        """the same -> int32 tensor(s) on the device holding the 32-bit entries: tc_esa_doc_match_dev"""
        import torch
        ctx = ctx or self._ctx
        out = [torch.zeros(self.n, dtype=torch.int32, device="cuda:%d" % ctx.device) for _ in range(1 + bool(src) + bool(doc))]
        po = [C.c_void_p(o.data_ptr()) if self.n else None for o in out]
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_doc_match_dev(ctx.handle, self._h, int(kind), int(bool(clamp)), po[0], po[1] if src else None,
                                                po[-1] if doc else None))
        return tuple(out) if src or doc else out[0]

    def doc_shared(self, min_len=1, kind=DOC_OTHER, ctx=None):
        """-> (shared, longest): per document the bytes that lie in a clamped match of at least min_len bytes (a uint64 array) and the
        longest clamped match (a uint32 array): tc_esa_doc_shared"""
        ctx = ctx or self._ctx
        shared = np.zeros(self.ndocs, np.uint64)
        longest = np.zeros(self.ndocs, np.uint32)
        ctx._check(ctx.lib.tc_esa_doc_shared(ctx.handle, self._h, int(kind), int(min_len), _ptr(shared), _ptr(longest)))
        return shared, longest

    def doc_shared_dev(self, min_len=1, kind=DOC_OTHER, ctx=None):
        """the same -> (an int64 tensor, an int32 tensor) on the device: tc_esa_doc_shared_dev"""
        import torch
        ctx = ctx or self._ctx
        shared = torch.zeros(self.ndocs, dtype=torch.int64, device="cuda:%d" % ctx.device)
        longest = torch.zeros(self.ndocs, dtype=torch.int32, device="cuda:%d" % ctx.device)
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_esa_doc_shared_dev(ctx.handle, self._h, int(kind), int(min_len), C.c_void_p(shared.data_ptr()) if self.ndocs else None,
                                                 C.c_void_p(longest.data_ptr()) if self.ndocs else None))
        return shared, longest

    def shared_spans_dev(self, min_len, kind=DOC_OTHER, cap=None, ctx=None):
        """-> (start, len, covered): the maximal stretches of the text that clamped matches of at least min_len bytes cover:
        doc_match_dev(clamp=True), then Context.cover_spans_dev"""
        ctx = ctx or self._ctx
        return ctx.cover_spans_dev(self.doc_match_dev(kind=kind, clamp=True, ctx=ctx), min_len, cap=cap)

    def shared_mask_dev(self, min_len, kind=DOC_OTHER, map=None, ctx=None):
        """-> (out, covered): the text with what each document shares with the others (DOC_EARLIER: with earlier ones) masked:
        doc_match_dev(clamp=True), then Context.cover_mask_dev on the handle's text"""
        ctx = ctx or self._ctx
        return ctx.cover_mask_dev(self.doc_match_dev(kind=kind, clamp=True, ctx=ctx), self.read_dev("text", ctx=ctx), min_len, map=map)

    def shared_dedup_dev(self, min_len, kind=DOC_OTHER, cap=None, ctx=None):
        """-> (out, covered): the text without the covered bytes; with DOC_EARLIER the first copy of everything stays:
        doc_match_dev(clamp=True), then Context.cover_dedup_dev on the handle's text"""
        ctx = ctx or self._ctx
        return ctx.cover_dedup_dev(self.doc_match_dev(kind=kind, clamp=True, ctx=ctx), self.read_dev("text", ctx=ctx), min_len, cap=cap)

    def shared_spans(self, min_len, kind=DOC_OTHER, cap=None, ctx=None):
        """shared_spans_dev -> (start, len, covered) with uint32 host arrays"""
        s, l, cov = self.shared_spans_dev(min_len, kind=kind, cap=cap, ctx=ctx)
        return s.cpu().numpy().view(np.uint32), l.cpu().numpy().view(np.uint32), cov

    def shared_mask(self, min_len, kind=DOC_OTHER, map=None, ctx=None):
        """shared_mask_dev -> (out, covered) with a uint8 host array"""
        out, cov = self.shared_mask_dev(min_len, kind=kind, map=map, ctx=ctx)
        return out.cpu().numpy(), cov

    def shared_dedup(self, min_len, kind=DOC_OTHER, cap=None, ctx=None):
        """shared_dedup_dev -> (out, covered) with a uint8 host array"""
        out, cov = self.shared_dedup_dev(min_len, kind=kind, cap=cap, ctx=ctx)
        return out.cpu().numpy(), cov

    # ---- further analyses on the arrays the handle keeps: the sort is paid once
    def arrays(self):
        """-> (d_text, d_sa, d_lcp, d_isa): the device addresses of the handle's arrays, valid until close: tc_esa_arrays"""
        p = [C.c_void_p() for _ in range(4)]
        rc = self._ctx.lib.tc_esa_arrays(self._h, *(C.byref(x) for x in p))
        if rc != 0:
            raise TcError(rc, "tc_esa_arrays")
        return tuple(x.value for x in p)

    def kmers(self, k, min_occ=1, max_occ=0, cap=None, ctx=None):
        """the k-mers of the text -> (pos, occ, row), int32 tensors on the device, as Context.kmers_dev answers them, from the
        handle's sa and lcp: tc_kmers_esa_dev"""
        ctx = ctx or self._ctx
        _, psa, plcp, _ = self.arrays()
        N = self.n + 1
        return ctx._kmers_retry(lambda p, o, r, nk: ctx.lib.tc_kmers_esa_dev(ctx.handle, psa, plcp, N, k, min_occ, max_occ, p, o, r, nk),
                                "cuda:%d" % ctx.device, cap)

    def kmer_spectrum(self, k, bins=256, ctx=None):
        """-> (hist, an int64 tensor of `bins` entries on the device, distinct, total): tc_kmer_spectrum_esa_dev"""
        import torch
        ctx = ctx or self._ctx
        _, psa, plcp, _ = self.arrays()
        d_hist = torch.empty(max(bins, 1), dtype=torch.int64, device="cuda:%d" % ctx.device)
        distinct, total = C.c_uint64(), C.c_uint64()
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_kmer_spectrum_esa_dev(ctx.handle, psa, plcp, self.n + 1, k, bins, C.c_void_p(d_hist.data_ptr()),
                                                    C.byref(distinct), C.byref(total)))
        return d_hist, int(distinct.value), int(total.value)

    def kmer_profile(self, kmax, unique=True, ctx=None):
        """-> (distinct, unique), uint64 host arrays of kmax entries: tc_kmer_profile_esa_dev"""
        ctx = ctx or self._ctx
        _, _, plcp, _ = self.arrays()
        d = np.empty(max(kmax, 1), np.uint64)
        u = np.empty(max(kmax, 1), np.uint64) if unique else None
        ctx._check(ctx.lib.tc_kmer_profile_esa_dev(ctx.handle, plcp, self.n + 1, kmax, _ptr(d), _ptr(u) if unique else None))
        return d[:kmax], (u[:kmax] if unique else None)


_DEFAULT = None


def concat_docs(docs):
    """a list of bytes-likes -> (text, doc_start): their concatenation without separators as a uint8 array and the ndocs + 1
    boundaries as a uint32 array, what Context.esa_build_docs takes"""
    parts = [_u8(d) for d in docs]
    doc_start = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(p) for p in parts], out=doc_start[1:])
    if doc_start[-1] > _lib.TC_MAX_N:
        raise ValueError("the documents have more than TC_MAX_N bytes")
    text = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8), doc_start.astype(np.uint32)


def absent_word_bytes(text, left, pos, ln):
    """the words of Context.absent_words as a list of bytes, in list order: left[k] followed by
    text[pos[k] : pos[k] + len[k] - 1].  For small results: the words of a long text need O(sigma n) bytes each."""
    t = _u8(text).tobytes()
    return [bytes([int(a)]) + t[int(p):int(p) + int(l) - 1] for a, p, l in zip(np.asarray(left), np.asarray(pos), np.asarray(ln))]


def container_coding(blob):
    """"packed" or "huffman": the coding of a container, from its header alone (tc_container_coding)."""
    b = np.frombuffer(bytes(blob[:_lib.TC_CONTAINER_HEADER]), np.uint8)
    out = C.c_int(-1)
    ctx = default_context()
    ctx._check(ctx.lib.tc_container_coding(ctx.handle, _ptr(b), len(b), C.byref(out)))
    return _CODING_NAMES[out.value]


def default_context():
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Context(0)
    return _DEFAULT


from . import bwt, fmindex, mtf, rle  # noqa: E402,F401
