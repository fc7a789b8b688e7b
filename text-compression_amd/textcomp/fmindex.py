"""Mirror of Data.FMIndex count / locate (reference src/Data/FMIndex.hs:49-82),
ByteString instantiation."""
from . import default_context


def bytestringFMIndexCountS(pats, text, ctx=None):
    """bytestringFMIndexCountS :: [ByteString] -> ByteString -> Seq (ByteString, Maybe Int)
    (FMIndex.hs:362-379).  Empty pattern list or empty input => empty result."""
    if len(pats) == 0 or len(text) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text)
    try:
        counts = fm.count(pats)
    finally:
        fm.close()
    return [(p, None if c == 0 else int(c)) for p, c in zip(pats, counts)]


def bytestringFMIndexCountP(pats, text, ctx=None):
    """bytestringFMIndexCountP (FMIndex.hs:411-432): same values, same order; the
    spark pool over patterns is one batched launch here."""
    return bytestringFMIndexCountS(pats, text, ctx)


def bytestringFMIndexLocateS(pats, text, ctx=None):
    """bytestringFMIndexLocateS (FMIndex.hs:475-497): 1-based positions, SA order."""
    if len(pats) == 0 or len(text) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text)
    try:
        hits = fm.locate(pats)
    finally:
        fm.close()
    return [(p, [int(v) for v in h]) for p, h in zip(pats, hits)]


def bytestringFMIndexLocateP(pats, text, ctx=None):
    """bytestringFMIndexLocateP (FMIndex.hs:538-563)."""
    return bytestringFMIndexLocateS(pats, text, ctx)


# ---- search with mismatches (no counterpart in the reference; the value shapes of the count / locate mirrors above) ----
def bytestringFMIndexCountMismatchS(pats, text, k, ctx=None):
    """[(pattern, Maybe Int)]: the text positions within Hamming distance k of each pattern (substitutions only, k at
    most TC_FM_MAX_MISMATCH), Nothing for none.  A pattern byte that does not occur in the text can only be a
    mismatch.  Empty pattern list or empty input => empty result."""
    if len(pats) == 0 or len(text) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text)
    try:
        counts = fm.count_mm(pats, k)
    finally:
        fm.close()
    return [(p, None if c == 0 else int(c)) for p, c in zip(pats, counts)]


def bytestringFMIndexCountMismatchP(pats, text, k, ctx=None):
    """the same values in the same order: the batch is one launch either way"""
    return bytestringFMIndexCountMismatchS(pats, text, k, ctx)


def bytestringFMIndexLocateMismatchS(pats, text, k, ctx=None):
    """[(pattern, [(position, mismatches)])]: 1-based positions within Hamming distance k, each once, in the device's
    enumeration order (deterministic, not sorted)."""
    if len(pats) == 0 or len(text) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text)
    try:
        hits = fm.locate_mm(pats, k)
    finally:
        fm.close()
    return [(p, [(int(v), int(d)) for v, d in zip(h, mm)]) for p, (h, mm) in zip(pats, hits)]


def bytestringFMIndexLocateMismatchP(pats, text, k, ctx=None):
    return bytestringFMIndexLocateMismatchS(pats, text, k, ctx)


# ---- factorize (no counterpart in the reference; the value shape of the locate mirrors above) ----
def bytestringFMIndexFactorizeS(pats, text, ctx=None):
    """[(pattern, [(pos, len)])]: the greedy right-to-left longest-match parse of each pattern against the text, factors
    in pattern order, in the ABI's convention: a match is (1-based text position of the occurrence in the first
    suffix-array row, length >= 1), a literal -- a byte the text does not hold -- is (byte value, 0).  Empty pattern list
    => empty result; against an empty text every byte is a literal."""
    if len(pats) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text)
    try:
        foffs, fpos, flen = fm.factorize(pats)
    finally:
        fm.close()
    return [(p, [(int(fpos[f]), int(flen[f])) for f in range(int(foffs[i]), int(foffs[i + 1]))]) for i, p in enumerate(pats)]


def bytestringFMIndexFactorizeP(pats, text, ctx=None):
    """the same values in the same order: the batch is one launch either way"""
    return bytestringFMIndexFactorizeS(pats, text, ctx)


# ---- matching statistics and maximal exact matches (no counterpart in the reference) ----
def bytestringFMIndexMatchStatsS(pats, text, ctx=None):
    """[(pattern, [(len, pos, occ)])]: for every position of each pattern the length of the longest match that starts
    there, the 1-based text position of its occurrence in the first suffix-array row and the number of its occurrences;
    (0, 0, 0) where the byte does not occur in the text.  Empty pattern list => empty result; against an empty text every
    entry is (0, 0, 0)."""
    if len(pats) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text, lcp=True)
    try:
        ms_len, ms_pos, ms_occ = fm.match_stats(pats)
    finally:
        fm.close()
    out, o = [], 0
    for p in pats:
        out.append((p, [(int(ms_len[o + i]), int(ms_pos[o + i]), int(ms_occ[o + i])) for i in range(len(p))]))
        o += len(p)
    return out


def bytestringFMIndexMatchStatsP(pats, text, ctx=None):
    """the same values in the same order: the batch is one launch either way"""
    return bytestringFMIndexMatchStatsS(pats, text, ctx)


def bytestringFMIndexMemsS(pats, text, min_len=1, ctx=None):
    """[(pattern, [(start, pos, len)])]: the maximal exact matches of at least min_len bytes of each pattern, in
    increasing start (0-based in the pattern); pos as in bytestringFMIndexMatchStatsS."""
    if len(pats) == 0:
        return []
    fm = (ctx or default_context()).fm_build(text, lcp=True)
    try:
        moffs, mstart, mpos, mlen = fm.mems(pats, min_len)
    finally:
        fm.close()
    return [(p, [(int(mstart[k]), int(mpos[k]), int(mlen[k])) for k in range(int(moffs[i]), int(moffs[i + 1]))])
            for i, p in enumerate(pats)]


def bytestringFMIndexMemsP(pats, text, min_len=1, ctx=None):
    return bytestringFMIndexMemsS(pats, text, min_len, ctx)


# ---- Text instantiations (FMIndex.hs:385-403,436-462,503-530,570-599) ----------------------------
# The index is built over the UTF-8 bytes, each turned into a Text by decodeUtf8 . BS.singleton
# (ASCII only, an exception otherwise); patterns are split into characters.  For ASCII input that is
# byte matching, which is what runs here; anything else raises as the reference does.
def _ascii_bytes(text):
    b = text.encode("utf-8")
    for v in b:
        if v >= 0x80:
            bytes([v]).decode("utf-8")     # raises UnicodeDecodeError like decodeUtf8
    return b


def textFMIndexCountS(pats, text, ctx=None):
    """textFMIndexCountS :: [Text] -> Text -> Seq (Text, Maybe Int) (FMIndex.hs:385-402)."""
    if len(pats) == 0 or len(text) == 0:
        return []
    res = bytestringFMIndexCountS([p.encode("utf-8") for p in pats], _ascii_bytes(text), ctx)
    return [(p, c) for p, (_, c) in zip(pats, res)]


def textFMIndexCountP(pats, text, ctx=None):
    """textFMIndexCountP (FMIndex.hs:441-462)."""
    return textFMIndexCountS(pats, text, ctx)


def textFMIndexLocateS(pats, text, ctx=None):
    """textFMIndexLocateS (FMIndex.hs:505-527)."""
    if len(pats) == 0 or len(text) == 0:
        return []
    res = bytestringFMIndexLocateS([p.encode("utf-8") for p in pats], _ascii_bytes(text), ctx)
    return [(p, h) for p, (_, h) in zip(pats, res)]


def textFMIndexLocateP(pats, text, ctx=None):
    """textFMIndexLocateP (FMIndex.hs:574-599)."""
    return textFMIndexLocateS(pats, text, ctx)


# ---- the FMIndex VALUE (FMIndex/Internal.hs:153-170) ------------------------------------------
# FMIndex (Cc, OccCK, SA): sigma pairs, sigma x N triples and N suffix records -- O(sigma N + N^2)
# elements, a shape for small inputs (the reference builds it through the O(n^2) rotation matrix).
# The device supplies what the path computes (BWT, C array, suffix array); the Seq-of-tuples shape
# is laid out here.  count / locate never materialise it: they run on the device index (`tc_fm`).
def bytestringToBWTToFMIndexB(bs, ctx=None):
    """bytestringToBWTToFMIndexB :: ByteString -> FMIndex ByteString (FMIndex.hs:108-111,162-183):
    (Cc, OccCK, SA) with Cc = [(C[c], c)], OccCK = [(c, [(k, Occ(c, k), L[k])  k = 1..N])] for the
    present symbols c in order (Nothing first, Occ inclusive of k; seqToCc / seqToOccCK,
    FMIndex/Internal.hs:195-316) and SA = [(suffixindex, suffixstartpos, suffix)], 1-based
    (createSuffixArray, BWT/Internal.hs:110-134)."""
    from . import bwt as _bwt
    if len(bs) == 0:
        return [], [], []
    c = ctx or default_context()
    B = _bwt.bytestringToBWT(bs, c)
    fm = c.fm_build(bs)
    try:
        info = fm.info()
    finally:
        fm.close()
    el = lambda s: None if s < 0 else bytes([int(s)])
    cc = [(int(v), el(s)) for s, v in zip(info["c_sym"], info["c_val"])]
    Lb = [None if v is None else bytes([v]) for v in B]
    occck = []
    for _, sym in cc:
        run, col = 0, []
        for k, x in enumerate(Lb, start=1):
            if x == sym:
                run += 1
            col.append((k, run, x))
        occck.append((sym, col))
    sa = c.suffix_array(bs)
    sarec = [(j + 1, int(p) + 1, bytes(bs[int(p):])) for j, p in enumerate(sa)]
    return cc, occck, sarec


def textToBWTToFMIndexB(text, ctx=None):
    """textToBWTToFMIndexB (FMIndex.hs:122-125)."""
    return bytestringToBWTToFMIndexB(text.encode("utf-8"), ctx)


def bytestringFromBWTFromFMIndexB(fmi, ctx=None):
    """bytestringFromBWTFromFMIndexB (FMIndex.hs:244-246): the text back from the index -- the BWT is
    the third component of the first OccCK row (seqFromFMIndex, FMIndex/Internal.hs:324-338)."""
    from . import bwt as _bwt
    cc, occck, sa = fmi
    if len(cc) == 0 or len(occck) == 0 or len(sa) == 0:
        return b""
    return _bwt.bytestringFromByteStringBWT([x for _, _, x in occck[0][1]], ctx)


def textFMIndexCountMismatchS(pats, text, k, ctx=None):
    """bytestringFMIndexCountMismatchS over the UTF-8 bytes (ASCII only, as the other text... variants)."""
    if len(pats) == 0 or len(text) == 0:
        return []
    res = bytestringFMIndexCountMismatchS([p.encode("utf-8") for p in pats], _ascii_bytes(text), k, ctx)
    return [(p, c) for p, (_, c) in zip(pats, res)]


def textFMIndexCountMismatchP(pats, text, k, ctx=None):
    return textFMIndexCountMismatchS(pats, text, k, ctx)


def textFMIndexLocateMismatchS(pats, text, k, ctx=None):
    """bytestringFMIndexLocateMismatchS over the UTF-8 bytes (ASCII only)."""
    if len(pats) == 0 or len(text) == 0:
        return []
    res = bytestringFMIndexLocateMismatchS([p.encode("utf-8") for p in pats], _ascii_bytes(text), k, ctx)
    return [(p, h) for p, (_, h) in zip(pats, res)]


def textFMIndexLocateMismatchP(pats, text, k, ctx=None):
    return textFMIndexLocateMismatchS(pats, text, k, ctx)


def textFMIndexFactorizeS(pats, text, ctx=None):
    """bytestringFMIndexFactorizeS over the UTF-8 bytes (ASCII only, as the other text... variants)."""
    if len(pats) == 0:
        return []
    res = bytestringFMIndexFactorizeS([p.encode("utf-8") for p in pats], _ascii_bytes(text), ctx)
    return [(p, f) for p, (_, f) in zip(pats, res)]


def textFMIndexFactorizeP(pats, text, ctx=None):
    return textFMIndexFactorizeS(pats, text, ctx)


def textFMIndexMatchStatsS(pats, text, ctx=None):
    """bytestringFMIndexMatchStatsS over the UTF-8 bytes (ASCII only, as the other text... variants)."""
    if len(pats) == 0:
        return []
    res = bytestringFMIndexMatchStatsS([p.encode("utf-8") for p in pats], _ascii_bytes(text), ctx)
    return [(p, f) for p, (_, f) in zip(pats, res)]


def textFMIndexMatchStatsP(pats, text, ctx=None):
    return textFMIndexMatchStatsS(pats, text, ctx)


def textFMIndexMemsS(pats, text, min_len=1, ctx=None):
    """bytestringFMIndexMemsS over the UTF-8 bytes (ASCII only)."""
    if len(pats) == 0:
        return []
    res = bytestringFMIndexMemsS([p.encode("utf-8") for p in pats], _ascii_bytes(text), min_len, ctx)
    return [(p, f) for p, (_, f) in zip(pats, res)]


def textFMIndexMemsP(pats, text, min_len=1, ctx=None):
    return textFMIndexMemsS(pats, text, min_len, ctx)
