"""Pure numpy / Python restatement of the Huffman container body (run format id 3), written from the format text
in include/textcomp.h ("Body of a format-3 container") and from nothing else: token stream from runs, canonical
codes from lengths, the chunked writer and a reader.  Test infrastructure: tests/test_huffman_format.py pins it on
the oracle's runs without a GPU; tests/test_gpu_container_huffman.py then uses its reader as the judge of what the
device writes."""
import heapq
import struct

import numpy as np

K_DEFAULT = 1024
LMAX_FORMAT = 12     # the format's limit on L_max


class Malformed(ValueError):
    pass


def _pad16(b):
    return (b + 15) & ~15


# ---- tokens -----------------------------------------------------------------------------------------------------------
def tokens_of_runs(counts, vals, sigma):
    """-> (tokens int64[], first int64[nruns + 1]: index of every run's value token, then the token count).
    A run (v, c >= 1): token v, then the digits of c - 1 in bijective base 2, least significant first,
    RUNA = sigma for digit 1 and RUNB = sigma + 1 for digit 2."""
    c = np.asarray(counts, dtype=np.int64)
    v = np.asarray(vals, dtype=np.int64)
    if len(c) and (c.min() < 1 or c.max() > 0xFFFFFFFF or v.min() < 0 or v.max() >= sigma):
        raise ValueError("a run without tokens (count 0, or value >= sigma)")
    m = c - 1
    # digits of m in bijective base 2: while m > 0: d = 2 - (m & 1); emit d; m = (m - d) >> 1
    ndig = np.zeros(len(c), dtype=np.int64)
    t = m.copy()
    digs = []
    while True:
        live = t > 0
        if not live.any():
            break
        d = np.where(live, 2 - (t & 1), 0)
        digs.append(d)
        ndig += live
        t = np.where(live, (t - d) >> 1, 0)
    ln = 1 + ndig
    first = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    tok = np.empty(int(first[-1]), dtype=np.int64)
    tok[first[:-1]] = v
    for j, d in enumerate(digs):
        sel = d > 0
        tok[first[:-1][sel] + 1 + j] = sigma + d[sel] - 1
    return tok, first


def runs_of_tokens(tok, sigma):
    """inverse of tokens_of_runs for ONE chunk's tokens; raises Malformed"""
    tok = np.asarray(tok, dtype=np.int64)
    if len(tok) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    isval = tok < sigma
    if not isval[0]:
        raise Malformed("a digit before any value token")
    run = np.cumsum(isval) - 1
    starts = np.nonzero(isval)[0]
    j = np.arange(len(tok)) - starts[run] - 1          # digit index inside its run (-1 for the value token)
    if j.max() >= 31:
        raise Malformed("more than 31 digits")
    m = np.zeros(len(starts), dtype=np.int64)
    dsel = ~isval
    np.add.at(m, run[dsel], (tok[dsel] - sigma + 1) << j[dsel])
    return m + 1, tok[starts]


# ---- code ---------------------------------------------------------------------------------------------------------------
def canonical_codes(lengths):
    """coded tokens in (length, token) order get consecutive values from 0, shifted left at every step up in length"""
    lengths = np.asarray(lengths, dtype=np.int64)
    codes = np.zeros(len(lengths), dtype=np.int64)
    code, prev = 0, None
    for ln, s in sorted((int(l), s) for s, l in enumerate(lengths) if l > 0):
        if prev is not None:
            code = (code + 1) << (ln - prev)
        codes[s] = code
        prev = ln
    return codes


def kraft(lengths, lmax):
    """sum of 2^-length over the coded tokens, in units of 2^-lmax"""
    return sum(1 << (lmax - int(l)) for l in lengths if l > 0)


def build_lengths(hist, lmax=LMAX_FORMAT):
    """length-limited optimal code lengths (package-merge); 0 for a token that does not occur, 1 for a lone token"""
    hist = [int(h) for h in hist]
    syms = sorted((s for s, h in enumerate(hist) if h > 0), key=lambda s: (hist[s], s))
    out = [0] * len(hist)
    if len(syms) == 1:
        out[syms[0]] = 1
    if len(syms) < 2:
        return np.array(out, dtype=np.uint8)
    m = len(syms)
    leaves = [(hist[s], (j,)) for j, s in enumerate(syms)]
    prev = list(leaves)
    for _ in range(lmax - 1):
        pk = [(prev[i][0] + prev[i + 1][0], prev[i][1] + prev[i + 1][1]) for i in range(0, len(prev) - 1, 2)]
        cur, x, y = [], 0, 0
        while x < m or y < len(pk):
            if y >= len(pk) or (x < m and leaves[x][0] <= pk[y][0]):
                cur.append(leaves[x]); x += 1
            else:
                cur.append(pk[y]); y += 1
        prev = cur
    for _, cover in prev[:2 * m - 2]:
        for j in cover:
            out[syms[j]] += 1
    return np.array(out, dtype=np.uint8)


def optimal_huffman_bits(hist):
    """cost in bits of an optimal Huffman code WITHOUT a length limit over the histogram (a lone token: 1 bit each)"""
    h = [int(x) for x in hist if x > 0]
    if len(h) == 1:
        return h[0]
    heapq.heapify(h)
    total = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        total += a + b
        heapq.heappush(h, a + b)
    return total


def histogram(counts, vals, sigma):
    tok, _ = tokens_of_runs(counts, vals, sigma)
    return np.bincount(tok, minlength=sigma + 2)


# ---- writer -------------------------------------------------------------------------------------------------------------
def write_body(counts, vals, sigma, lengths=None, K=K_DEFAULT, lmax=LMAX_FORMAT):
    """runs -> body bytes (head, lengths, directory of chunk bit counts, payload words; each padded to 16)"""
    nruns = len(counts)
    tok, first = tokens_of_runs(counts, vals, sigma)
    nsyms = sigma + 2
    if lengths is None:
        lengths = build_lengths(np.bincount(tok, minlength=nsyms), lmax)
    lengths = np.asarray(lengths, dtype=np.int64)
    codes = canonical_codes(lengths)
    nchunks = (nruns + K - 1) // K
    tl = lengths[tok]
    if len(tl) and tl.min() < 1:
        raise ValueError("a token without a code")
    cum = np.concatenate([[0], np.cumsum(tl)])                 # bits before every token
    ctok = first[np.minimum(np.arange(nchunks + 1) * K, nruns)]   # first token of every chunk (and the end)
    cbit = cum[ctok]
    chunk_bits = np.diff(cbit)
    chunk_words = (chunk_bits + 31) // 32
    wstart = np.concatenate([[0], np.cumsum(chunk_words)])
    nwords = int(wstart[-1])
    chunk_of_tok = np.searchsorted(ctok[1:], np.arange(len(tok)), side="right")
    pos = wstart[chunk_of_tok] * 32 + (cum[:-1] - cbit[chunk_of_tok])   # bit position of every token in the payload
    bits = np.zeros(nwords * 32, dtype=np.uint8)
    tc = codes[tok]
    for b in range(int(tl.max()) if len(tl) else 0):
        sel = tl > b
        bits[pos[sel] + b] = (tc[sel] >> (tl[sel] - 1 - b)) & 1
    # stream bit b of a word is its bit 31 - (b mod 32): big-endian bit order inside little-endian stored words
    words = np.packbits(bits).view(">u4").astype("<u4")
    head = struct.pack("<4I", K, nchunks, nsyms, lmax)
    lens = lengths.astype(np.uint8).tobytes()
    lens += bytes(_pad16(len(lens)) - len(lens))
    dirb = chunk_bits.astype("<u4").tobytes()
    dirb += bytes(_pad16(len(dirb)) - len(dirb))
    pay = words.tobytes()
    pay += bytes(_pad16(len(pay)) - len(pay))
    return head + lens + dirb + pay


# ---- reader -------------------------------------------------------------------------------------------------------------
def parse_body(body, nruns, sigma):
    """validates head, lengths and directory -> dict(K, nchunks, lmax, lengths, chunk_bits, words)"""
    body = bytes(body)
    nsyms = sigma + 2
    if len(body) < 16 + _pad16(nsyms) or len(body) % 16:
        raise Malformed("body too short")
    K, nchunks, hs, lmax = struct.unpack_from("<4I", body, 0)
    if K == 0 or K & (K - 1):
        raise Malformed("K is no power of two")
    if hs != nsyms:
        raise Malformed("nsyms != sigma + 2")
    if not 1 <= lmax <= LMAX_FORMAT:
        raise Malformed("L_max outside 1..12")
    if nchunks != (nruns + K - 1) // K:
        raise Malformed("nchunks != ceil(nruns / K)")
    lengths = np.frombuffer(body, np.uint8, nsyms, 16).astype(np.int64)
    if lengths.max() > lmax:
        raise Malformed("a length above L_max")
    if kraft(lengths, lmax) > (1 << lmax):
        raise Malformed("Kraft sum above 1")
    doff = 16 + _pad16(nsyms)
    poff = doff + _pad16(4 * nchunks)
    if poff > len(body):
        raise Malformed("directory longer than the body")
    chunk_bits = np.frombuffer(body, "<u4", nchunks, doff).astype(np.int64)
    nwords = int(((chunk_bits + 31) // 32).sum())
    if _pad16(4 * nwords) != len(body) - poff:
        raise Malformed("directory does not sum to the payload")
    words = np.frombuffer(body, "<u4", nwords, poff)
    return dict(K=K, nchunks=nchunks, lmax=lmax, lengths=lengths, chunk_bits=chunk_bits, words=words)


def read_body(body, nruns, sigma):
    """body bytes -> (counts int64[nruns], vals int64[nruns]); raises Malformed"""
    p = parse_body(body, nruns, sigma)
    K, lmax, lengths, chunk_bits = p["K"], p["lmax"], p["lengths"], p["chunk_bits"]
    codes = canonical_codes(lengths)
    # what starts at every bit position: one table lookup on the next lmax bits
    tab_sym = np.full(1 << lmax, -1, dtype=np.int64)
    tab_len = np.zeros(1 << lmax, dtype=np.int64)
    for s in np.nonzero(lengths)[0]:
        lo = int(codes[s]) << (lmax - int(lengths[s]))
        tab_sym[lo:lo + (1 << (lmax - int(lengths[s])))] = s
        tab_len[lo:lo + (1 << (lmax - int(lengths[s])))] = lengths[s]
    bits = np.unpackbits(p["words"].astype(">u4").view(np.uint8))
    ext = np.concatenate([bits, np.zeros(lmax, np.uint8)]).astype(np.int64)
    win = np.zeros(len(bits), dtype=np.int64)
    for i in range(lmax):
        win = (win << 1) | ext[i:i + len(bits)]
    sym_at, len_at = tab_sym[win], tab_len[win]
    nxt = (np.arange(len(bits)) + len_at).tolist()
    ok = (sym_at >= 0).tolist()
    out_c, out_v = [], []
    w0 = 0
    for k in range(p["nchunks"]):
        q, end = w0 * 32, w0 * 32 + int(chunk_bits[k])
        at = []
        while q < end:
            if not ok[q]:
                raise Malformed("bits that match no code")
            at.append(q)
            q = nxt[q]
        if q != end:
            raise Malformed("a chunk ends inside a code")
        c, v = runs_of_tokens(sym_at[at], sigma)
        if len(c) != min(K, nruns - k * K):
            raise Malformed("chunk %d holds %d runs" % (k, len(c)))
        out_c.append(c)
        out_v.append(v)
        w0 += (int(chunk_bits[k]) + 31) // 32
    if not out_c:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_c), np.concatenate(out_v)


# ---- the packed bodies' sizes (include/textcomp.h, "encoded-block wire format"), for the never-larger rule ---------------
def packed_body_bytes(counts, sigma):
    c = np.asarray(counts, dtype=np.int64)
    n = len(c)
    if n == 0:
        return 0
    if sigma <= 6:
        nib = int(np.where((c == 1) | (c == 2), 1, 2).sum())
        return (nib + 31) // 32 * 16 + 4 * int(((c == 0) | (c >= 5)).sum())
    if sigma <= 16:
        return ((n + 7) & ~7) + 8 * int((c >= 15).sum())
    return ((2 * n + 7) & ~7) + 8 * int((c >= 127).sum())
