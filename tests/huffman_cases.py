"""Shared by the Huffman container tests (a plain module, no test in it): the container header / checksum helpers of
tests/test_gpu_container_huffman.py, the SYNTHETIC run lists of tests/test_gpu_huffman_synthetic.py -- run lists no
text produces, each named for the regime of csrc/tc_huff.hpp it is meant to reach -- the measurements that say whether
a run list reaches its regime, and the seeded single mutations of a body.  Everything here is numpy on the CPU, so
tests/test_huffman_format.py pins the restatement on the same run lists where no GPU is present."""
import heapq
import struct

import numpy as np

import huffman_format as H

PACKED, HUFFMAN = 0, 1
HDR = 640
IMG_WORDS = 1024          # HF_IMG_WORDS: the LDS window of huff_encode_kernel<true>
RPT = 4                   # HF_RPT: consecutive runs per thread
SCAN_TURN = 8192          # entries huff_dir_scan_kernel takes per turn
U32_MAX = (1 << 32) - 1


# ---- container header, checksum ---------------------------------------------------------------------------------------
def header(blob):
    magic, n, prim, nruns, nesc, body, csum, sigma, fmt = struct.unpack_from("<8s6Q2I", blob, 0)
    assert magic == b"TCBLK01\0"
    return dict(n=n, primary=prim, nruns=nruns, nesc=nesc, body=body, checksum=csum, sigma=sigma, format=fmt)


def checksum64(body):
    """tests/long/parity_digest.py:28, the numpy restatement of the container checksum"""
    w = np.frombuffer(body, "<u4").astype(np.uint64)
    i = np.arange(len(w), dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = ((w << np.uint64(32)) | (i & np.uint64(0xFFFFFFFF))) + (i >> np.uint64(32)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        acc = int(z.sum(dtype=np.uint64))
    return acc ^ ((len(body) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1))


def resealed(blob, body):
    """the container with another body, sizes and checksum made consistent so that only the body's content is wrong"""
    b = bytearray(blob[:HDR]) + bytearray(body)
    struct.pack_into("<Q", b, 40, len(body))
    struct.pack_into("<Q", b, 48, checksum64(bytes(body)))
    return bytes(b)


def as_format3(blob, body):
    """a device-written container of the same nruns, sigma and final list, carrying `body` as a format-3 body"""
    b = bytearray(resealed(blob, body))
    struct.pack_into("<Q", b, 32, 0)      # nesc
    struct.pack_into("<I", b, 60, 3)      # format
    return bytes(b)


def set_coding(ctx, coding):
    assert ctx.lib.tc_ctx_set_container_coding(ctx.handle, coding) == 0


# ---- what a run list reaches ------------------------------------------------------------------------------------------
def unlimited_lengths(hist):
    """code lengths of an optimal Huffman code WITHOUT a length limit (a lone token: 1)"""
    hist = [int(h) for h in hist]
    out = [0] * len(hist)
    heap = [(h, s, (s,)) for s, h in enumerate(hist) if h > 0]
    if len(heap) == 1:
        out[heap[0][1]] = 1
        return out
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            out[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return out


def ndigits(counts):
    """digit tokens of every run: floor(log2 c)"""
    c = np.asarray(counts, dtype=np.int64)
    nd = np.zeros(len(c), dtype=np.int64)
    for b in range(1, 32):
        nd += c >= (1 << b)
    return nd


def run_bits(counts, vals, sigma, lengths):
    """bits of every run under `lengths`"""
    c = np.asarray(counts, dtype=np.int64)
    v = np.asarray(vals, dtype=np.int64)
    ln = np.asarray(lengths, dtype=np.int64)
    nd = ndigits(c)
    nb = _popcount(c) - 1
    return ln[v] + (nd - nb) * ln[sigma] + nb * ln[sigma + 1]


def _popcount(c):
    c = c.astype(np.uint64)
    n = np.zeros(len(c), dtype=np.int64)
    for b in range(32):
        n += ((c >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


def regime(counts, vals, sigma, K=H.K_DEFAULT, lmax=H.LMAX_FORMAT, lengths=None):
    """dict of what the run list reaches under the restatement's own lengths (or `lengths`)"""
    hist = H.histogram(counts, vals, sigma)
    if lengths is None:
        lengths = H.build_lengths(hist, lmax)
    lengths = np.asarray(lengths, dtype=np.int64)
    rb = run_bits(counts, vals, sigma, lengths)
    n = len(rb)
    nchunks = (n + K - 1) // K
    cum = np.concatenate([[0], np.cumsum(rb)])
    edges = np.minimum(np.arange(nchunks + 1) * K, n)
    chunk_bits = np.diff(cum[edges])
    unl = unlimited_lengths(hist)
    # threads (RPT consecutive runs of a chunk) whose bits cross a window boundary of their chunk
    straddlers = 0
    if K == H.K_DEFAULT:
        g0 = np.arange(0, n, RPT)
        g1 = np.minimum(g0 + RPT, n)
        k = g0 // K
        start = cum[g0] - cum[edges[k]]
        end = cum[g1] - cum[edges[k]]          # (a group never crosses a chunk: RPT divides K)
        some = end > start
        straddlers = int((some & ((start >> 5) // IMG_WORDS != ((end - 1) >> 5) // IMG_WORDS)).sum())
    return dict(hist=hist, lengths=lengths, coded=int((hist > 0).sum()), longest=int(lengths.max()),
                unlimited_depth=max(unl), limited_bits=int((hist * lengths).sum()), unlimited_bits=H.optimal_huffman_bits(hist),
                chunk_bits=chunk_bits, chunk_words=(chunk_bits + 31) // 32, max_chunk_words=int(((chunk_bits + 31) // 32).max()),
                straddlers=straddlers, max_thread_bits=int(np.add.reduceat(rb, np.arange(0, n, RPT)).max()),
                max_digits=int(ndigits(counts).max()))


# ---- synthetic run lists ------------------------------------------------------------------------------------------------
def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def fib_values(nvalues, sigma, seed):
    """value v occurs Fibonacci(v) times, every count 1: the unlimited Huffman code is a comb of depth nvalues - 1"""
    vals = np.repeat(np.arange(nvalues), _fib(nvalues))
    np.random.default_rng(seed).shuffle(vals)
    return np.ones(len(vals), np.int64), vals.astype(np.int64), sigma


def fib_all_tokens(seed):
    """all 257 values and both digits coded (259 tokens): values 0..19 by Fibonacci numbers, the others 3 times each,
    counts 1..4 so that RUNA and RUNB occur"""
    freq = np.full(257, 3, np.int64)
    freq[:20] = _fib(22)[2:]
    vals = np.repeat(np.arange(257), freq)
    r = np.random.default_rng(seed)
    r.shuffle(vals)
    return r.integers(1, 5, len(vals)).astype(np.int64), vals.astype(np.int64), 257


def long_chunk(seed, nruns=60000 + 3, sigma=257):
    """chunk 1 of K = 1024 runs is all counts of 31 digits (2^31 .. 2^32 - 1), the only digits of the record, under
    uniform values: several LDS windows; the chunks before and behind it are short"""
    r = np.random.default_rng(seed)
    counts = np.ones(nruns, np.int64)
    counts[1024:2048] = r.integers(1 << 31, 1 << 32, 1024)
    counts[1024], counts[2047] = 1 << 31, U32_MAX
    return counts, r.integers(0, sigma, nruns).astype(np.int64), sigma


def every_digit_count(seed, sigma=7, cheap=6000):
    """counts 2^k - 1, 2^k, 2^k + 1 for k = 1..31 and 2^32 - 1 (0..31 digits), spread among cheap runs"""
    r = np.random.default_rng(seed)
    special = sorted({c for k in range(1, 32) for c in ((1 << k) - 1, 1 << k, (1 << k) + 1)} | {1, U32_MAX})
    counts = r.integers(1, 4, cheap).astype(np.int64)
    at = r.choice(cheap, len(special), replace=False)
    counts[at] = special
    return counts, r.integers(0, sigma, cheap).astype(np.int64), sigma


def rare_digit(seed, which, sigma=17, nruns=400000):
    """RUNA (which = 0) or RUNB (1) occurs only in the 31 digits of 4 consecutive runs (one thread's) among values
    with a geometric histogram: the digit gets the longest code, and those threads the longest bit strings"""
    r = np.random.default_rng(seed)
    vals = np.minimum(r.geometric(0.5, nruns) - 1, sigma - 1).astype(np.int64)
    counts = np.ones(nruns, np.int64)
    other = 3 if which == 0 else 2          # 3 = one RUNB, 2 = one RUNA: the other digit is common
    counts[r.random(nruns) < 0.3] = other
    counts[5000:5004] = (1 << 31) if which == 0 else U32_MAX
    return counts, vals, sigma


def single_token(nruns, sigma):
    return np.ones(nruns, np.int64), np.zeros(nruns, np.int64), sigma


def two_tokens(seed, nruns=5000, sigma=2):
    r = np.random.default_rng(seed)
    return np.ones(nruns, np.int64), (r.random(nruns) < 0.2).astype(np.int64), sigma


def mild(seed, nruns, sigma, escapes=True):
    """text-like counts with a sprinkling of what the packed formats escape (>= 5, >= 15, >= 127)"""
    r = np.random.default_rng(seed)
    counts = r.integers(1, 5, nruns).astype(np.int64)
    if escapes:
        m = r.random(nruns)
        counts[m < 0.03] = r.integers(5, 15, int((m < 0.03).sum()))
        counts[m < 0.015] = r.integers(15, 127, int((m < 0.015).sum()))
        counts[m < 0.005] = r.integers(127, 100000, int((m < 0.005).sum()))
    vals = np.minimum(r.geometric(0.35, nruns) - 1, sigma - 1).astype(np.int64)
    return counts, vals, sigma


def random_u32_counts(seed, nruns=5000, sigma=6):
    r = np.random.default_rng(seed)
    return r.integers(1, 1 << 32, nruns).astype(np.int64), r.integers(0, sigma, nruns).astype(np.int64), sigma


# ---- single mutations of a body -------------------------------------------------------------------------------------------
def body_layout(body):
    K, nchunks, nsyms, lmax = struct.unpack_from("<4I", body, 0)
    doff = 16 + ((nsyms + 15) & ~15)
    poff = doff + ((4 * nchunks + 15) & ~15)
    return dict(K=K, nchunks=nchunks, nsyms=nsyms, lmax=lmax, doff=doff, poff=poff)


def mutants(body, seed, nflips=60, ndir=30, nlen=24, nhead=12):
    """[(what, bytes)]: seeded single mutations of a well-formed body -- a flipped payload bit; a directory entry moved
    by +-1..33 bits (every other one with the opposite change to its neighbour, so that short moves keep the word sum);
    a length-table entry raised or lowered by one; K, nchunks or L_max changed to another legal-looking value"""
    r = np.random.default_rng(seed)
    L = body_layout(body)
    out = []

    def put32(b, off, val):
        struct.pack_into("<I", b, off, val & 0xFFFFFFFF)

    def get32(b, off):
        return struct.unpack_from("<I", b, off)[0]
    npay = len(body) - L["poff"]
    for _ in range(nflips):
        bit = int(r.integers(0, 8 * npay))
        b = bytearray(body)
        b[L["poff"] + bit // 8] ^= 1 << (bit % 8)
        out.append(("payload bit %d" % bit, bytes(b)))
    for i in range(ndir):
        k = int(r.integers(0, L["nchunks"]))
        d = int(r.integers(1, 34)) * (1 if r.random() < 0.5 else -1)
        b = bytearray(body)
        off = L["doff"] + 4 * k
        put32(b, off, get32(b, off) + d)
        what = "directory[%d] %+d" % (k, d)
        if i % 2 and L["nchunks"] > 1:
            nb = off + 4 if k + 1 < L["nchunks"] else off - 4
            put32(b, nb, get32(b, nb) - d)
            what += ", neighbour %+d" % -d
        out.append((what, bytes(b)))
    for _ in range(nlen):
        s = int(r.integers(0, L["nsyms"]))
        d = 1 if r.random() < 0.5 else -1
        b = bytearray(body)
        b[16 + s] = (b[16 + s] + d) & 0xFF
        out.append(("length[%d] %+d" % (s, d), bytes(b)))
    for i in range(nhead):
        b = bytearray(body)
        field = i % 3
        if field == 0:
            k2 = 1 << int(r.integers(0, 21))
            put32(b, 0, k2)
            what = "K = %d" % k2
        elif field == 1:
            d = int(r.integers(1, 3)) * (1 if r.random() < 0.5 else -1)
            put32(b, 4, L["nchunks"] + d)
            what = "nchunks %+d" % d
        else:
            l2 = int(r.integers(1, 13))
            put32(b, 12, l2)
            what = "L_max = %d" % l2
        out.append((what, bytes(b)))
    return [(what, b) for what, b in out if b != bytes(body)]


def verdict(body, nruns, sigma):
    """the restatement's: None for Malformed, else (counts, vals)"""
    try:
        return H.read_body(body, nruns, sigma)
    except H.Malformed:
        return None
