"""The exported FM-index (the TCFMI02 byte string of tc_fm_export_dev / tc_fm_import_dev) and every query on it, in numpy
and Python integers: no GPU, no library.  It follows FmWire and fm_wire_layout of csrc/tc_fm_host.hpp for the format and
the rules written above each kernel for the queries, and it is defined on the CONTENTS of the string, not on a text: a
string no build writes -- wrong rank counts, lines with two codes per row, samples at the wrong rows -- still has exactly
one answer per query here, the exact numbers or MALFORMED, and that is what the device must answer too
(tests/test_gpu_fm_import_foreign.py).

The string: a header of 1600 bytes (magic, n, N, primary, lines, bytes, sigma_bytes, with_locate | text_rate << 8, with_pairs,
sa_rate, counts[256], sym_of_code[256]), then the parts, each at a multiple of 256 bytes:
  bits    [sigma][lines][8] u64: one rank vector per present byte value, 64-byte lines = {ones before the line, 448 payload
          bits}, lines = N / 448 + 1; the primary row has no bit in any of them
  bits2   [sigma^2][lines][8], the pair vectors (with_pairs)
  L       N bytes (+ 16 bytes of slack), behind a locate part only
  marks   [lines][8] and samples [n / sa_rate + 1] u32 (a sampled index), or sa [N] u32 (a full one)
  isa     [n / text_rate + 1] u32 (text samples)

Every read a query makes of a part goes through an accessor of WireIndex that asserts the index lies inside the part: a
written rule that allowed a read outside a part would fail here, on the CPU, where it is an AssertionError and not a fault.

tc_fm_unfactorize and the LCP part (never imported) are out of scope."""
import numpy as np

MALFORMED = "MALFORMED"
OK = "OK"

MAGIC = b"TCFMI02\0"
HDR_BYTES = 1600            # sizeof(FmWire)
LINE_BITS = 448
PAIR_SIGMA = 5
MAX_N = 0x7ffffff0
MAX_RATE = 4096
MAX_K = 3                   # TC_FM_MAX_MISMATCH
NONE = 0xFFFFFFFF
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1

OFF_N, OFF_NN, OFF_PRIMARY, OFF_LINES, OFF_BYTES = 8, 16, 24, 32, 40
OFF_SIGMA, OFF_WITH_LOCATE, OFF_PAIRS, OFF_RATE, OFF_COUNTS, OFF_SYMS = 48, 52, 56, 60, 64, 1088


def align(v):
    return (v + 255) & ~255


def rate_ok(r):
    return 1 <= r <= MAX_RATE and (r & (r - 1)) == 0


def make_tab(counts):
    """fm_make_tab: [0..255] code of byte (NONE absent), [256..511] C[code], [512..767] count[code]; -> (tab, sigma)"""
    tab = [0] * 768
    sig, acc = 0, 1
    for b in range(256):
        tab[b] = NONE
        if counts[b]:
            tab[b] = sig
            tab[256 + sig] = acc
            tab[512 + sig] = int(counts[b])
            acc += int(counts[b])
            sig += 1
    return tab, sig


class Header:
    def __init__(self, wire):
        h = np.frombuffer(bytes(wire[:HDR_BYTES]), np.uint8)
        self.magic = h[:8].tobytes()
        self.n, self.N, self.primary, self.lines, self.bytes = (int(v) for v in h[8:48].view(np.uint64))
        self.sigma, self.with_locate, self.with_pairs, self.sa_rate = (int(v) for v in h[48:64].view(np.uint32))
        self.counts = [int(v) for v in h[OFF_COUNTS:OFF_COUNTS + 1024].view(np.uint32)]
        self.syms = [int(v) for v in h[OFF_SYMS:OFF_SYMS + 512].view(np.int16)]

    @property
    def locate(self):
        return (self.with_locate & 0xff) != 0

    @property
    def text_rate(self):
        return self.with_locate >> 8

    @property
    def sampled(self):
        return self.sa_rate > 1


def layout(n, N, lines, sigma, pairs, locate, sampled, nsamples, nisa):
    """fm_wire_layout: [(name, offset, bytes)] and the total"""
    parts, o = [], align(HDR_BYTES)

    def add(name, nbytes, reserved):
        nonlocal o
        parts.append((name, o, nbytes))
        o += align(reserved)
    if n:
        bb = sigma * lines * 64
        add("bits", bb, bb)
        if pairs:
            add("bits2", bb * sigma, bb * sigma)
        if locate:
            add("L", N, N + 16)
            if sampled:
                add("marks", lines * 64, lines * 64)
                add("samples", 4 * nsamples, 4 * nsamples)
            else:
                add("sa", 4 * N, 4 * N)
        if nisa:
            add("isa", 4 * nisa, 4 * nisa)
    return parts, o


def header_layout(h):
    nsamples = h.n // h.sa_rate + 1 if h.sampled else 0
    nisa = h.n // h.text_rate + 1 if h.text_rate else 0
    return layout(h.n, h.N, h.lines, h.sigma, h.with_pairs != 0, h.locate, h.sampled, nsamples, nisa)


def header_verdict(wire):
    """the refusals fm_import_device makes before it reads a part: OK or MALFORMED"""
    if len(wire) < HDR_BYTES:
        raise ValueError("shorter than a header: TC_ERR_ARG, not a verdict")
    h = Header(wire)
    if h.magic != MAGIC:
        return MALFORMED
    if h.bytes > len(wire) or h.N != (h.n + 1 if h.n else 0) or h.n > MAX_N or h.sigma > 256:
        return MALFORMED
    if h.n and h.lines != h.N // LINE_BITS + 1:
        return MALFORMED
    total = present = 0
    codes_ok = True
    for b in range(256):
        total += h.counts[b]
        if h.counts[b]:
            codes_ok = codes_ok and present < h.sigma and h.syms[present] == b
            present += 1
    if h.n and (h.primary == 0 or h.primary >= h.N or total != h.n or present != h.sigma or not codes_ok):
        return MALFORMED
    if h.with_pairs > 1 or (h.with_pairs and (h.sigma > PAIR_SIGMA or h.n < 2)):
        return MALFORMED
    if h.sampled and (not rate_ok(h.sa_rate) or not h.locate or not h.n):
        return MALFORMED
    if h.text_rate and (not rate_ok(h.text_rate) or (h.with_locate & 0xff) != 1 or not h.n):
        return MALFORMED
    if h.n and header_layout(h)[1] != h.bytes:
        return MALFORMED
    return OK


def import_verdict(wire):
    """exactly the refusals fm_import_device makes: the header rules, the size, marks popcount != nsamples, a text sample
    >= N or isa[0] != primary"""
    if header_verdict(wire) == MALFORMED:
        return MALFORMED
    h = Header(wire)
    if not h.n:
        return OK
    w = np.frombuffer(bytes(wire), np.uint8)
    for name, o, nb in header_layout(h)[0]:
        if name == "marks":
            words = w[o:o + nb].view(np.uint64).reshape(-1, 8)[:, 1:]
            if sum(int(v).bit_count() for v in words.ravel()) != h.n // h.sa_rate + 1:
                return MALFORMED
        if name == "isa":
            isa = w[o:o + nb].view(np.uint32)
            if int(isa.max()) >= h.N or int(isa[0]) != h.primary:
                return MALFORMED
    return OK


# ---------------------------------------------------------------------------------------------------------------- the builder
def suffix_array(text):
    """rows of text + '$', the empty suffix first (Python's bytes order puts a proper prefix first)"""
    t = bytes(text)
    return sorted(range(len(t) + 1), key=lambda i: t[i:])


def _pack_lines(rows_of_vec, nvec, lines):
    """[nvec][lines][8] u64 from the set rows of every vector: payload bits, then word 0 = ones before the line"""
    out = np.zeros((nvec, lines, 8), np.uint64)
    for v, rows in rows_of_vec.items():
        for j in rows:
            out[v, j // LINE_BITS, 1 + (j % LINE_BITS) // 64] |= np.uint64(1 << (j % 64))
    for v in range(nvec):
        run = 0
        for l in range(lines):
            out[v, l, 0] = run
            run += sum(int(x).bit_count() for x in out[v, l, 1:])
    return out


def build_wire(text, sa_rate=1, text_rate=0, with_locate=True, pairs=None):
    """the string tc_fm_export_dev writes for the index of `text` (n >= 1) built with these rates; pairs=None: where the
    library keeps them (at most 5 byte values, n >= 2)"""
    t = bytes(text)
    n = len(t)
    N = n + 1
    sa = suffix_array(t)
    counts = [0] * 256
    for b in t:
        counts[b] += 1
    tab, sigma = make_tab(counts)
    lines = N // LINE_BITS + 1
    primary = sa.index(0)
    if pairs is None:
        pairs = sigma <= PAIR_SIGMA and n >= 2
    L = bytearray(N)
    rows, rows2 = {}, {}
    for j, p in enumerate(sa):
        if p == 0:
            continue                                    # the primary row: no bit in any symbol vector, L = 0
        L[j] = t[p - 1]
        rows.setdefault(tab[t[p - 1]], []).append(j)
        if pairs and p >= 2:
            rows2.setdefault(tab[t[p - 2]] * sigma + tab[t[p - 1]], []).append(j)
    sampled = with_locate and sa_rate > 1
    text_rate = text_rate if with_locate else 0
    nsamples = n // sa_rate + 1 if sampled else 0
    nisa = n // text_rate + 1 if text_rate else 0
    parts, total = layout(n, N, lines, sigma, pairs, with_locate, sampled, nsamples, nisa)
    w = np.zeros(total, np.uint8)
    w[:8] = np.frombuffer(MAGIC, np.uint8)
    w[8:48] = np.array([n, N, primary, lines, total], np.uint64).view(np.uint8)
    w[48:64] = np.array([sigma, (1 | text_rate << 8) if with_locate else 0, int(pairs), sa_rate if sampled else 0],
                        np.uint32).view(np.uint8)
    w[OFF_COUNTS:OFF_COUNTS + 1024] = np.array(counts, np.uint32).view(np.uint8)
    syms = np.zeros(256, np.int16)
    for b in range(256):
        if counts[b]:
            syms[tab[b]] = b
    w[OFF_SYMS:OFF_SYMS + 512] = syms.view(np.uint8)
    for name, o, nb in parts:
        if name == "bits":
            data = _pack_lines(rows, sigma, lines)
        elif name == "bits2":
            data = _pack_lines(rows2, sigma * sigma, lines)
        elif name == "L":
            data = np.frombuffer(bytes(L), np.uint8)
        elif name == "marks":
            data = _pack_lines({0: [j for j, p in enumerate(sa) if p % sa_rate == 0]}, 1, lines)
        elif name == "samples":
            data = np.array([p for p in sa if p % sa_rate == 0], np.uint32)
        elif name == "sa":
            data = np.array(sa, np.uint32)
        else:
            isa = np.zeros(nisa, np.uint32)
            for j, p in enumerate(sa):
                if p % text_rate == 0:
                    isa[p // text_rate] = j
            data = isa
        w[o:o + nb] = np.ascontiguousarray(data).view(np.uint8).ravel()
    return w.tobytes()


# ------------------------------------------------------------------------------------------------------------------ the model
class WireIndex:
    """an imported index: the header and the parts of a string whose import_verdict is OK, and the queries on them"""

    def __init__(self, wire):
        assert import_verdict(wire) == OK
        self.h = h = Header(wire)
        assert h.n, "the empty index has no parts: out of scope"
        self.n, self.N, self.primary, self.lines, self.sigma = h.n, h.N, h.primary, h.lines, h.sigma
        self.pairs = h.with_pairs != 0
        self.sa_rate = h.sa_rate if h.sampled else (1 if h.locate else 0)
        self.text_rate = h.text_rate
        self.nsamples = h.n // h.sa_rate + 1 if h.sampled else 0
        self.nisa = h.n // h.text_rate + 1 if h.text_rate else 0
        w = np.frombuffer(bytes(wire), np.uint8)
        self.part = {name: w[o:o + nb] for name, o, nb in header_layout(h)[0]}
        self._vec = {k: self.part[k].view(np.uint64) for k in ("bits", "bits2", "marks") if k in self.part}
        self._u32 = {k: self.part[k].view(np.uint32) for k in ("samples", "sa", "isa") if k in self.part}
        self._lines = {}
        self.tab, sig = make_tab(h.counts)
        assert sig == self.sigma
        self.reads = {}                                # part -> set of the indexes read (lines, bytes, words)
        self._memo = {}                                 # (a query's deterministic sub-results, computed once)
        self.cuts = 0                                   # searches of count_one ended by an interval that is not merely empty
        self.tab2 = None
        if self.pairs:                                  # fm_c2_kernel
            self.tab2 = [0] * (PAIR_SIGMA * PAIR_SIGMA)
            for t in range(self.sigma * self.sigma):
                a, b = divmod(t, self.sigma)
                self.tab2[t] = (self.C(a) + self.occ64("bits", a, self.C(b))) & M32

    # ---- the guarded accessors: every read of a part
    def _note(self, part, i):
        self.reads.setdefault(part, set()).add(i)

    def line(self, vec, v, line):
        """(ones-before word, the 448 payload bits as an integer) of line `line` of vector v"""
        nvec = {"bits": self.sigma, "bits2": self.sigma * self.sigma, "marks": 1}[vec]
        assert vec in self._vec, "no part " + vec
        assert 0 <= v < nvec and 0 <= line < self.lines, "%s: vector %d line %d outside [%d][%d]" % (vec, v, line, nvec, self.lines)
        at = v * self.lines + line
        self._note(vec, at)
        got = self._lines.get((vec, at))
        if got is None:
            w = self._vec[vec][at * 8:at * 8 + 8]
            assert len(w) == 8
            got = (int(w[0]), int.from_bytes(w[1:].tobytes(), "little"))
            self._lines[(vec, at)] = got
        return got

    def L(self, row):
        assert 0 <= row < self.N, "L[%d] outside [%d]" % (row, self.N)
        self._note("L", row)
        return int(self.part["L"][row])

    def word(self, part, i):
        size = {"samples": self.nsamples, "sa": self.N, "isa": self.nisa}[part]
        assert part in self._u32, "no part " + part
        assert 0 <= i < size, "%s[%d] outside [%d]" % (part, i, size)
        self._note(part, i)
        return int(self._u32[part][i])

    def code(self, byte):
        assert 0 <= byte < 256
        return self.tab[byte]

    def C(self, c):
        assert 0 <= c < self.sigma, "table entry of code %d" % c
        return self.tab[256 + c]

    def cnt(self, c):
        assert 0 <= c < self.sigma
        return self.tab[512 + c]

    def C2(self, pr):
        assert self.pairs and 0 <= pr < self.sigma * self.sigma
        return self.tab2[pr]

    # ---- rank
    def occ64(self, vec, v, k):
        """fm_occ / fm_occ2: Occ(v, k) in 64-bit arithmetic"""
        head, bits = self.line(vec, v, k // LINE_BITS)
        return (head + (bits & ((1 << (k % LINE_BITS)) - 1)).bit_count()) & M64

    def occ32(self, vec, v, k):
        """fm_mm_occ2: the low half of the ones-before word, 32-bit sums"""
        head, bits = self.line(vec, v, k // LINE_BITS)
        return ((head & M32) + (bits & ((1 << (k % LINE_BITS)) - 1)).bit_count()) & M32

    def shape_ok(self, s, e):
        return 1 <= s <= e <= self.N

    # ---- count (fm_count_lane): -> (count, s, e), s = e = 0 for count 0
    def _no_interval(self, s, e):
        """the answer of a search whose interval is not of the shape 1 <= s <= e <= N: nothing; an interval that is not
        merely empty (s = e + 1 inside the index) is one that only the rule stops"""
        if not (s == e + 1 and 1 <= s <= self.N + 1):
            self.cuts += 1
        return 0, 0, 0

    def count_one(self, pat):
        s, e, q, first = 1, self.N, len(pat), True
        while q > 0:
            if not self.shape_ok(s, e):
                return self._no_interval(s, e)
            c = self.code(pat[q - 1])
            if c == NONE:
                break                                   # a byte without a code stops the loop
            if first:
                s, e, first = self.C(c) + 1, self.C(c) + self.cnt(c), False
                q -= 1
                continue
            if self.pairs and q >= 2:
                a = self.code(pat[q - 2])
                if a != NONE:
                    pr = a * self.sigma + c
                    o1, o2 = self.occ64("bits2", pr, s - 1), self.occ64("bits2", pr, e)
                    s, e = (self.C2(pr) + o1 + 1) & M64, (self.C2(pr) + o2) & M64
                    q -= 2
                    continue
            o1, o2 = self.occ64("bits", c, s - 1), self.occ64("bits", c, e)
            s, e = (self.C(c) + o1 + 1) & M64, (self.C(c) + o2) & M64
            q -= 1
        if first:
            return 0, 0, 0
        if not self.shape_ok(s, e):
            return self._no_interval(s, e)
        return e - s + 1, s, e

    def count(self, pats):
        return [self.count_one(p)[0] for p in pats]

    # ---- the walk of a sampled index (fm_locate_walk_body): row -> 1-based position, or None where it raises FM_ERR_WALK
    def walk(self, row):
        if ("walk", row) not in self._memo:
            self._memo[("walk", row)] = self._walk(row)
        return self._memo[("walk", row)]

    def _walk(self, row):
        bad = row >= self.N
        if bad:
            row = 0
        steps = pos = 0
        while True:
            byte = self.L(row)
            head, bits = self.line("marks", 0, row // LINE_BITS)
            off = row % LINE_BITS
            r = (head + (bits & ((1 << off) - 1)).bit_count()) & M64
            if (bits >> off) & 1:
                if r >= self.nsamples:
                    bad = True
                    break
                v = self.word("samples", r)
                pos = v + steps
                if v & (self.sa_rate - 1) or pos >= self.N:
                    bad = True
                break
            c = self.code(byte)
            if steps + 1 >= self.sa_rate or row == self.primary or c >= self.sigma:
                bad = True
                break
            nr = (self.C(c) + self.occ64("bits", c, row)) & M64
            if nr >= self.N:
                bad = True
                break
            row = nr
            steps += 1
        return None if bad else pos + 1

    def _positions(self, rows):
        """rows of hits -> positions: the suffix array's word + 1 on a full index, the walk on a sampled one (None: a walk
        raised the error)"""
        assert self.sa_rate, "no locate part"
        if self.sa_rate == 1:
            return [self.word("sa", r) + 1 for r in rows]
        return [self.walk(r) for r in rows]

    def locate(self, pats):
        """-> [positions] per pattern, rows in increasing order, or MALFORMED"""
        out = []
        for p in pats:
            cnt, s, e = self.count_one(p)
            out.append(self._positions(range(s - 1, e) if cnt else []))
        return MALFORMED if any(v is None for h in out for v in h) else out

    # ---- extract (fm_extract_plan_kernel + fm_extract_walk_kernel): starts 1-based; -> [bytes] or MALFORMED
    def extract(self, starts, lens):
        assert self.text_rate, "no text samples"
        lg = self.text_rate.bit_length() - 1
        n, bad_any, out = self.n, False, []
        for start, ln in zip(starts, lens):
            a = start - 1
            assert 0 <= a <= n and ln <= n - a, "a query outside the text is TC_ERR_ARG: not this model's"
            buf = bytearray(ln)
            e = a + ln
            for k in range(a >> lg, ((a + ln - 1) >> lg) + 1 if ln else 0):
                seg_lo, seg_hi = k << lg, (k + 1) << lg
                lo, anchor = max(a, seg_lo), min(seg_hi, n)
                top = min(e, anchor)
                bad, row = False, 0
                if anchor != n:
                    if k + 1 < self.nisa:
                        row = self.word("isa", k + 1)
                    else:
                        bad = True
                    if row >= self.N:
                        bad, row = True, 0
                if not bad and lo < anchor:
                    p = anchor - 1
                    while True:
                        if row == self.primary:
                            bad = True
                            break
                        byte = self.L(row)
                        c = self.code(byte)
                        if c >= self.sigma:
                            bad = True
                            break
                        if p < top:
                            buf[p - a] = byte
                        if p == lo:
                            break
                        nr = (self.C(c) + self.occ64("bits", c, row)) & M64
                        if nr >= self.N:
                            bad = True
                            break
                        row = nr
                        p -= 1
                bad_any = bad_any or bad
            out.append(bytes(buf))
        return MALFORMED if bad_any else out

    # ---- search with mismatches (fm_mm_kernel): -> [(row, distance)] in the enumeration's order
    def _mm_rows(self, pat, k):
        if ("mm", pat, k) not in self._memo:
            self._memo[("mm", pat, k)] = self._mm_enumerate(pat, k)
        return self._memo[("mm", pat, k)]

    def _mm_enumerate(self, pat, k):
        m, N, sigma = len(pat), self.N, self.sigma
        hits = []
        if m == 0 or m >= N:
            return hits
        k = min(k, MAX_K)
        q, s, e, alt, d = m, 1, N, 0, 0
        frames = []
        while True:
            pop = True
            if q == 0:
                hits.extend((r, d) for r in range(s - 1, e))
            else:
                own = self.code(pat[q - 1])
                c, nq = own, q - 1
                branch = d < k and alt < sigma
                if branch:
                    c = alt
                    alt += 1
                    if c == own:
                        continue
                if c != NONE:
                    if s == 1 and e == N:
                        s2, e2 = self.C(c) + 1, self.C(c) + self.cnt(c)
                    else:
                        vec, v, Cv = "bits", c, self.C(c)
                        if self.pairs and not branch and d == k and q >= 2:
                            a = self.code(pat[q - 2])
                            if a != NONE:
                                vec, v = "bits2", a * sigma + c
                                Cv, nq = self.C2(v), q - 2
                        assert self.shape_ok(s, e)
                        o1, o2 = self.occ32(vec, v, s - 1), self.occ32(vec, v, e)
                        s2, e2 = Cv + o1 + 1, Cv + o2
                    if s2 <= e2 <= N:
                        if branch:
                            frames.append((q, s, e, alt))
                            d += 1
                        q, s, e, alt = nq, s2, e2, 0
                        continue
                    if branch:
                        continue
            if pop:
                if d == 0:
                    break
                d -= 1
                q, s, e, alt = frames.pop()
        return hits

    def count_mm(self, pats, k):
        return [len(self._mm_rows(p, k)) for p in pats]

    def locate_mm(self, pats, k):
        """-> [(positions, distances)] per pattern in the enumeration's order, or MALFORMED"""
        out = []
        for p in pats:
            rows = self._mm_rows(p, k)
            out.append((self._positions([r for r, _ in rows]), [d for _, d in rows]))
        return MALFORMED if any(v is None for h, _ in out for v in h) else out

    # ---- factorize (fm_factor_kernel): -> [(row or byte, len)] of one pattern, in pattern order
    def _factor_rows(self, pat):
        N, sigma = self.N, self.sigma
        q, out = len(pat), []
        s = e = ln = 0
        while True:
            if q != 0:
                byte = pat[q - 1]
                c = self.code(byte)
                if ln == 0:
                    s2, e2 = 1, 0
                    if c != NONE:
                        s2, e2 = self.C(c) + 1, self.C(c) + self.cnt(c)
                    if s2 <= e2 <= N:
                        s, e, ln = s2, e2, 1
                    else:
                        out.append((byte, 0))
                    q -= 1
                    continue
                if c != NONE and ln < N - 1:
                    last = False
                    taken = False
                    assert self.shape_ok(s, e)
                    if self.pairs and q >= 2:
                        a = self.code(pat[q - 2])
                        if a != NONE:
                            pr = a * sigma + c
                            o1, o2 = self.occ32("bits2", pr, s - 1), self.occ32("bits2", pr, e)
                            s2, e2 = self.C2(pr) + o1 + 1, self.C2(pr) + o2
                            if s2 <= e2 <= N:
                                s, e, ln, q = s2, e2, ln + 2, q - 2
                                continue
                            last = True
                    o1, o2 = self.occ32("bits", c, s - 1), self.occ32("bits", c, e)
                    s2, e2 = self.C(c) + o1 + 1, self.C(c) + o2
                    if s2 <= e2 <= N:
                        s, e, ln, q = s2, e2, ln + 1, q - 1
                        taken = True
                    if taken and not last:
                        continue
            elif ln == 0:
                break
            out.append((s - 1, ln))
            ln = 0
        return out[::-1]

    def factorize(self, pats):
        """-> (fac_offs, fac_pos, fac_len) as lists, or MALFORMED"""
        offs, pos, lens = [0], [], []
        for p in pats:
            for a, l in self._factor_rows(p):
                pos.append(self._positions([a])[0] if l else a)
                lens.append(l)
            offs.append(len(pos))
        return MALFORMED if any(v is None for v in pos) else (offs, pos, lens)


# -------------------------------------------------------------------------------------------------- brute force over the text
def brute_count(text, pat):
    """what tc_fm_count answers: a byte the text lacks stops the loop, so the pattern's part behind the last such byte is
    what is counted (nothing at all when that part is empty)"""
    t, p = bytes(text), bytes(pat)
    present = set(t)
    cut = len(p)
    while cut > 0 and p[cut - 1] in present:
        cut -= 1
    p = p[cut:]
    return [i for i in range(len(t) - len(p) + 1) if t[i:i + len(p)] == p] if p else []
