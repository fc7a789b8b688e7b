"""Exported FM-indexes that no build writes: the base indexes, the patterns and the damage families shared by
tests/test_fm_wire_ref.py (the model alone, no GPU) and tests/test_gpu_fm_import_foreign.py (the device against the model).
Everything here is made from tests/fm_wire_ref.py's builder and is deterministic: both tests see the same strings.

Bases: four texts -- ACGTN at n = 1343 (N = 1344 = 3 * 448: the last rank line is empty) and n = 1344, six letters at
n = 1499 (no pair vectors), random bytes at n = 1000 (253 byte values: three are kept out so that a byte without a code
exists) -- each built full, sampled at rates 4 and 32, and with text samples at rate 8 (tc_fm_build_self; behind a full
suffix array on two texts, behind one sampled at 4 on the other two).

A damage is placed on a line, byte or word that the undamaged index READS for the patterns below (WireIndex.reads), so it
is reached.  Families (the issue's table): V1 payload bits permuted inside a line; V2 a line's ones-before word; V3 a
line all ones / all zeros / a bit at the primary row / bits behind row N; V4 the same on pair vectors and on the
byte-vector line the pair table is made from; V5 L bytes; V6 marks bits and samples; V7 text samples permuted; V8
suffix-array words; V9 header (primary row, counts); VR 64 seeded random damages of a few bytes."""
import functools
import random

import numpy as np

import fm_wire_ref as W

TEXTS = ("acgtn1343", "acgtn1344", "six1499", "bytes1000")
BUILDS = ("full", "s4", "s32", "self")
ABSENT = (0x5A, 0xEE, 0xFF)          # 'Z' and two more: in no text


@functools.lru_cache(maxsize=None)
def text_of(name):
    rng = random.Random("text " + name)
    if name.startswith("acgtn"):
        return bytes(rng.choice(b"ACGTN") for _ in range(int(name[5:])))
    if name.startswith("six"):
        return bytes(rng.choice(b"ACGTNU") for _ in range(int(name[3:])))
    alphabet = [b for b in range(256) if b not in ABSENT]
    return bytes(rng.choice(alphabet) for _ in range(int(name[5:])))


def rates_of(text_name, build):
    """(sa_rate, text_rate) of a build"""
    if build == "self":
        return (1, 8) if text_name in ("acgtn1343", "bytes1000") else (4, 8)
    return {"full": (1, 0), "s4": (4, 0), "s32": (32, 0)}[build]


@functools.lru_cache(maxsize=None)
def base_wire(text_name, build):
    sa_rate, text_rate = rates_of(text_name, build)
    return W.build_wire(text_of(text_name), sa_rate=sa_rate, text_rate=text_rate)


@functools.lru_cache(maxsize=None)
def patterns(text_name):
    """-> (pats, mm_pats, mm2_pats): the batch of count / locate / factorize; the (shorter) batch of the search with
    mismatches at k = 1; the part of it that also runs at k = 2 (the enumeration's cost grows with sigma^k)"""
    t = text_of(text_name)
    n = len(t)
    rng = random.Random("patterns " + text_name)
    small = len(set(t)) <= 6
    singles = [bytes([b]) for b in (sorted(set(t)) + [ABSENT[0]] if small else range(256))]

    def sub(ln):
        a = rng.randrange(n - ln + 1)
        return t[a:a + ln]

    def changed(p):
        i = rng.randrange(len(p))
        return p[:i] + bytes([t[rng.randrange(n)]]) + p[i + 1:]

    def foreign(p):
        i = rng.randrange(len(p))
        return p[:i] + bytes([ABSENT[1]]) + p[i + 1:]
    subs = [sub(ln) for ln in (2, 2, 3, 3, 5, 8, 13, 21, 40, 100, 300)]
    pats = singles + subs + [changed(p) for p in subs] + [foreign(p) for p in subs[2:6]] + [b"", t, t + t[:50]]
    short = [sub(ln) for ln in (2, 3, 4, 7, 12)]
    mm = (singles if small else singles[:4] + [bytes([ABSENT[2]])]) + short + [changed(p) for p in short] + [foreign(short[3]), b""]
    mm2 = mm if small else mm[:5] + [changed(short[1])]
    return pats, mm, mm2


def extract_queries(text_name):
    """(starts, lens), starts 1-based: the whole text, single bytes at both ends, ranges inside and across the rate-8
    segments, an empty range"""
    n = len(text_of(text_name))
    q = [(1, n), (1, 1), (n, 1), (5, 20), (8, 1), (9, 16), (10, 6), (n + 1, 0), (700, 300), (n - 6, 7), (17, 0)]
    return [a for a, _ in q], [l for _, l in q]


# ---------------------------------------------------------------------------------------------------------------- answers
def answers(ix, text_name):
    """every query of the model on one index: {name: answer or MALFORMED}"""
    pats, mm, mm2 = patterns(text_name)
    out = {"count": ix.count(pats), "count_mm1": ix.count_mm(mm, 1), "count_mm2": ix.count_mm(mm2, 2)}
    if ix.sa_rate:
        out["locate"] = ix.locate(pats)
        out["locate_mm1"] = ix.locate_mm(mm, 1)
        out["locate_mm2"] = ix.locate_mm(mm2, 2)
        out["factorize"] = ix.factorize(pats)
        out["factor_total"] = sum(len(ix._factor_rows(p)) for p in pats)
    if ix.text_rate:
        out["extract"] = ix.extract(*extract_queries(text_name))
    return out


@functools.lru_cache(maxsize=None)
def base_index(text_name, build):
    """the undamaged index with its answers computed (so that .reads holds what the queries read)"""
    ix = W.WireIndex(base_wire(text_name, build))
    ix.base_answers = answers(ix, text_name)
    return ix


# ---------------------------------------------------------------------------------------------------------------- damages
def part_of(wire, name):
    """(offset, bytes) of a part"""
    for nm, o, nb in W.header_layout(W.Header(wire))[0]:
        if nm == name:
            return o, nb
    raise KeyError(name)


def _u64(b, off):
    return int.from_bytes(b[off:off + 8], "little")


def _put(b, off, v, size):
    b[off:off + size] = int(v & ((1 << (8 * size)) - 1)).to_bytes(size, "little")


def line_off(wire, vec, at):
    """byte offset of line `at` (= v * lines + line) of a vector part"""
    return part_of(wire, vec)[0] + 64 * at


def set_head(wire, vec, at, value):
    b = bytearray(wire)
    _put(b, line_off(wire, vec, at), value, 8)
    return bytes(b)


def set_payload(wire, vec, at, bits):
    b = bytearray(wire)
    _put(b, line_off(wire, vec, at) + 8, bits, 56)
    return bytes(b)


def payload(wire, vec, at):
    o = line_off(wire, vec, at) + 8
    return int.from_bytes(wire[o:o + 56], "little")


def rows_in_line(N, lines, at):
    """how many of the 448 rows of a line lie below N"""
    line = at % lines
    return max(0, min(W.LINE_BITS, N - line * W.LINE_BITS))


def set_bytes(wire, part, index, value, size):
    b = bytearray(wire)
    _put(b, part_of(wire, part)[0] + index * size, value, size)
    return bytes(b)


def _read_lines(ix, vec, rng, count, pred=lambda at: True):
    got = sorted(at for at in ix.reads.get(vec, ()) if pred(at))
    rng.shuffle(got)
    return got[:count]


def heads_for(ix, wire, vec, at):
    """the V2 values of one line: 0, N, 2^32 - 1, 2^63, one less than the predecessor's, and one that makes s > e (or e > N)
    behind it"""
    own = _u64(wire, line_off(wire, vec, at))
    prev = _u64(wire, line_off(wire, vec, at - 1)) if at % ix.lines else 0
    return [("0", 0), ("N", ix.N), ("2^32-1", (1 << 32) - 1), ("2^63", 1 << 63), ("prev-1", (prev - 1) & W.M64), ("own+2000", own + 2000),
            ("own+1", own + 1)]


def _line_damages(ix, wire, vec, at):
    """V3 on one line: [(name, wire)]"""
    N, lines = ix.N, ix.lines
    live = rows_in_line(N, lines, at)
    out = [("ones", set_payload(wire, vec, at, (1 << live) - 1)), ("zeros", set_payload(wire, vec, at, 0))]
    if at % lines == ix.primary // W.LINE_BITS:
        out.append(("primary", set_payload(wire, vec, at, payload(wire, vec, at) | 1 << (ix.primary % W.LINE_BITS))))
    if at % lines == lines - 1 and live < W.LINE_BITS:
        out.append(("behindN", set_payload(wire, vec, at, payload(wire, vec, at) | ((1 << W.LINE_BITS) - (1 << live)))))
    return out


def _permuted(wire, ix, vec, at, rng):
    """V1: the payload bits of the line's live rows permuted: the line's count, and so every header, stays true"""
    live = rows_in_line(ix.N, ix.lines, at)
    bits = payload(wire, vec, at)
    order = list(range(live))
    rng.shuffle(order)
    new = 0
    for i, j in enumerate(order):
        new |= ((bits >> j) & 1) << i
    return set_payload(wire, vec, at, new | (bits >> live << live))


def family(name, text_name, build):
    """[(case name, damaged wire)] of one family on one base index ([] where the base lacks the part)"""
    wire = base_wire(text_name, build)
    ix = base_index(text_name, build)
    rng = random.Random("%s %s %s" % (name, text_name, build))
    N, lines = ix.N, ix.lines
    out = []
    if name == "V1":
        for at in _read_lines(ix, "bits", rng, 3, lambda at: payload(wire, "bits", at) != 0):
            out.append(("bits[%d]" % at, _permuted(wire, ix, "bits", at, rng)))
    elif name == "V2":
        for at in _read_lines(ix, "bits", rng, 1):
            out += [("bits[%d].head=%s" % (at, nm), set_head(wire, "bits", at, v)) for nm, v in heads_for(ix, wire, "bits", at)]
    elif name == "V3":
        picked = _read_lines(ix, "bits", rng, 2)
        picked += _read_lines(ix, "bits", rng, 1, lambda at: at % lines == ix.primary // W.LINE_BITS)
        picked += _read_lines(ix, "bits", rng, 1, lambda at: at % lines == lines - 1)
        for at in dict.fromkeys(picked):
            out += [("bits[%d].%s" % (at, nm), w) for nm, w in _line_damages(ix, wire, "bits", at)]
    elif name == "V4":
        if not ix.pairs:
            return []
        for at in _read_lines(ix, "bits2", rng, 1):
            out += [("bits2[%d].head=%s" % (at, nm), set_head(wire, "bits2", at, v)) for nm, v in heads_for(ix, wire, "bits2", at)]
        picked = _read_lines(ix, "bits2", rng, 1) + _read_lines(ix, "bits2", rng, 1, lambda at: at % lines == lines - 1)
        for at in dict.fromkeys(picked):
            out += [("bits2[%d].%s" % (at, nm), w) for nm, w in _line_damages(ix, wire, "bits2", at)]
        # the byte-vector line fm_c2_kernel reads for C2[a, b]: line C[b] / 448 of vector a
        a, b = rng.randrange(ix.sigma), rng.randrange(1, ix.sigma)
        at = a * lines + ix.tab[256 + b] // W.LINE_BITS
        out += [("c2 bits[%d].head=%s" % (at, nm), set_head(wire, "bits", at, v)) for nm, v in heads_for(ix, wire, "bits", at)[:5]]
        out += [("c2 bits[%d].%s" % (at, nm), w) for nm, w in _line_damages(ix, wire, "bits", at)[:2]]
    elif name == "V5":
        if not ix.sa_rate or (ix.sa_rate == 1 and not ix.text_rate):
            return []                                   # L is read by the walks only
        rows = sorted(r for r in ix.reads["L"] if r != ix.primary)
        rng.shuffle(rows)
        for r in rows[:3]:
            out.append(("L[%d]=absent" % r, set_bytes(wire, "L", r, ABSENT[0], 1)))
        present = sorted(set(text_of(text_name)))
        for r in rows[3:7]:
            other = rng.choice([b for b in present if b != ix.part["L"][r]])
            out.append(("L[%d]=other" % r, set_bytes(wire, "L", r, other, 1)))
    elif name == "V6":
        if ix.sa_rate <= 1:
            return []
        rate = ix.sa_rate
        marks = [payload(wire, "marks", l) for l in range(lines)]
        marked = [r for r in range(N) if (marks[r // W.LINE_BITS] >> (r % W.LINE_BITS)) & 1]
        unmarked = [r for r in range(N) if not (marks[r // W.LINE_BITS] >> (r % W.LINE_BITS)) & 1]
        for _ in range(3):                              # a marks bit moved, the popcount kept: some walk finds no mark in time
            src, dst = rng.choice(marked[1:]), rng.choice(unmarked)
            w = set_payload(wire, "marks", src // W.LINE_BITS, payload(wire, "marks", src // W.LINE_BITS) & ~(1 << (src % W.LINE_BITS)))
            w = set_payload(w, "marks", dst // W.LINE_BITS, payload(w, "marks", dst // W.LINE_BITS) | 1 << (dst % W.LINE_BITS))
            out.append(("mark %d->%d" % (src, dst), w))
        src = rng.choice(marked[1:])                    # ... moved to its neighbour row inside one word: the ranks stay true
        dst = src + 1 if (src + 1) % 64 and src + 1 in set(unmarked) else src - 1
        if dst in set(unmarked) and dst // 64 == src // 64:
            w = set_payload(wire, "marks", src // W.LINE_BITS,
                            (payload(wire, "marks", src // W.LINE_BITS) & ~(1 << (src % W.LINE_BITS))) | 1 << (dst % W.LINE_BITS))
            out.append(("mark %d->%d (neighbour)" % (src, dst), w))
        used = sorted(ix.reads["samples"])
        rng.shuffle(used)
        i, j, k, l = (used * 4)[:4]
        out.append(("samples[%d]+=1" % i, set_bytes(wire, "samples", i, ix.word("samples", i) + 1, 4)))
        out.append(("samples[%d]>=N" % j, set_bytes(wire, "samples", j, (N + rate - 1) // rate * rate, 4)))
        out.append(("samples[%d]=0xFFFFFFFF" % j, set_bytes(wire, "samples", j, 0xFFFFFFFF, 4)))
        out.append(("samples[%d]=samples[%d]" % (k, l), set_bytes(wire, "samples", k, ix.word("samples", l), 4)))
        out.append(("samples[%d]=0" % k, set_bytes(wire, "samples", k, 0, 4)))
    elif name == "V7":
        if not ix.text_rate:
            return []
        isa = [ix.word("isa", i) for i in range(ix.nisa)]
        for kind in ("swap", "rotate", "shuffle"):
            new = isa[:]
            if kind == "swap":
                i, j = rng.sample(range(1, ix.nisa), 2)
                new[i], new[j] = new[j], new[i]
            elif kind == "rotate":
                new = isa[:1] + isa[2:] + isa[1:2]
            else:
                tail = isa[1:]
                rng.shuffle(tail)
                new = isa[:1] + tail
            o, nb = part_of(wire, "isa")
            b = bytearray(wire)
            b[o:o + nb] = np.array(new, np.uint32).tobytes()
            out.append(("isa " + kind, bytes(b)))
    elif name == "V8":
        if ix.sa_rate != 1:
            return []
        rows = sorted(ix.reads["sa"])
        rng.shuffle(rows)
        for r, v in zip(rows, (0xFFFFFFFF, 0, N, 0x80000000, 12345678)):
            out.append(("sa[%d]=%#x" % (r, v), set_bytes(wire, "sa", r, v, 4)))
        b = bytearray(wire)
        o, nb = part_of(wire, "sa")
        b[o:o + nb] = bytes(rng.randrange(256) for _ in range(nb))
        out.append(("sa random", bytes(b)))
    elif name == "V9":
        for row in (1 if ix.primary != 1 else 2, N - 1 if ix.primary != N - 1 else N - 2, rng.randrange(1, N)):
            b = bytearray(wire)
            _put(b, W.OFF_PRIMARY, row, 8)
            out.append(("primary=%d" % row, bytes(b)))
        present = sorted(set(text_of(text_name)))
        for _ in range(2):                              # two present bytes trade counts: the total and the code table stay
            x, y = rng.sample(present, 2)
            b = bytearray(wire)
            cx, cy = ix.h.counts[x], ix.h.counts[y]
            _put(b, W.OFF_COUNTS + 4 * x, cy, 4)
            _put(b, W.OFF_COUNTS + 4 * y, cx, 4)
            if cx != cy:
                out.append(("counts %d<->%d" % (x, y), bytes(b)))
    else:
        raise KeyError(name)
    return [(n_, w) for n_, w in out if w != wire]


FAMILIES = ("V1", "V2", "V3", "V4", "V5", "V6", "V7", "V8", "V9")
# which bases a family runs on: every family meets every text and every build that has its part at least once, and the whole
# stays a few seconds per test
FAMILY_BASES = {
    "V1": [("acgtn1343", "full"), ("six1499", "s4"), ("bytes1000", "self"), ("acgtn1344", "s32")],
    "V2": [("acgtn1343", "s4"), ("acgtn1344", "full"), ("six1499", "self"), ("bytes1000", "s32"), ("six1499", "full")],
    "V3": [("acgtn1343", "self"), ("acgtn1344", "s4"), ("six1499", "s32"), ("bytes1000", "full")],
    "V4": [("acgtn1343", "full"), ("acgtn1344", "self"), ("acgtn1343", "s32"), ("acgtn1344", "s4")],
    "V5": [("acgtn1343", "s4"), ("acgtn1344", "self"), ("six1499", "s32"), ("bytes1000", "self"), ("bytes1000", "s4")],
    "V6": [("acgtn1343", "s32"), ("acgtn1344", "self"), ("six1499", "s4"), ("bytes1000", "s32"), ("six1499", "self")],
    "V7": [("acgtn1343", "self"), ("acgtn1344", "self"), ("six1499", "self"), ("bytes1000", "self")],
    "V8": [("acgtn1343", "full"), ("acgtn1343", "self"), ("six1499", "full"), ("bytes1000", "self")],
    "V9": [("acgtn1344", "full"), ("acgtn1343", "s4"), ("six1499", "self"), ("bytes1000", "s32"), ("acgtn1343", "self")],
}

VR_CASES = 64
VR_CHUNKS = 8


def random_case(i):
    """VR case i of 64: -> (text name, build, case name, wire): a few bytes of every part of one base index replaced by
    random ones -- one to three per part, the header's scalar words left alone (their rules are family V9's and
    test_gpu_fm_sampled's), in marks two bytes exchanged instead (a random byte there changes the popcount, which is the one
    thing the import checks of it)"""
    rng = random.Random("VR %d" % i)
    text_name, build = TEXTS[i % 4], BUILDS[(i // 4) % 4]
    wire = base_wire(text_name, build)
    b = bytearray(wire)
    notes = []
    for name, o, nb in W.header_layout(W.Header(wire))[0]:
        if rng.random() < 0.5:
            continue
        for _ in range(rng.randint(1, 3)):
            at = rng.randrange(nb)
            if name == "marks":
                at2 = at // 64 * 64 + rng.randrange(8, 64)
                at = at // 64 * 64 + rng.randrange(8, 64)
                b[o + at], b[o + at2] = b[o + at2], b[o + at]
            elif name in ("samples", "isa", "sa") and at % 4 >= 2 and rng.random() < 0.75:
                b[o + at - 2] = rng.randrange(256)      # (mostly the low half of a word: the high half is nearly always >= N)
            else:
                b[o + at] = rng.randrange(256)
            notes.append("%s+%d" % (name, at))
    if bytes(b) == wire:
        o, nb = part_of(wire, "bits")
        b[o + rng.randrange(nb)] ^= 1 << rng.randrange(8)
        notes.append("bits")
    return text_name, build, "VR%d %s" % (i, " ".join(notes)), bytes(b)
