"""tests/fm_wire_ref.py -- the exported FM-index and its queries in numpy -- checked here, without a GPU:
  - on well-formed strings the model agrees with brute force over the text for every query (mismatch_ref.py and
    factor_ref.py for those two);
  - every damaged string of tests/fm_foreign_cases.py goes through the model without one of its accessors' assertions:
    no written rule lets a read leave a part, on any content;
  - the damages discriminate, which is what keeps tests/test_gpu_fm_import_foreign.py from passing emptily: per family at
    least one case is answered (no MALFORMED) with an answer different from the undamaged index's; in V2, V4 and V6 at
    least one case ends MALFORMED or is cut to 0 by the rule of fm_count_kernel (an interval is stepped from only when
    1 <= s <= e <= N); of the 64 random damages at most half are refused at import."""
import numpy as np
import pytest

import factor_ref
import fm_foreign_cases as FC
import fm_wire_ref as W
import mismatch_ref

BASES = [(t, b) for t in FC.TEXTS for b in FC.BUILDS]


@pytest.mark.parametrize("text_name,build", BASES)
def test_model_agrees_with_brute_force(text_name, build):
    t = FC.text_of(text_name)
    ix = FC.base_index(text_name, build)
    got = ix.base_answers
    pats, mm, mm2 = FC.patterns(text_name)
    assert W.import_verdict(FC.base_wire(text_name, build)) == W.OK and ix.cuts == 0
    rank = factor_ref.suffix_ranks(t)
    hits = [sorted(W.brute_count(t, p), key=lambda i: rank[i]) for p in pats]      # a locate answers in suffix-array order
    assert got["count"] == [len(h) for h in hits]
    assert got["locate"] == [[i + 1 for i in h] for h in hits]
    for k, batch in ((1, mm), (2, mm2)):
        want = [mismatch_ref.hits(t, p, k) for p in batch]
        assert got["count_mm%d" % k] == [len(h) for h, _ in want]
        for (pos, dist), (wp, wd) in zip(got["locate_mm%d" % k], want):
            gp, gd = mismatch_ref.sorted_pairs(pos, dist)
            assert gp.tolist() == wp.tolist() and gd.tolist() == wd.tolist()
    offs, pos, lens = factor_ref.factorize(t, pats, rank)
    assert got["factorize"] == (offs.tolist(), pos.tolist(), lens.tolist()) and got["factor_total"] == len(pos)
    if ix.text_rate:
        starts, lens = FC.extract_queries(text_name)
        assert got["extract"] == [t[a - 1:a - 1 + l] for a, l in zip(starts, lens)]


def test_builder_layout_and_import_verdict():
    w = FC.base_wire("acgtn1343", "self")
    h = W.Header(w)
    assert (h.n, h.N, h.lines, h.sigma, h.with_pairs, h.sa_rate, h.text_rate) == (1343, 1344, 4, 5, 1, 0, 8)
    assert [nm for nm, _, _ in W.header_layout(h)[0]] == ["bits", "bits2", "L", "sa", "isa"] and all(o % 256 == 0 for _, o, _ in W.header_layout(h)[0])
    assert [nm for nm, _, _ in W.header_layout(W.Header(FC.base_wire("six1499", "self")))[0]] == ["bits", "L", "marks", "samples", "isa"]

    def put(off, value, size, base=w):
        b = bytearray(base)
        b[off:off + size] = int(value).to_bytes(size, "little")
        return bytes(b)
    refused = [put(0, 0x58, 1), put(5, 0x31, 1), put(W.OFF_BYTES, len(w) + 1, 8), put(W.OFF_BYTES, len(w) - 256, 8), put(W.OFF_NN, 1343, 8),
               put(W.OFF_LINES, 3, 8), put(W.OFF_PRIMARY, 0, 8), put(W.OFF_PRIMARY, 1344, 8), put(W.OFF_SIGMA, 4, 4),
               put(W.OFF_COUNTS + 4 * 65, h.counts[65] + 1, 4), put(W.OFF_SYMS, 66, 2), put(W.OFF_PAIRS, 2, 4), put(W.OFF_RATE, 3, 4),
               put(W.OFF_RATE, 4, 4), put(W.OFF_WITH_LOCATE, 1 | 3 << 8, 4), put(W.OFF_WITH_LOCATE, 1 | 16 << 8, 4),
               put(W.OFF_WITH_LOCATE, 2 | 8 << 8, 4), put(W.OFF_PAIRS, 1, 4, FC.base_wire("six1499", "full"))]
    assert [W.import_verdict(b) for b in refused] == [W.MALFORMED] * len(refused)
    o, nb = FC.part_of(w, "isa")
    assert W.import_verdict(put(o, h.primary + 1, 4)) == W.MALFORMED and W.import_verdict(put(o + 4 * 5, 1344, 4)) == W.MALFORMED
    assert W.import_verdict(put(o + 4 * 5, 1343, 4)) == W.OK
    ws = FC.base_wire("acgtn1344", "s32")
    o, nb = FC.part_of(ws, "marks")
    assert W.import_verdict(put(o + 8, ws[o + 8] ^ 1, 1, ws)) == W.MALFORMED    # one mark more or less
    assert W.import_verdict(put(o, 77, 8, ws)) == W.OK                           # (a line's ones-before word is not counted)


def _outcomes(text_name, build, cases):
    """[(case, 'import' | {query: answer})] -- the model's accessors assert on every read as it goes"""
    out = []
    for name, wire in cases:
        if W.import_verdict(wire) == W.MALFORMED:
            out.append((name, "import", 0))
            continue
        ix = W.WireIndex(wire)
        out.append((name, FC.answers(ix, text_name), ix.cuts))
    return out


def _answered_differently(got, base):
    return got != "import" and got != base and all(v != W.MALFORMED for v in got.values())


def _stopped(got, cuts, base):
    return got != "import" and (cuts > 0 or any(v == W.MALFORMED for v in got.values()))


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_family_goes_through_the_model_and_discriminates(family):
    differently = stopped = cases = 0
    for text_name, build in FC.FAMILY_BASES[family]:
        base = FC.base_index(text_name, build).base_answers
        for name, got, cuts in _outcomes(text_name, build, FC.family(family, text_name, build)):
            cases += 1
            differently += _answered_differently(got, base)
            stopped += _stopped(got, cuts, base)
    assert cases >= 8 and differently >= 1, (family, cases, differently)
    if family in ("V2", "V4", "V6"):
        assert stopped >= 1, (family, cases, stopped)


@pytest.mark.parametrize("chunk", range(FC.VR_CHUNKS))
def test_random_damages_go_through_the_model(chunk):
    per = FC.VR_CASES // FC.VR_CHUNKS
    for i in range(chunk * per, (chunk + 1) * per):
        text_name, build, name, wire = FC.random_case(i)
        assert wire != FC.base_wire(text_name, build)
        _outcomes(text_name, build, [(name, wire)])


def test_random_damages_are_mostly_imported():
    verdicts = [W.import_verdict(FC.random_case(i)[3]) for i in range(FC.VR_CASES)]
    assert verdicts.count(W.MALFORMED) <= FC.VR_CASES // 2, verdicts.count(W.MALFORMED)


def test_random_damages_discriminate():
    """(the first cases that are imported, until one answers differently: the whole family runs above)"""
    for i in range(FC.VR_CASES):
        text_name, build, name, wire = FC.random_case(i)
        (_, got, _), = _outcomes(text_name, build, [(name, wire)])
        if _answered_differently(got, FC.base_index(text_name, build).base_answers):
            return
    assert False, "no random damage changed an answer"
