"""The Huffman container body (run format id 3) as include/textcomp.h describes it, restated in numpy
(tests/huffman_format.py) and pinned here on the ORACLE's runs, without a GPU: the writer's output read back by the
reader is the run list, for small texts and for hand-made run lists with the counts that matter (1, 2, 3, 4, 2^16,
2^32 - 1, a single-token record).  tests/test_gpu_container_huffman.py uses this reader as the judge of the device.

tests/test_gpu_huffman_synthetic.py compares the device with this restatement on run lists no text produces, and
requires the coded size under the device's lengths to EQUAL that under build_lengths: so the builder is checked here
exhaustively for optimality on small cases, and the restatement's own round trips are pinned on the regimes of that
file (tests/huffman_cases.py: histograms on which the limit binds, 31-digit counts, K != 1024, L_max < 12, incomplete
codes)."""
import itertools
import struct

import numpy as np
import pytest

import huffman_cases as S
import huffman_format as H
import oracle as O


def _oracle_runs(text):
    L = O.bwt_encode_arr(text)
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return np.asarray(counts, np.int64), np.asarray(vals, np.int64), len(fl)


def _texts():
    r = np.random.default_rng(5)
    return {
        "acgtn_3000": O.gen_acgtn(3, 3000),
        "acgtn_70001": O.gen_acgtn(4, 70001),
        "ascii_20000": O.gen_ascii(9, 20000),
        "binary_9000": r.integers(0, 256, 9000).astype(np.uint8),
        "unary_70000": np.full(70000, 65, np.uint8),                     # a run of 2^16 and more
        "runs_1_to_6": np.repeat(np.frombuffer(b"ACGNT", np.uint8)[r.integers(0, 5, 6000)], r.integers(1, 7, 6000)).astype(np.uint8),
        "one_byte": np.frombuffer(b"A", np.uint8),
    }


TEXTS = _texts()


@pytest.mark.parametrize("name", list(TEXTS), ids=list(TEXTS))
def test_writer_and_reader_agree_on_the_oracles_runs(name):
    counts, vals, sigma = _oracle_runs(TEXTS[name])
    body = H.write_body(counts, vals, sigma)
    K, nchunks, nsyms, lmax = struct.unpack_from("<4I", body, 0)
    assert (K, nchunks, nsyms, lmax) == (1024, (len(counts) + 1023) // 1024, sigma + 2, 12)
    assert len(body) % 16 == 0
    c, v = H.read_body(body, len(counts), sigma)
    assert np.array_equal(c, counts) and np.array_equal(v, vals)
    lengths = np.frombuffer(body, np.uint8, nsyms, 16)
    assert lengths.max() <= lmax and H.kraft(lengths, lmax) <= 1 << lmax


@pytest.mark.parametrize("K", [1, 4, 1024])
def test_counts_that_matter(K):
    counts = np.array([1, 2, 3, 4, 5, 6, 7, 8, 1 << 16, (1 << 16) + 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1], np.int64)
    vals = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3], np.int64)
    body = H.write_body(counts, vals, 6, K=K)
    c, v = H.read_body(body, len(counts), 6)
    assert c.tolist() == counts.tolist() and v.tolist() == vals.tolist()


def test_tokens_are_bzip2s_run_digits():
    # c - 1 in bijective base 2, least significant digit first: RUNA = sigma is digit 1, RUNB = sigma + 1 is digit 2
    tok, first = H.tokens_of_runs([1, 2, 3, 4, 5, 6, 7, 8], [0] * 8, 6)
    runs = [tok[first[i]:first[i + 1]].tolist() for i in range(8)]
    assert runs == [[0], [0, 6], [0, 7], [0, 6, 6], [0, 7, 6], [0, 6, 7], [0, 7, 7], [0, 6, 6, 6]]
    with pytest.raises(ValueError):
        H.tokens_of_runs([0], [0], 6)


def test_single_token_record_gets_length_one():
    counts, vals = np.ones(5, np.int64), np.zeros(5, np.int64)
    body = H.write_body(counts, vals, 2)
    assert np.frombuffer(body, np.uint8, 4, 16).tolist() == [1, 0, 0, 0]
    c, v = H.read_body(body, 5, 2)
    assert c.tolist() == [1] * 5 and v.tolist() == [0] * 5


def test_canonical_codes_and_length_builder():
    assert H.canonical_codes([2, 1, 3, 3, 0]).tolist() == [0b10, 0b0, 0b110, 0b111, 0]
    hist = [1000, 500, 250, 125, 60, 30, 15, 8, 4, 2, 1, 1, 0]
    ln = H.build_lengths(hist, 12)
    assert ln[-1] == 0 and ln[:-1].min() >= 1 and H.kraft(ln, 12) == 1 << 12
    assert sum(int(h) * int(l) for h, l in zip(hist, ln)) == H.optimal_huffman_bits(hist)      # the limit does not bind
    ln5 = H.build_lengths(hist, 5)
    assert ln5.max() <= 5 and H.kraft(ln5, 5) <= 1 << 5
    assert sum(int(h) * int(l) for h, l in zip(hist, ln5)) >= H.optimal_huffman_bits(hist)


def test_reader_refuses_what_the_format_forbids():
    counts, vals, sigma = _oracle_runs(TEXTS["acgtn_3000"])
    good = bytearray(H.write_body(counts, vals, sigma))
    n = len(counts)

    def edited(fn):
        b = bytearray(good)
        fn(b)
        return bytes(b)
    doff = 16 + ((sigma + 2 + 15) & ~15)
    cases = {
        "K=0": lambda b: struct.pack_into("<I", b, 0, 0),
        "K=3": lambda b: struct.pack_into("<I", b, 0, 3),
        "nchunks+1": lambda b: struct.pack_into("<I", b, 4, struct.unpack_from("<I", b, 4)[0] + 1),
        "nsyms": lambda b: struct.pack_into("<I", b, 8, sigma + 3),
        "lmax=13": lambda b: struct.pack_into("<I", b, 12, 13),
        "length>lmax": lambda b: b.__setitem__(16, 13),
        "kraft": lambda b: b.__setitem__(slice(16, 16 + sigma + 2), bytes([1] * (sigma + 2))),
        "dir-32": lambda b: struct.pack_into("<I", b, doff, struct.unpack_from("<I", b, doff)[0] - 32),
        "dir+32": lambda b: struct.pack_into("<I", b, doff, struct.unpack_from("<I", b, doff)[0] + 32),
    }
    for name, fn in cases.items():
        with pytest.raises(H.Malformed):
            H.read_body(edited(fn), n, sigma)
    c, v = H.read_body(bytes(good), n, sigma)
    assert np.array_equal(c, counts)


# ---- the length builder is optimal under the limit ------------------------------------------------------------------------
def _feasible(m, lmax):
    """every assignment of lengths 1..lmax to m tokens with a Kraft sum <= 1, as rows"""
    rows = np.array(list(itertools.product(range(1, lmax + 1), repeat=m)), dtype=np.int64)
    return rows[(1 << (lmax - rows)).sum(axis=1) <= 1 << lmax]


@pytest.mark.parametrize("lmax", [1, 2, 3, 4])
def test_length_builder_is_optimal_by_exhaustion(lmax):
    r = np.random.default_rng(1000 + lmax)
    checked = bound = 0
    for m in range(2, min(7, 1 << lmax) + 1):
        rows = _feasible(m, lmax)
        assert len(rows)
        for i in range(60):
            kind = i % 4          # uniform small weights (many ties), wide weights, geometric, Fibonacci-like with noise
            if kind == 0:
                h = r.integers(1, 5, m)
            elif kind == 1:
                h = r.integers(1, 100000, m)
            elif kind == 2:
                h = (1 << r.permutation(m)) + r.integers(0, 2, m)
            else:
                h = r.permutation(np.array([1, 1, 2, 3, 5, 8, 13][:m])) * int(r.integers(1, 50)) + r.integers(0, 2, m)
            nz = int(r.integers(0, 3))          # tokens that do not occur, anywhere in the table
            hist = np.zeros(m + nz, np.int64)
            at = np.sort(r.choice(m + nz, m, replace=False))
            hist[at] = h
            ln = H.build_lengths(hist, lmax).astype(np.int64)
            assert (ln[hist == 0] == 0).all() and ln[at].min() >= 1 and ln.max() <= lmax and H.kraft(ln, lmax) <= 1 << lmax
            best = int((rows @ h).min())
            assert int((hist * ln).sum()) == best, (hist.tolist(), ln.tolist(), best)
            checked += 1
            bound += best > H.optimal_huffman_bits(hist)
    assert checked >= 60 and (bound > 0 or lmax == 1 or lmax == 4)       # (the limit does bind on some of them)
    # a lone token: length 1, whatever the limit
    assert H.build_lengths([0, 7, 0], lmax).tolist() == [0, 1, 0]


def test_length_builder_costs_no_more_than_any_shorter_limit_and_meets_huffman_when_it_can():
    r = np.random.default_rng(77)
    for _ in range(40):
        m = int(r.integers(2, 260))
        hist = np.maximum(1, (r.pareto(0.7, m) * 10).astype(np.int64))
        need = max(S.unlimited_lengths(hist))
        costs = []
        for lmax in range(max(1, int(np.ceil(np.log2(m)))), 13):
            ln = H.build_lengths(hist, lmax).astype(np.int64)
            assert ln.min() >= 1 and ln.max() <= lmax and H.kraft(ln, lmax) <= 1 << lmax
            costs.append(int((hist * ln).sum()))
            if lmax >= need:
                assert costs[-1] == H.optimal_huffman_bits(hist)
            else:
                assert costs[-1] >= H.optimal_huffman_bits(hist)
        assert costs == sorted(costs, reverse=True)


# ---- round trips on the regimes of tests/test_gpu_huffman_synthetic.py ------------------------------------------------------
def _round_trip(counts, vals, sigma, **kw):
    body = H.write_body(counts, vals, sigma, **kw)
    assert len(body) % 16 == 0
    c, v = H.read_body(body, len(counts), sigma)
    assert np.array_equal(c, counts) and np.array_equal(v, vals)
    return body


def test_round_trip_where_the_limit_binds():
    for counts, vals, sigma in (S.fib_values(22, 24, 1), S.fib_all_tokens(2)):
        g = S.regime(counts, vals, sigma)
        assert g["unlimited_depth"] > 12 and g["longest"] == 12 and g["limited_bits"] > g["unlimited_bits"]
        body = _round_trip(counts, vals, sigma)
        assert len(body) < H.packed_body_bytes(counts, sigma)
    counts, vals, sigma = S.fib_values(22, 24, 1)
    g = S.regime(counts, vals, sigma)
    assert (len(counts), g["unlimited_depth"], g["limited_bits"], g["unlimited_bits"]) == (46367, 21, 121376, 121367)


def test_round_trip_of_31_digit_counts_and_long_chunks():
    counts, vals, sigma = S.every_digit_count(4)
    assert set(S.ndigits(counts).tolist()) == set(range(32))
    _round_trip(counts, vals, sigma)
    counts, vals, sigma = S.long_chunk(3)
    g = S.regime(counts, vals, sigma)
    assert g["chunk_words"][1] > 2 * S.IMG_WORDS and g["straddlers"] >= 2
    _round_trip(counts, vals, sigma)
    for which in (0, 1):
        counts, vals, sigma = S.rare_digit(5 + which, which, nruns=150000)
        _round_trip(counts[:12000], vals[:12000], sigma, lengths=S.regime(counts, vals, sigma)["lengths"])
    # the closed form of a run's bits (what the device counts by) against the token stream itself
    counts, vals, sigma = S.every_digit_count(4)
    tok, first = H.tokens_of_runs(counts, vals, sigma)
    ln = H.build_lengths(np.bincount(tok, minlength=sigma + 2)).astype(np.int64)
    assert np.array_equal(S.run_bits(counts, vals, sigma, ln), np.add.reduceat(ln[tok], first[:-1]))


@pytest.mark.parametrize("K", [1, 2, 64, 512, 4096, 1 << 20])
@pytest.mark.parametrize("lmax", [9, 10, 12])
def test_round_trip_with_other_chunk_sizes_and_limits(K, lmax):
    counts, vals, sigma = S.fib_values(19, 20, 3)          # 6764 runs, 18 deep without a limit
    body = _round_trip(counts, vals, sigma, K=K, lmax=lmax)
    L = S.body_layout(body)
    assert (L["K"], L["lmax"], L["nchunks"]) == (K, lmax, (len(counts) + K - 1) // K)
    assert np.frombuffer(body, np.uint8, sigma + 2, 16).max() == lmax


def test_round_trip_with_the_shortest_limits():
    c, v, s = S.two_tokens(52, 9001, 2)
    assert np.frombuffer(_round_trip(c, v, s, lmax=1, K=32), np.uint8, 4, 16).tolist() == [1, 1, 0, 0]
    c, v, s = S.single_token(9001, 3)
    _round_trip(c, v, s, lmax=1, K=8)
    r = np.random.default_rng(53)
    c, v = r.integers(1, 3, 7001).astype(np.int64), r.integers(0, 2, 7001).astype(np.int64)
    body = _round_trip(c, v, 2, lmax=2, K=2048)
    assert sorted(np.frombuffer(body, np.uint8, 4, 16).tolist()) == [0, 1, 2, 2]


def test_round_trip_with_incomplete_codes():
    counts, vals, sigma = S.mild(51, 10007, 9)
    hist = H.histogram(counts, vals, sigma)
    plus = np.where(H.build_lengths(hist, 8) > 0, H.build_lengths(hist, 8).astype(np.int64) + 1, 0)
    assert H.kraft(plus, 9) == 1 << 8
    body = _round_trip(counts, vals, sigma, lengths=plus, K=128, lmax=9)
    # bits that match no code are refused: the last code of an incomplete table is not all ones, so a payload of ones fails
    L = S.body_layout(body)
    bad = bytearray(body)
    bad[L["poff"]:L["poff"] + 4] = b"\xff" * 4
    with pytest.raises(H.Malformed):
        H.read_body(bytes(bad), len(counts), sigma)
    order = np.argsort(-hist, kind="stable")
    gap = np.zeros(sigma + 2, np.int64)
    gap[order[:2]], gap[order[2:10]], gap[order[10:]] = 2, 7, 12
    gap[hist == 0] = 0
    assert H.kraft(gap, 12) < 1 << 12 and set(gap[gap > 0].tolist()) == {2, 7, 12}
    _round_trip(counts, vals, sigma, lengths=gap)


def test_mutation_lists_are_fixed_and_mixed():
    """part C of the GPU file: every seeded list holds both verdicts at least 20 times, by the restatement alone"""
    counts, vals, sigma = S.every_digit_count(4)
    body = H.write_body(counts, vals, sigma)
    muts = S.mutants(body, 101)
    assert muts == S.mutants(body, 101) and all(b != body and len(b) == len(body) for _, b in muts)
    refused = sum(S.verdict(b, len(counts), sigma) is None for _, b in muts)
    assert 100 <= len(muts) <= 140 and refused >= 20 and len(muts) - refused >= 20
