"""The Huffman container body (run format id 3) as include/textcomp.h describes it, restated in numpy
(tests/huffman_format.py) and pinned here on the ORACLE's runs, without a GPU: the writer's output read back by the
reader is the run list, for small texts and for hand-made run lists with the counts that matter (1, 2, 3, 4, 2^16,
2^32 - 1, a single-token record).  tests/test_gpu_container_huffman.py uses this reader as the judge of the device."""
import struct

import numpy as np
import pytest

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
