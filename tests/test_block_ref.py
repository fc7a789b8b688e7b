"""The foreign blocks of tests/block_ref.py on the CPU: every transformation's and every damage's claim is asserted from
the oracle inside block_ref as the block is built; here every one of them is built, and the families are checked to hold
the outcomes the GPU tests (test_gpu_decode_foreign.py) rely on.  No GPU, no product library."""
import numpy as np
import pytest

import block_ref as B
import oracle as O


def test_mtf_encode_over_is_the_oracles_encoder_on_present_alphabets():
    for name, n in (("acgtn", 4096), ("s12", 4097), ("b256", 4097)):
        sym = B.base_sym(name, n)
        idx, fl = B.mtf_encode_over(sym, np.unique(sym))
        oidx, ofl = O.mtf_encode_arr(sym)
        assert idx.tolist() == oidx.tolist() and fl.tolist() == ofl.tolist()


def test_mtf_encode_over_a_wider_list_round_trips():
    sym = B.base_sym("acgtn", 70001)
    for name, lst in B.t4_lists().items():
        idx, fl = B.mtf_encode_over(sym, lst)
        assert len(fl) == int(name) and sorted(fl.tolist()) == sorted(lst)
        assert O.mtf_decode_arr(idx, fl).tolist() == sym.tolist()
        if int(name) > 6:
            assert int(idx.max()) > 5      # unused symbols below `A` push the indices past the text's own alphabet


def test_base_blocks_are_what_the_table_says():
    sig = {name: {int(B.base_block(name, n)["sigma"]) for n in ns if n >= 255} for name, ns in B.BASES.items()}
    assert sig == dict(acgtn={6}, s12={13}, s40={41}, s100={101}, s150={151}, s200={201}, s255={256}, b256={257}, late={257})
    late = np.frombuffer(B.base_text("late", 70001), np.uint8)
    assert late[:60000].max() == 15 and len(np.unique(late)) == 256
    for name, n in B.all_bases():
        blk = B.base_block(name, n)
        assert B.decode_block_ref(blk) == B.base_text(name, n) and len(B.base_text(name, n)) == n
        assert B.base_sym(name, n)[blk["primary"]] == -1


def test_decode_block_ref_does_not_read_primary():
    blk = dict(B.base_block("s12", 4097))
    del blk["primary"]
    assert B.decode_block_ref(blk) == B.base_text("s12", 4097)


@pytest.mark.parametrize("family", ["T1", "T2", "T3", "T4", "T5"])
def test_transformations_keep_the_text(family):
    k = 0
    for name, n in B.FAMILY_BASES[family]:
        for cid, blk, exp in B.cases(family, name, n):
            assert exp == B.base_text(name, n), (family, name, n, cid)
            k += 1
    assert k >= 10


def test_t1_zero_runs_carry_foreign_values():
    _, blk, _ = [c for c in B.cases("T1", "acgtn", 4096) if c[0] == "zero_foreign"][0]
    zero = blk["run_value"][blk["run_count"] == 0].tolist()
    assert {6, 255, 256, 65535} <= set(zero)
    assert int(blk["run_value"][blk["run_count"] > 0].max()) < 6


def test_t3_grows_sigma_as_stated():
    assert [int(b["sigma"]) for _, b, _ in B.cases("T3", "acgtn", 70001)] == [9, 17]
    assert [int(b["sigma"]) for _, b, _ in B.cases("T3", "s40", 70001)] == [257]
    for _, b, _ in B.cases("T3", "s40", 70001):
        assert len(np.unique(b["final_list"])) == 41


def test_t4_sigma_257_over_a_text_that_lacks_byte_values():
    for name, n in (("acgtn", 70001), ("s12", 70001)):
        blk = [b for cid, b, _ in B.cases("T4", name, n) if cid == "over257"][0]
        assert int(blk["sigma"]) == 257 and 0 < int(blk["primary"]) < n
        assert int(blk["run_value"].max()) > 16


@pytest.mark.parametrize("family", ["M1", "M2", "M4"])
def test_damages_per_base(family):
    for name, n in B.FAMILY_BASES[family]:
        cs = B.cases(family, name, n)
        assert cs and any(exp == B.MALFORMED for _, _, exp in cs), (family, name, n)
        if family in ("M1", "M4"):
            assert all(exp == B.MALFORMED for _, _, exp in cs)


def test_m2_second_nothing_throws_only_on_the_walk():
    kinds = {}
    for name, n in B.FAMILY_BASES["M2"]:
        for cid, blk, exp in B.cases("M2", name, n):
            k = B.ref_outcome(blk)[0]
            kinds[k] = kinds.get(k, 0) + 1
            assert (exp == B.MALFORMED) == (k != "text")
    assert kinds.get("throw", 0) >= 5 and kinds.get("short", 0) >= 5


@pytest.mark.parametrize("name", list(B.BASES))
def test_m3_outcomes_per_alphabet(name):
    full = short = 0
    for n in dict(B.m3_bases())[name]:
        cs = B.cases("M3", name, n)
        assert len(cs) == B.M3_SWAPS
        for cid, blk, exp in cs:
            if exp == B.MALFORMED:
                short += 1
            else:
                assert len(exp) == n and exp != B.base_text(name, n)
                full += 1
    assert full >= 5 and short >= 5, (name, full, short)


def test_m5_lists():
    got = {cid: exp for cid, _, exp in B.m5_lists(B.base_block("s12", 4097))}
    assert got == dict(entry_minus_2="arg", entry_256="arg", sigma_0=B.MALFORMED, sigma_258="arg")
