"""Interval inputs (--bed), no GPU: the recorded XXH3 digests against libd2g's d2g_xxh3_64 (and against the `xxhash` module where it
imports), libd2g's line parser against the restatement of tests/bed_ref.py, and that restatement held to closed forms: set-space
registers are the per-register minimum over the UNION of the covered positions whatever the line order; integer multiset weights are
coverage counts whatever the line order."""
import random

import numpy as np
import pytest

import bed_ref as R

LINES = (b"#track name=x\n\nchr1\t5\t10\nChr1\t7\t12\tpeak\t+\n1\t0\t3\r\nCHR1\t1\t2\nch1\t4\t5\nchr\t1\t2\n\t1\t2\nchrX\t +5 \t 9\n"
         b"chrY\t5\nchrMT\t\nchr2\t10\t5\nchr3\t4294967295\t4294967298\nchr4\t-1\t3\nchr5\tx\t9\nchr6\t18446744073709551616\t7\nchr7\t3\t4")


def test_golden_digests_match_the_library(d2g):
    t = R.golden_table()
    assert {len(n) for n in t} >= set(range(241)) and len(t) >= 241 + 75
    for name, want in t.items():
        assert d2g.xxh3_64(name) == want, name
    with pytest.raises(ValueError):
        d2g.xxh3_64(b"a" * 241)


def test_golden_digests_match_the_xxhash_module():
    xxhash = pytest.importorskip("xxhash")
    for name, want in R.golden_table().items():
        assert xxhash.xxh3_64_intdigest(name) == want


def test_strtoul_restatement():
    assert R.strtoul(b"  +5x", 0) == (5, 4) and R.strtoul(b"-1", 0) == ((1 << 64) - 1, 2) and R.strtoul(b"x5", 0) == (0, 0)
    assert R.strtoul(b"18446744073709551616", 0) == ((1 << 64) - 1, 20) and R.strtoul(b"-18446744073709551616", 0) == ((1 << 64) - 1, 21)
    assert R.strtoul(b"\t\r 7\r", 0) == (7, 4) and R.strtoul(b"", 0) == (0, 0) and R.strtoul(b"+", 0) == (0, 0)


@pytest.mark.parametrize("trim", [True, False])
def test_library_parser_against_the_restatement(d2g, trim):
    want = R.parse(LINES, trim)
    h, a, b = d2g.bed_parse(LINES, trim)
    assert len(want) == 16 and h.size == len(want)
    for j, (name, s, e) in enumerate(want):
        assert (int(h[j]), int(a[j]), int(b[j])) == (R.chrom_hash(name), s, e), (j, name)
    if trim:
        assert [n for n, _, _ in want[:7]] == [b"1", b"1", b"1", b"CHR1", b"ch1", b"", b""]
        assert want[8][1:] == (5, 0) and want[9][1:] == (0, 0) and want[12][1:] == ((1 << 64) - 1, 3) and want[13][1:] == (0, 0)


@pytest.mark.parametrize("buf", [b"chr1 5 10\n", b"chr1\t1\t2\nnope\n", b"\r\n"])
def test_a_line_without_a_tab_is_refused_in_the_references_words(d2g, buf):
    with pytest.raises(ValueError) as r:
        R.parse(buf)
    with pytest.raises(ValueError) as l:
        d2g.bed_parse(buf)
    assert str(l.value) == str(r.value) and str(r.value).startswith("Malformed line: ")


def test_gzip_and_long_names_are_refused_by_name(d2g):
    with pytest.raises(ValueError, match="gzip"):
        d2g.bed_parse(b"\x1f\x8b\x08\x00rest\t1\t2\n")
    with pytest.raises(ValueError, match="241 bytes"):
        d2g.bed_parse(b"q" * 241 + b"\t1\t2\n")
    assert d2g.bed_parse(b"chr" + b"q" * 240 + b"\t1\t2\n")[0][0] == d2g.xxh3_64(b"q" * 240)


def _lines(seed, n=40):
    rng = random.Random(seed)
    hs = [R.chrom_hash(c) for c in (b"1", b"2", b"X")]
    out = []
    for _ in range(n):
        a = rng.choice([0, 50, (1 << 32) - 20]) + rng.randrange(60)
        out.append((rng.choice(hs), a, a + rng.choice([0, 1, 3, 7, 63, 64, 65, 130])))
    return out + out[:3]                                                 # duplicates


@pytest.mark.parametrize("S", [64, 33, 100])
def test_set_space_is_the_minimum_over_the_union_whatever_the_order(S):
    lines = _lines(1)
    want = R.oph_registers(lines, S)
    # closed form: every distinct covered (chromosome, position) once, ascending
    union = sorted({(h, i) for h, a, b in lines for i in range(a, b)})
    m = S + (S & 1)
    regs = [R.M64] * m
    for h, i in union:
        x = int(R.wang64(np.array([(h ^ i) ^ R.OPH_XOR], np.uint64))[0])
        r = x & (m - 1) if m & (m - 1) == 0 else (x & 0xFFFFFFFF) % m
        regs[r] = min(regs[r], x)
    assert want.tolist() == regs
    for seed in range(3):
        sh = lines[:]
        random.Random(seed).shuffle(sh)
        assert np.array_equal(R.oph_registers(sh, S), want)


def test_integer_multiset_weights_are_coverage_counts_whatever_the_order():
    lines = _lines(2)
    want = R.closed_form_weights(lines)
    ids0, w0, tw0 = R.multiset_lists(lines)
    assert tw0 == float(sum(want.values())) and ids0.size == len(want)
    for seed in range(3):
        sh = lines[:]
        random.Random(seed).shuffle(sh)
        w = R.multiset_weights(sh)
        assert {k: int(v) for k, v in w.items()} == want and all(v == int(v) for v in w.values())
        ids, ws, tw = R.multiset_lists(sh)
        assert np.array_equal(ids, ids0) and np.array_equal(ws, w0) and tw == tw0


def test_normalised_weights_follow_the_line_order():
    h = R.chrom_hash(b"1")
    lines = [(h, 0, 3), (h, 0, 7), (h, 2, 3), (h, 0, 3)]
    w = R.multiset_weights(lines, normalize=True)
    assert w[(h, 2)] == ((0.0 + 1.0 / 3.0) + 1.0 / 7.0 + 1.0) + 1.0 / 3.0 and w[(h, 5)] == 1.0 / 7.0
    assert R.multiset_weights([(h, 5, 5), (h, 9, 2)], normalize=True) == {}
