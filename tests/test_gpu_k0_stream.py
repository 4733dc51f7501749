"""K0's packed stream read back BASE FOR BASE, at the seams of the device parser (cases: k0_seam_cases.py; reference: the plain model
of k0_ref.py, itself pinned against the host packer and the oracle by test_k0_ref.py).

The readback needs no entry point of its own.  d2g_sketcher_run with packed == NULL runs K1 over the stream ingested last with the
CALLER's run table, so the table here is one genome per window of W = min(32, nbases) bases -- windows at 0, 32, 64, ... and a last one
ending at nbases -- with k = W, canon off, xormask 0, S = 2.  Each genome then has exactly one k-mer, the smaller of its two registers is
wang64(wang64(x) ^ d2g_oph_xor_const()) with x the window's bases (first base most significant), and Wang's mix is a bijection: equal
hashes for every window <=> every base of the stream is the model's.  test_readback_returns_a_known_stream is the control: the same
window tables over a stream packed on the host, at all 16 word alignments.

test_gpu_k0.py sees K0 through run lengths (a lost base shows, a wrong or misplaced one does not) and through minima over k-mers (one
wrong base rarely moves a register); this file sees the bases."""
import numpy as np
import pytest

import k0_ref
import k0_seam_cases as kc

pytestmark = pytest.mark.gpu

KS = (1, 5, 31, 32)
_parsed = {}


def parsed(case):
    if case.name not in _parsed:
        _parsed[case.name] = k0_ref.Parsed(case.files, case.genome_nfiles)
    return _parsed[case.name]


def assert_stream_is(sk, d2g, m, what):
    """every window of the device stream ingested last equals the model's"""
    starts, W = k0_ref.window_starts(m.nbases)
    if not W:
        return
    regs = sk.run_ingested(k0_ref.window_table(starts, W), 2, canon=False, xormask=0, k=W)
    got = regs.min(axis=1)
    exp = k0_ref.window_hashes(m.codes, starts, W, d2g.oph_xor_const())
    bad = np.flatnonzero(got != exp)
    if bad.size:
        a = int(starts[bad[0]])
        pytest.fail(f"{what}: {bad.size} of {starts.size} windows differ; the first holds bases [{a}, {a + W}) of {m.nbases}, "
                    f"expected {m.bases(a, W)}")
    assert ((regs == np.uint64(0xFFFFFFFFFFFFFFFF)).sum(axis=1) >= 1).all(), what    # one k-mer per genome: one register stays empty


def assert_ingest_is(sk, d2g, case, k):
    m = parsed(case)
    what = f"case {case.name}, k = {k}"
    rs, rl, go, nk, nbases = sk.ingest_fasta(case.files, k, genome_nfiles=case.genome_nfiles)
    assert nbases == m.nbases, what
    assert_stream_is(sk, d2g, m, what)
    mrs, mrl, mgo, mnk = m.run_table(k)
    np.testing.assert_array_equal(rs, mrs, err_msg=what + ": run_start")
    np.testing.assert_array_equal(rl, mrl, err_msg=what + ": run_len")
    np.testing.assert_array_equal(go, mgo, err_msg=what + ": genome_run_off")
    np.testing.assert_array_equal(nk, mnk, err_msg=what + ": genome_nkmers")


def assert_refused(sk, d2g, case, k):
    with pytest.raises(d2g.D2GError) as ei:
        sk.ingest_fasta(case.files, k, genome_nfiles=case.genome_nfiles)
    assert ei.value.status == -5, case.name                            # D2G_ERR_UNSUPPORTED
    with pytest.raises(d2g.D2GError):                                  # nothing is staged after a refusal
        sk.run_ingested(k0_ref.window_table([0], 1), 2, canon=False, k=1)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("group", kc.GROUPS)
def test_stream_and_run_table_equal_the_model(gpu_ctx, d2g, group, k):
    cases = kc.by_group(group)
    assert cases
    sk = gpu_ctx.sketcher()
    for case in cases:
        assert not parsed(case).refused, case.name
        assert_ingest_is(sk, d2g, case, k)
    sk.close()


@pytest.mark.parametrize("k", KS)
def test_plus_at_a_line_start_is_refused(gpu_ctx, d2g, k):
    cases = [c for c in kc.CASES if c.refused]
    assert len(cases) == len(kc.SEAMS) * 3 + 1
    sk = gpu_ctx.sketcher()
    for case in cases:
        assert parsed(case).refused, case.name
        assert_refused(sk, d2g, case, k)
    # the same bytes with the '+' moved off the line start are accepted (the catalogue's plus_midline cases), and the sketcher that
    # refused still parses exactly
    assert_ingest_is(sk, d2g, kc.by_group("plus")[0], k)
    sk.close()


@pytest.mark.parametrize("k", KS)
def test_reused_sketcher_leaves_no_stale_bits(gpu_ctx, d2g, k):
    """the emit pass ORs into the words that tiles share: a stream of all T (every bit set), then smaller inputs on the same buffers --
    also right after a refused input -- must come out exact"""
    sk = gpu_ctx.sketcher()
    for case in kc.REUSE:
        if case.refused:
            assert_refused(sk, d2g, case, k)
        else:
            assert_ingest_is(sk, d2g, case, k)
    sk.close()


def test_readback_returns_a_known_stream(gpu_ctx, d2g):
    """control: window tables over a stream packed on the host return that stream, whatever the word alignment of the windows and
    whatever W; and one changed base changes exactly the windows that hold it"""
    n = 5000
    codes = np.random.default_rng(9).integers(0, 4, n).astype(np.uint8)
    packed = k0_ref.pack_codes(codes)
    xc = d2g.oph_xor_const()
    for W in (1, 5, 31, 32):
        for a in range(16):
            starts = np.arange(a, n - W + 1, 32)
            regs = gpu_ctx.oph_sketch(packed, *k0_ref.window_table(starts, W), W, 2, canon=False, xormask=0)
            np.testing.assert_array_equal(regs.min(axis=1), k0_ref.window_hashes(codes, starts, W, xc), err_msg=f"W={W} alignment {a}")
    starts, W = k0_ref.window_starts(n)
    for p in (0, 31, 32, 2500, n - 1):
        wrong = codes.copy()
        wrong[p] ^= 1
        regs = gpu_ctx.oph_sketch(k0_ref.pack_codes(wrong), *k0_ref.window_table(starts, W), W, 2, canon=False, xormask=0)
        differ = regs.min(axis=1) != k0_ref.window_hashes(codes, starts, W, xc)
        np.testing.assert_array_equal(differ, (starts <= p) & (p < starts + W), err_msg=f"base {p}")
