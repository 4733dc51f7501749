"""Truncated registers on the host (no GPU): d2g_regs_truncate and the two compressed epilogues of compare() against the independent
NumPy restatement tests/trunc_ref.py -- codes, a and b bit for bit; float32 values bit for bit -- and against the frozen
tests/golden/trunc_kat.npz.  The CLI's flag handling is checked at parse time, before any device is touched."""
import os
import subprocess

import numpy as np
import pytest

import trunc_cases as TC
import trunc_ref as R
from conftest import GOLDEN, ROOT

LD = np.longdouble
METHODS = [(rb, bb) for rb in (1, 2, 4) for bb in (False, True)]


def ld_bits(x):
    return np.array([x], LD).tobytes()[:10]


def _matrices():
    rng = np.random.default_rng(77)
    mats = {"oph_families": TC.oph_shaped(rng, 60, 100, families=4, unrelated=6)[0],
            "oph_empty_rows": TC.oph_shaped(rng, 40, 33, families=3, unrelated=4, empty_rows=5)[0],
            "wide_range": TC.wide_range(rng, 30, 65)}
    for seed in range(6):                           # several draws: which side of the seam minreg falls on depends on the data
        mats[f"seam{seed}"] = TC.exp_over_1024(np.random.default_rng(1000 + seed), 24, 48)
    return mats


MATS = _matrices()


@pytest.mark.parametrize("regbytes,bbit", METHODS)
@pytest.mark.parametrize("name", sorted(MATS))
def test_truncate_equals_restatement(d2g, name, regbytes, bbit):
    """codes exactly, a and b bit for bit.  The matrices hold registers equal to minreg and maxreg (the seam of the code range: the
    last bit of logl decides between the top code and the one below), zeros, DBL_MAX and all-zero rows"""
    sigs = MATS[name]
    ecodes, ea, eb, emin, emax = R.truncate(sigs, regbytes, bbit)
    codes, a, b, mn, mx = d2g.regs_truncate(sigs, regbytes, bbit, nthreads=3, with_minmax=True)
    assert codes.dtype == ecodes.dtype
    np.testing.assert_array_equal(codes, ecodes)
    assert ld_bits(a) == ld_bits(ea) and ld_bits(b) == ld_bits(eb)
    if bbit:
        assert int(codes.max()) < (1 << (8 * regbytes if regbytes > 1 else 6))      # a byte code has six significant bits
        assert a == 0 and b == 0
    else:
        assert (mn, mx) == (emin, emax)
        assert (sigs == emin).sum() >= 1 and (sigs == emax).sum() >= 1
        assert (codes[sigs <= 0] == 0).all()                                        # registers <= 0: code 0 by definition
        assert (codes[sigs == emax] == 0).all() or regbytes == 4
        top = {1: 255, 2: 65535, 4: 4294967295}[regbytes]
        assert int(codes[sigs == emin].min()) >= top - 3 and int(codes.max()) <= top


def _grid(S):
    pairs = {(0, 0), (S, 0), (0, S), (S // 2, S - S // 2), (1, S - 1), (1, 0), (0, 1), (S - 1, 0), (S // 3, S // 3), (S // 4, S // 2)}
    return sorted(pairs)


CARDS = [(1e6, 2.5e6), (5000.0, 5000.0), (0.0, 5.0), (7.25, 0.0), (0.0, 0.0), (3e9, 99.5)]
BASES = [LD("1.0647364376997199655"), LD("1.0002434383974204486"), LD("1.0000000037140097567"), LD(2.25)]


@pytest.mark.parametrize("S", [3, 100, 1000, 1024])
def test_epilogue_gtlt_bit_exact(d2g, S):
    """setsketch epilogue (cmp_core.cpp:425-448) for every measure: grid with gt + lt = S, (0, 0), g_b(alpha) + g_b(beta) >= 1, cards
    0 and equal, S not a power of two; the array forms (triangle rows, rectangle) equal the scalar form"""
    pairs = _grid(S)
    for b in BASES:
        gb = R.g_b(b, np.array([p[0] for p in pairs], LD) / LD(S)) + R.g_b(b, np.array([p[1] for p in pairs], LD) / LD(S))
        assert (gb >= 1).any() and (gb < 1).any()
        for meas in range(6):
            for k in ((31,) if meas != d2g.POISSON_LLR else (31, 0)):
                for lhc, rhc in CARDS:
                    g, l = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
                    exp = R.epilogue_gtlt(g, l, S, b, np.full(len(pairs), lhc), np.full(len(pairs), rhc), meas, k)
                    got = np.array([d2g.epilogue_trunc_gtlt(int(x), int(y), S, b, lhc, rhc, meas, k) for x, y in pairs], np.float32)
                    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"b={b} meas={meas} k={k} cards={lhc},{rhc}")
    # array forms: N sketches, counts drawn per pair
    rng = np.random.default_rng(S)
    N = 9
    cards = np.array([1e6, 1e6, 0.0, 5.5, 3e9, 123.0, 77.0, 1e4, 2.0])
    i, j = R.ut_index(N)
    g = rng.integers(0, S + 1, i.size)
    l = np.array([rng.integers(0, S - x + 1) for x in g])
    for meas in range(6):
        exp = R.epilogue_gtlt(g, l, S, BASES[0], cards[i], cards[j], meas, 21)
        got = d2g.host_epilogue_trunc_ut(g, l, cards, N, S, 0, N, meas, 21, 1, BASES[0], nthreads=3)
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
        o0, o1 = d2g.ut_count(N, 0, 2), d2g.ut_count(N, 0, 7)
        part = d2g.host_epilogue_trunc_ut(g[o0:o1], l[o0:o1], cards, N, S, 2, 7, meas, 21, 1, BASES[0], nthreads=2)
        np.testing.assert_array_equal(part.view(np.uint32), exp[o0:o1].view(np.uint32))
        a0, a1, b0, b1 = 1, 6, 3, 9
        rg, rl = rng.integers(0, S // 2 + 1, (a1 - a0, b1 - b0)), rng.integers(0, S - S // 2 + 1, (a1 - a0, b1 - b0))
        rexp = R.epilogue_gtlt(rg.ravel(), rl.ravel(), S, BASES[1], np.repeat(cards[a0:a1], b1 - b0), np.tile(cards[b0:b1], a1 - a0), meas, 21)
        rgot = d2g.host_epilogue_trunc_rect(rg, rl, cards, N, S, a0, a1, b0, b1, meas, 21, 2, BASES[1], nthreads=2)
        np.testing.assert_array_equal(rgot.ravel().view(np.uint32), rexp.view(np.uint32))


@pytest.mark.parametrize("S", [3, 100, 1000, 1024])
def test_epilogue_bbit_bit_exact(d2g, S):
    """b-bit epilogue (cmp_core.cpp:406-423; the fmal is one rounding) for every measure: neq in {0, 1, S-1, S} and between; the
    array forms equal the scalar form"""
    neqs = sorted({0, 1, S // 2, S - 1, S, S // 3})
    for regbytes in (1, 2, 4):
        for meas in range(6):
            for k in ((31,) if meas != d2g.POISSON_LLR else (31, 0)):
                for lhc, rhc in CARDS:
                    exp = R.epilogue_bbit(neqs, S, regbytes, np.full(len(neqs), lhc), np.full(len(neqs), rhc), meas, k)
                    got = np.array([d2g.epilogue_trunc_neq(n, S, regbytes, lhc, rhc, meas, k) for n in neqs], np.float32)
                    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"rb={regbytes} meas={meas} k={k} cards={lhc},{rhc}")
    rng = np.random.default_rng(S + 1)
    N = 8
    cards = np.array([1e6, 1e6, 0.0, 5.5, 3e9, 123.0, 77.0, 1e4])
    i, j = R.ut_index(N)
    neq = rng.integers(0, S + 1, i.size)
    for meas in range(6):
        exp = R.epilogue_bbit(neq, S, 2, cards[i], cards[j], meas, 31)
        got = d2g.host_epilogue_trunc_ut(neq, None, cards, N, S, 0, N, meas, 31, 2, None, nthreads=3)
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
        rn = rng.integers(0, S + 1, (3, N))
        rexp = R.epilogue_bbit(rn.ravel(), S, 1, np.repeat(cards[2:5], N), np.tile(cards, 3), meas, 31)
        rgot = d2g.host_epilogue_trunc_rect(rn, None, cards, N, S, 2, 5, 0, N, meas, 31, 1, None, nthreads=2)
        np.testing.assert_array_equal(rgot.ravel().view(np.uint32), rexp.view(np.uint32))


def test_fmal_restatement_is_one_rounding():
    """the checker's own fmal: (1 + 2^-63)(1 + 2^-62) - 1 = 3 * 2^-63 + 2^-125 exactly, which multiply-then-add loses"""
    x, y, z = LD(1) + np.ldexp(LD(1), -63), LD(1) + np.ldexp(LD(1), -62), LD(-1)
    want = np.ldexp(LD(3), -63) + np.ldexp(LD(1), -125)
    assert R.fmal(x, y, z) == want and x * y + z != want
    assert R.fmal(LD(2), LD(0.5), LD(0.25)) == LD(1.25) and R.fmal(LD(3), LD(0), LD(0)) == 0
    big = np.ldexp(LD(1), 63) + LD(1)
    assert R.fraction_to_ld(R.ld_to_fraction(big)) == big and R.fraction_to_ld(R.ld_to_fraction(-big / LD(3))) == -big / LD(3)


def test_frozen_fixture(d2g):
    """tests/golden/trunc_kat.npz (made by tests/golden/make_trunc_golden.py from the restatement)"""
    z = np.load(os.path.join(GOLDEN, "trunc_kat.npz"))
    for name in ("oph", "wide", "seam"):
        for rb in (1, 2, 4):
            for bb in (0, 1):
                codes, a, b = d2g.regs_truncate(z[f"sig_{name}"], rb, bb)
                np.testing.assert_array_equal(codes, z[f"codes_{name}_{rb}_{bb}"])
                if not bb:
                    assert ld_bits(a) == z[f"a_{name}_{rb}"].tobytes() and ld_bits(b) == z[f"b_{name}_{rb}"].tobytes()
    bases = [np.frombuffer(bytes(r) + b"\0" * 6, LD)[0] for r in z["bases"]]
    gi, gc = z["gtlt_in"], z["gtlt_cards"]
    got = np.array([d2g.epilogue_trunc_gtlt(int(r[0]), int(r[1]), int(r[2]), bases[int(r[3])], c[0], c[1], int(r[4]), int(r[5]))
                    for r, c in zip(gi, gc)], np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), z["gtlt_out"])
    ni, nc = z["neq_in"], z["neq_cards"]
    got = np.array([d2g.epilogue_trunc_neq(int(r[0]), int(r[1]), int(r[2]), c[0], c[1], int(r[3]), int(r[4])) for r, c in zip(ni, nc)], np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), z["neq_out"])


def test_truncate_refusals(d2g):
    sigs = MATS["oph_families"]
    for rb in (3, 0, 8):
        with pytest.raises(d2g.D2GError, match="1, 2 or 4"):
            d2g.regs_truncate(sigs, rb)
    bad = sigs.copy()
    bad[3, 5] = np.inf
    with pytest.raises(d2g.D2GError, match=r"\+inf"):
        d2g.regs_truncate(bad, 2)
    for empty in (np.zeros((4, 8)), np.full((4, 8), TC.DBL_MAX)):
        with pytest.raises(d2g.D2GError, match="no finite positive register"):
            d2g.regs_truncate(empty, 1)
    codes, a, b = d2g.regs_truncate(np.zeros((4, 8)), 1, bbit=True)          # the b-bit method hashes whatever is there
    np.testing.assert_array_equal(codes, R.truncate(np.zeros((4, 8)), 1, True)[0])


def test_cli_fastcmp_flag_validation():
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
    for flag in ("--fastcmp", "--regsize", "--regbytes"):
        for arg in ("3", "0.5", "16", "x"):
            r = subprocess.run([exe, "cmp", "--presketched", flag, arg, "nothing.bin"], capture_output=True, text=True)
            assert r.returncode == 1, (flag, arg)
            assert "--fastcmp must have 8, 4, 2, or 1 as the argument. These are the only register sizes supported.\n" in r.stderr   # options.h:323
            assert "See usage for --fastcmp instructions." in r.stderr                                                              # options.h:324
    for flag in (["--fastcmp-bytes"], ["--fastcmp-shorts"], ["--fastcmp-words"], ["--fastcmp-nibbles"], ["--setsketch-ab", "1,2"]):
        r = subprocess.run([exe, "cmp", "--presketched"] + flag + ["nothing.bin"], capture_output=True, text=True)
        assert r.returncode == 1 and "outside the hot-path scope" in r.stderr, flag
    r = subprocess.run([exe, "cmp", "-h"], capture_output=True, text=True)
    assert "--fastcmp/--regsize/--regbytes <8|4|2|1>" in r.stderr and "--bbit-sigs" in r.stderr
