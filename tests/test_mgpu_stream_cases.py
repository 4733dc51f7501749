"""mgpu_stream_cases.py held to what it promises, without a GPU: P1-P3 of its docstring for every shape, world size and sequence that
test_gpu_mgpu_streams.py feeds to the engine, with the pair ranges of d2g.ut_partition and the even split of the rows.  The figures are
printed past pytest's capture, so the plain command shows them; the minima stand in the case module's docstring."""
import numpy as np
import pytest

import mgpu_stream_cases as M


def _figures(d2g, mats, W, min_pairs, min_frac, witness_rows=None):
    """P1-P3 over consecutive matrices; -> (P1 maximum over steps of the patterns shared with the step before, P2 minimum over steps,
    groups and ranks as (pairs, step, group, rank), P3 minimum over steps and ranks)"""
    N, S = mats[0].shape
    b = d2g.ut_partition(N, W)
    held = M.even_split(N, W)
    assert b[0] == 0 and b[-1] == N and held[0] == 0 and held[-1] == N
    # the rows whose pairs are counted: a rank's whole slab, or its first `witness_rows` rows (a lower bound of P2)
    rows = [(b[r], b[r + 1] if witness_rows is None else min(b[r + 1], b[r] + witness_rows)) for r in range(W)]
    rows = [(r, lo, hi) for r, (lo, hi) in enumerate(rows) if d2g.ut_count(N, b[r], b[r + 1]) > 0]   # ranks with a non-empty slab
    assert rows
    p1, p2, p3 = [], [], []
    prev = None
    for t, m in enumerate(mats):
        assert m.shape == (N, S) and m.dtype == np.float64 and np.isfinite(m).all() and (m >= 0).all()
        cur = [M.group_counts(m, lo, hi) for _, lo, hi in rows]
        if t:
            p1.append(M.shared_patterns(m, mats[t - 1]))
            assert p1[-1] == 0, f"P1: step {t} shares {p1[-1]} patterns with step {t - 1}"
            for (r, lo, hi), ga, gb in zip(rows, cur, prev):
                d = M.pairs_that_differ(ga, gb, lo)
                assert d.size == (S + 31) // 32
                p2.append((int(d.min()), t, int(d.argmin()), r))
                assert d.min() >= min_pairs, f"P2: step {t} rank {r} rows [{lo},{hi}) group {int(d.argmin())}: {int(d.min())} pairs differ"
            for r in range(W):
                f = M.slab_fraction_that_differs(m, mats[t - 1], held[r], held[r + 1])
                p3.append(f)
                assert f >= min_frac, f"P3: step {t} rank {r}: {f}"
        prev = cur
    return max(p1), min(p2), min(p3)


def _show(capsys, text):
    with capsys.disabled():
        print("\n" + text)


def test_group_counts_add_up_to_the_oracle(d2g, oracle):
    """the blocked NumPy counts per 32-register group, summed over the groups, are the oracle's counts (S no multiple of 32)"""
    N, S = 129, 100
    m = M.sequence(N, S, 1, 5, M.PLANTED_KINDS)[0]
    g = M.group_counts(m, 0, N)
    assert g.shape == (N, N, 4)
    full = g.sum(axis=2, dtype=np.uint32)
    np.testing.assert_array_equal(full[np.triu_indices(N, 1)], oracle.eqcounts_ut(m))
    same = M.pairs_that_differ(g, g, 0)
    assert (same == 0).all()
    g2 = g.copy()
    g2[3, 7, 2] += 1                                                  # pair (3, 7), group 2 -- and (7, 3), which is below the diagonal
    g2[7, 3, 1] += 1
    assert M.pairs_that_differ(g, g2, 0).tolist() == [0, 0, 1, 0]
    assert M.ut_offsets(N)[-1] == N * (N - 1) // 2 and M.ut_offsets(N)[1] == N - 1


def test_sequences_are_what_the_docstring_says():
    mats = M.sequence(200, 64, 4, 1, M.PLANTED_KINDS)
    for t, (m, (_, nvals)) in enumerate(zip(mats, M.PLANTED_KINDS)):
        per_col = [np.unique(m[:, c][m[:, c] != 0]).size for c in range(64)]
        assert max(per_col) <= nvals and ((m == 0).any() == (t % 2 == 0))
    fam, one, fam2, pl = M.sequence(400, 64, 4, 2, M.FAMILY_KINDS)
    # one_family: the most frequent value of every column is held by about half of the sketches; families: by about 0.7 x 40 of them
    top = lambda m: np.array([np.unique(m[:, c], return_counts=True)[1].max() for c in range(m.shape[1])])
    assert top(one).min() > 150 and 10 <= top(fam).min() and top(fam).max() < 80 and top(pl).min() > 100
    assert M.shared_patterns(fam, fam2) == 0
    assert [a is not b and np.array_equal(a, b) for a, b in zip(mats, M.sequence(200, 64, 4, 1, M.PLANTED_KINDS))] == [True] * 4   # same seed, same stream


@pytest.mark.parametrize("W,N,S", M.STREAM_SHAPES)
def test_planted_stream_meets_p1_p2_p3(d2g, capsys, W, N, S):
    mats = M.sequence(N, S, M.STREAM_T, M.seed_of(W, N, S), M.PLANTED_KINDS)
    p1, p2, p3 = _figures(d2g, mats, W, min_pairs=100, min_frac=0.90)
    _show(capsys, f"planted W={W} N={N} S={S} T={M.STREAM_T}: P1 shared patterns {p1}, P2 min pairs {p2[0]} (step {p2[1]}, group {p2[2]}, rank {p2[3]}), P3 min fraction {p3:.4f}")


@pytest.mark.parametrize("W,N,S", M.FAMILY_SHAPES)
def test_family_stream_meets_p1_p2_p3(d2g, capsys, W, N, S):
    mats = M.sequence(N, S, M.FAMILY_T, M.seed_of(W, N, S), M.FAMILY_KINDS)
    p1, p2, p3 = _figures(d2g, mats, W, min_pairs=1, min_frac=0.01, witness_rows=M.FAMILY_WITNESS_ROWS)
    _show(capsys, f"families W={W} N={N} S={S} T={M.FAMILY_T}: P1 shared patterns {p1}, P2 min pairs >= {p2[0]} (step {p2[1]}, group {p2[2]}, rank {p2[3]}; first "
                  f"{M.FAMILY_WITNESS_ROWS} rows of every slab), P3 min fraction {p3:.4f}")


def test_overflow_then_clean_meets_p1_p2_p3(d2g, capsys):
    W, N, S = M.OVERFLOW_SHAPE
    mats = M.overflow_then_clean(N, S, M.seed_of(W, N, S))
    assert all(np.unique(mats[0][:, c]).size == N for c in range(64)) and all(np.unique(mats[0][:, c]).size == 1 for c in range(64, S))
    p1, p2, p3 = _figures(d2g, mats, W, min_pairs=100, min_frac=0.90, witness_rows=M.FAMILY_WITNESS_ROWS)
    _show(capsys, f"overflow, then clean W={W} N={N} S={S}: P1 shared patterns {p1}, P2 min pairs >= {p2[0]} (group {p2[2]}, rank {p2[3]}; first "
                  f"{M.FAMILY_WITNESS_ROWS} rows of every slab), P3 min fraction {p3:.4f}")
