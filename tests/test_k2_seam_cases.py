"""The generator of the K2 seam tests (k2_seam_cases.py) is test infrastructure: its label counts and its D2 per column -- both computed
from the recipe -- are pinned here against the matrix it returns, on shapes small enough for a whole-triangle broadcast compare of
the uint64 values, and (for the pools without special values) against the oracle.  No GPU."""
import numpy as np
import pytest

import k2_seam_cases as kc

SHAPES = [(300, 100), (299, 33), (64, 32), (7, 5)]


def _broadcast_counts(m):
    """equal 64-bit patterns per pair, whole triangle, condensed: the ten-line restatement that looks at the VALUES"""
    N, S = m.shape
    out = []
    for i in range(N - 1):
        out.append((m[i + 1:] == m[i]).sum(axis=1, dtype=np.int64))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def _d2_from_values(m):
    return np.array([(np.unique(m[:, t], return_counts=True)[1] >= 2).sum() for t in range(m.shape[1])], np.int64)


def _recipes(N):
    r = [kc.distinct, kc.pairs, kc.constant]
    if N >= 4:
        r.append(kc.two_values)
    for b in range(1, 8):
        for d in (2 ** b - 2, 2 ** b - 1, 2 ** b):
            if d >= 1 and 2 * d + 1 <= N:
                r.append(kc.shared(d, 2))
    if N >= 40:
        r.append(kc.shared(5, [N // 3, 2, 3, 2, 7]))
    return r


def _pin(case, oracle, plain):
    m = case.matrix
    N, S = m.shape
    assert m.dtype == np.uint64 and case.labels.shape == (S, N) and case.labels.dtype == np.int32
    want = _broadcast_counts(m)
    np.testing.assert_array_equal(case.counts_ut(), want)
    assert case.counts_ut().dtype == np.int64
    np.testing.assert_array_equal(case.d2, _d2_from_values(m))
    for t in range(S):                                                 # the labels name the values: label k <-> shared[t][k], -1 <-> held once
        lab = case.labels[t]
        assert case.shared[t].size == case.d2[t] == lab.max() + 1
        np.testing.assert_array_equal(m[lab >= 0, t], case.shared[t][lab[lab >= 0]])
        assert np.unique(m[lab < 0, t]).size == int((lab < 0).sum())
        assert not np.isin(m[lab < 0, t], case.shared[t]).any()
    # row ranges and rectangles are cuts of the same counts
    off = kc.ut_offsets(N)
    for r0, r1 in ((0, 1), (N // 2, N // 2 + 3), (N - 2, N), (N - 1, N), (1, N)):
        np.testing.assert_array_equal(case.counts_ut(r0, r1), want[off[r0]:off[r1]])
    full = np.zeros((N, N), np.int64)
    full[np.triu_indices(N, 1)] = want
    full += full.T + S * np.eye(N, dtype=np.int64)
    for a0, a1, b0, b1 in ((0, N, 0, N), (2, 5, 1, N - 1), (N - 3, N, 0, 2)):
        np.testing.assert_array_equal(case.counts_rect(a0, a1, b0, b1), full[a0:a1, b0:b1])
    if plain:
        f = m.view(np.float64)
        assert not np.isnan(f).any() and not (f == 0.0).any()
        np.testing.assert_array_equal(oracle.eqcounts_ut(f), want)


@pytest.mark.parametrize("pool", kc.POOLS)
@pytest.mark.parametrize("N,S", SHAPES)
def test_uniform_matrices_of_every_recipe_and_pool(oracle, N, S, pool):
    for k, rec in enumerate(_recipes(N)):
        if rec.name == "constant" and N < 2:
            continue
        case = kc.uniform(N, S, rec, pool, seed=1000 * N + k)
        assert (case.d2 == rec.reps(N).size).all() and all(p == pool for p in case.pools)
        _pin(case, oracle, pool in kc.PLAIN_POOLS)


@pytest.mark.parametrize("pools", [kc.PLAIN_POOLS, kc.POOLS, ("specials", "twins")])
@pytest.mark.parametrize("N,S", SHAPES[:3])
def test_striped_matrices(oracle, N, S, pools):
    recs = [kc.distinct, kc.pairs, kc.constant, kc.two_values, kc.shared(2 ** 4 - 1, 2)]
    case = kc.striped(N, S, recs, pools, seed=N + S)
    for t in range(S):
        assert case.recipes[t] is recs[t % 5] and case.pools[t] == pools[(t // 5) % len(pools)]
    _pin(case, oracle, "specials" not in pools)
    # the operand's groups, columns in the caller's order: the maximum of the recipes' D2 over every 32 columns
    gm = case.group_max_d2()
    assert gm.tolist() == [max(recs[t % 5].reps(N).size for t in range(g, min(g + 32, S))) for g in range(0, S, 32)]
    md, nb, mean = case.planes_expected(sorted_columns=False)
    bl = [int(x + 1).bit_length() for x in gm]
    assert md == N // 2 + 1 and nb == (N // 2 + 1).bit_length() and mean == np.float32(sum(bl) / len(bl))   # (a `pairs` column in the first group)
    assert case.planes_expected(sorted_columns=True)[:2] == (md, nb)


@pytest.mark.parametrize("pool", ["random", "specials"])
@pytest.mark.parametrize("N,S", SHAPES[:3])
def test_one_busy_column_per_group(oracle, N, S, pool):
    case = kc.one_busy_column_per_group(N, S, kc.shared(13, 3), pool=pool, seed=S)
    _pin(case, oracle, pool != "specials")
    assert case.group_max_d2().tolist() == [13] * -(-S // 32)
    assert np.flatnonzero(case.d2).tolist() == [32 * g + (7 * g + 3) % min(32, S - 32 * g) for g in range(-(-S // 32))]
    # sorted, the busy columns share the first group
    md, nb, mean = case.planes_expected(sorted_columns=True)
    ng = -(-S // 32)
    assert (md, nb) == (14, 4) and mean == np.float32((4 + (ng - 1)) / ng)


def test_the_specials_reach_shared_labels_and_unique_sketches():
    """column t deals SPECIALS from SPECIALS[t % 10] on: in turn the value of label 0, of a unique sketch, of label 1, ...: over ten
    columns every special value is once the value of label 0 -- in column 1 that is ~0, an EMPTY register, held by a third of the sketches"""
    N, S = 300, 33
    case = kc.uniform(N, S, kc.shared(5, [N // 3, 2, 3, 2, 7]), "specials", seed=3)
    for t in range(S):
        sp = [kc.SPECIALS[(t + k) % 10] for k in range(10)]
        assert case.shared[t].tolist() == sp[0::2]
        col, lab = case.matrix[:, t], case.labels[t]
        assert int((lab == 0).sum()) == N // 3 and (col[lab == 0] == np.uint64(sp[0])).all()
        for s in sp[1::2]:
            assert int((col == np.uint64(s)).sum()) == 1 and lab[col == np.uint64(s)][0] == -1
    assert int(case.shared[1][0]) == kc.M64
    d = kc.uniform(N, S, kc.distinct, "specials", seed=4)              # no shared label: all ten go to unique sketches
    for t in range(S):
        assert all(int((d.matrix[:, t] == np.uint64(s)).sum()) == 1 for s in kc.SPECIALS)


def test_twins_agree_in_one_half_only():
    v = kc.pool_values("twins", 200, np.random.default_rng(1))
    hi, lo = v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)
    assert np.unique(v).size == 200
    assert np.unique(hi, return_counts=True)[1].max() == 100 and np.unique(lo, return_counts=True)[1].max() == 100
    assert (kc.pool_values("low_only", 50, np.random.default_rng(2)) >> np.uint64(32) == 0).all()
    assert (kc.pool_values("high_only", 50, np.random.default_rng(2)) & np.uint64(0xFFFFFFFF) == 0).all()


def test_recipes_refuse_what_does_not_fit():
    with pytest.raises(ValueError):
        kc.uniform(9, 2, kc.shared(5, 2))
    with pytest.raises(ValueError):
        kc.uniform(3, 2, kc.two_values)
    assert kc.pairs.reps(7).tolist() == [2, 2, 3] and kc.pairs.reps(1).size == 0 and kc.constant.reps(1).size == 0
