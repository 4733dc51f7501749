"""edit_within_ref (the model the GPU tests of K2i compare with): its clamp pinned to the reference's recorded edlib distances, its
restatement of the band recurrence against the dynamic programme at the word seams, and top-K lists that do not depend on the bound the
search starts from."""
import itertools
import json
import os

import numpy as np
import pytest

import edit_ref as E
import edit_within_ref as W
from conftest import GOLDEN


def _decode(x):
    return bytes.fromhex(x["hex"]) if isinstance(x, dict) else x.encode("ascii")


def test_closeness_is_the_clamped_distance():
    assert W.closeness([0, 1, 3, 4, 5, 900], 3).tolist() == [4, 3, 1, 0, 0, 0]
    assert W.closeness([0, 1], 0).tolist() == [1, 0]


def test_clamp_of_the_recorded_edlib_distances():
    with open(os.path.join(GOLDEN, "edit_edlib_pairs.json")) as f:
        doc = json.load(f)
    pairs = [(_decode(p["a"]), _decode(p["b"]), p["d"]) for p in doc["pairs"]]
    assert len(pairs) == 185
    ours = np.array([E.edit_distance(a, b) for a, b, _ in pairs])
    theirs = np.array([d for _, _, d in pairs])
    for T in (0, 1, 31, 32, 2049):
        np.testing.assert_array_equal(W.closeness(ours, T), W.closeness(theirs, T), err_msg=f"T = {T}")
        assert W.closeness(theirs, T).max() <= T + 1 and W.closeness(theirs, T).min() >= 0


LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 150]
BOUNDS = [0, 1, 2, 15, 30, 31]


def _mutated(rng, x, edits, alphabet):
    y = list(x)
    for _ in range(edits):
        op = int(rng.integers(3))
        if op == 0 and y:
            y[int(rng.integers(len(y)))] = int(rng.choice(alphabet))
        elif op == 1 and y:
            del y[int(rng.integers(len(y)))]
        else:
            y.insert(int(rng.integers(len(y) + 1)), int(rng.choice(alphabet)))
    return bytes(y)


def test_band_recurrence_equals_the_clamped_dp_at_the_seams():
    """query shorter than, equal to and longer than the column: every length against its mutations (a few edits: inside the band; many:
    outside) and against an unrelated record of every other length that the length filter lets through or not"""
    rng = np.random.default_rng(8100)
    alphabet = np.frombuffer(b"ACGT", np.uint8)
    cases = 0
    seen = set()
    for n in LENGTHS:
        q = bytes(rng.choice(alphabet, n).tolist())
        others = [q, bytes(rng.choice(alphabet, n).tolist())]
        others += [_mutated(rng, q, e, alphabet) for e in (1, 2, 3, 8, 16, 31, 40)]
        others += [q[:k] for k in (n - 1, n - 2, n - 31, n - 32) if k >= 0] + [q + q[:k] for k in (1, 2, 31, 32) if k <= n]
        others += [bytes(rng.choice(alphabet, k).tolist()) for k in LENGTHS]
        for t in others:
            d = E.edit_distance(q, t)
            for T in BOUNDS:
                want = min(d, T + 1)
                assert W.band_distance(q, t, T) == want, (len(q), len(t), T, d)
                assert W.band_distance(t, q, T) == want, (len(t), len(q), T, d)
                cases += 2
                seen.add((np.sign(len(q) - len(t)), want <= T))
    assert cases > 2000 and len(seen) == 6                     # shorter / equal / longer, each inside and outside the bound


def test_band_recurrence_on_other_alphabets():
    rng = np.random.default_rng(8101)
    for alphabet in (np.frombuffer(b"a", np.uint8), np.arange(256, dtype=np.uint8)):
        for n, T in itertools.product([1, 33, 64, 150], [0, 2, 31]):
            q = bytes(rng.choice(alphabet, n).tolist())
            for t in (q, _mutated(rng, q, T, alphabet), _mutated(rng, q, T + 3, alphabet), q[: max(0, n - T)]):
                assert W.band_distance(q, t, T) == min(E.edit_distance(q, t), T + 1)


@pytest.fixture(scope="module")
def family():
    rng = np.random.default_rng(8102)
    alphabet = np.frombuffer(b"ACGT", np.uint8)
    roots = [bytes(rng.choice(alphabet, n).tolist()) for n in (40, 44, 60)]
    recs = []
    for r in roots:
        recs += [r, r] + [_mutated(rng, r, e, alphabet) for e in (1, 2, 2, 4, 7)]
    recs.append(b"")
    return recs, E.edit_matrix(recs)


def test_threshold_lists(family):
    recs, d = family
    n = len(recs)
    for T in (0, 2, 5):
        lists, _ = W.within_lists(recs, 0, T, d)
        for i, js in enumerate(lists):
            assert i not in js and set(js) == {j for j in range(n) if j != i and d[i, j] <= T}
            assert [(d[i, j], j) for j in js] == sorted((d[i, j], j) for j in js)
        assert 0 < sum(map(len, lists)) < n * (n - 1)
    assert 1 in W.within_lists(recs, 0, 0, d)[0][0]            # duplicates list each other


def test_topk_keeps_the_ties_of_the_kth(family):
    recs, d = family
    n = len(recs)
    for K in (1, 3, n - 1, n + 5):
        lists, _ = W.within_lists(recs, K, 0, d)
        for i, js in enumerate(lists):
            others = sorted(int(d[i, j]) for j in range(n) if j != i)
            kth = others[min(K, n - 1) - 1]
            assert set(js) == {j for j in range(n) if j != i and d[i, j] <= kth}
            assert len(js) >= min(K, n - 1)
    ip, ix, dt = W.csr_of(W.within_lists(recs, 1, 0, d)[0], d)
    assert ip[-1] == ix.size == dt.size and dt.dtype == np.float32 and ip[1] >= 1


def test_topk_does_not_depend_on_the_starting_bound(family):
    recs, d = family
    maxlen = max(len(r) for r in recs)
    for K in (1, 3, len(recs) - 1, len(recs) + 5):
        want, _ = W.within_lists(recs, K, 0, d)
        for start in (0, 1, 40):
            assert W.topk_lists_from(d, K, start, maxlen) == want, (K, start)
