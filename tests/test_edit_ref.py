"""edit_ref (the NumPy dynamic programme the GPU tests compare with) pinned to the reference: it returns what the reference's own edlib
returned for every pair of tests/golden/edit_edlib_pairs.json, and the known answers of pairs made by construction."""
import json
import os

import numpy as np
import pytest

import edit_ref as E
from conftest import GOLDEN


def _decode(x):
    return bytes.fromhex(x["hex"]) if isinstance(x, dict) else x.encode("ascii")


@pytest.fixture(scope="module")
def pairs():
    with open(os.path.join(GOLDEN, "edit_edlib_pairs.json")) as f:
        doc = json.load(f)
    assert "edlib" in doc["provenance"]
    return [(p["what"], _decode(p["a"]), _decode(p["b"]), p["d"]) for p in doc["pairs"]]


def test_the_fixture_covers_the_seams(pairs):
    assert len(pairs) >= 180
    seams = {0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049}
    assert seams <= {len(a) for _, a, _, _ in pairs} and seams <= {len(b) for _, _, b, _ in pairs}
    assert max(max(len(a), len(b)) for _, a, b, _ in pairs) <= 2100
    assert any(len(set(a) | set(b)) == 256 for _, a, b, _ in pairs)                   # all 256 byte values
    assert any(len(set(a) | set(b)) == 1 and a != b for _, a, b, _ in pairs)          # sigma = 1
    assert any(a.lower() == b.lower() and a != b for _, a, b, _ in pairs)             # mixed case
    assert ("mixed case", b"ACGT", b"acgt", 4) in pairs and ("empty", b"", b"abc", 3) in pairs


def test_dp_equals_every_recorded_edlib_distance(pairs):
    bad = [(i, w, len(a), len(b), d, E.edit_distance(a, b)) for i, (w, a, b, d) in enumerate(pairs) if E.edit_distance(a, b) != d]
    assert not bad, bad[:5]


def test_dp_is_symmetric_on_the_fixture(pairs):
    for _, a, b, d in pairs[::7]:
        assert E.edit_distance(b, a) == d


def test_inserted_symbols_give_exactly_their_number():
    rng = np.random.default_rng(7001)
    for n, d in [(1, 1), (31, 2), (64, 33), (200, 70), (1000, 5)]:
        x = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())
        y = bytearray(x)
        for _ in range(d):
            y.insert(int(rng.integers(len(y) + 1)), int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
        assert len(y) - len(x) == d                                                  # length difference <= distance <= d insertions
        assert E.edit_distance(x, bytes(y)) == d


def test_disjoint_alphabets_give_the_longer_length():
    for m, n in [(0, 5), (1, 1), (33, 32), (64, 200), (300, 7)]:
        assert E.edit_distance(b"AC" * (m // 2) + b"A" * (m % 2), b"gt" * (n // 2) + b"g" * (n % 2)) == max(m, n)


def test_one_letter_gives_the_length_difference_and_equal_records_zero():
    for m, n in [(0, 0), (1, 64), (32, 33), (65, 31), (300, 300)]:
        assert E.edit_distance(b"a" * m, b"a" * n) == abs(m - n)
    rng = np.random.default_rng(7002)
    x = bytes(rng.integers(0, 256, 700, dtype=np.uint8).tolist())
    assert E.edit_distance(x, x) == 0 and E.edit_distance(x, x[:-1]) == 1


def test_matrix_and_triangle_helpers():
    recs = [b"kitten", b"sitting", b"", b"kitten"]
    d = E.edit_matrix(recs)
    assert d.tolist() == [[0, 3, 6, 0], [3, 0, 7, 3], [6, 7, 0, 6], [0, 3, 6, 0]]
    assert E.triangle(d).tolist() == [3, 6, 0, 7, 3, 6] and E.triangle(d, 1, 3).tolist() == [7, 3, 6] and E.triangle(d, 3, 4).size == 0
