"""The record families of the edit-distance clustering tests (K2j), each with its distance matrix, built once per process.
test_edit_dedup_ref.py checks the model on them, test_gpu_edit_dedup.py the device."""
import functools

import numpy as np

import edit_dedup_ref as R
import edit_ref as E

SEAMS = [1, 31, 32, 33, 63, 64, 65, 96, 150, 257]
DNA = np.frombuffer(b"ACGT", np.uint8)


def mutated(rng, x, edits, alphabet):
    y = list(x)
    for _ in range(edits):
        op = int(rng.integers(3))
        if op == 0 and y:
            y[int(rng.integers(len(y)))] = int(rng.choice(alphabet))
        elif op == 1 and len(y) > 1:
            del y[int(rng.integers(len(y)))]
        else:
            y.insert(int(rng.integers(len(y) + 1)), int(rng.choice(alphabet)))
    return bytes(y)


@functools.lru_cache(maxsize=None)
def seam_family():
    """the 70 records of test_gpu_edit_within.py's seam family (its generator, copied): prefixes of one base at the seam lengths, each
    twice and with 1, 2, 16, 31 and 34 random edits, shuffled"""
    rng = np.random.default_rng(8200)
    base = bytes(rng.choice(DNA, 300).tolist())
    recs = []
    for n in SEAMS:
        recs += [base[:n], base[:n]] + [mutated(rng, base[:n], e, DNA) for e in (1, 2, 16, 31, 34)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    return recs, E.edit_matrix(recs)


def walks(rng, nwalks, steps, lo, hi):
    """nwalks walks of `steps` records, each one edit from the one before, from a random DNA record of lo .. hi symbols; shuffled"""
    recs = []
    for _ in range(nwalks):
        x = bytes(rng.choice(DNA, int(rng.integers(lo, hi + 1))).tolist())
        for _ in range(steps):
            recs.append(x)
            x = mutated(rng, x, 1, DNA)
    return [recs[i] for i in rng.permutation(len(recs))]


@functools.lru_cache(maxsize=None)
def chains():
    """300 records: a record's neighbours along its walk are one edit away, the walk's ends up to 50"""
    recs = walks(np.random.default_rng(77), 6, 50, 40, 60)
    return recs, R.edit_matrix_batch(recs)


@functools.lru_cache(maxsize=None)
def band_family():
    """the first 513 records of 11 walks of 50 steps from records of 20 .. 30 symbols; the tests take the first N of them"""
    recs = walks(np.random.default_rng(513), 11, 50, 20, 30)[:513]
    return recs, R.edit_matrix_batch(recs)


@functools.lru_cache(maxsize=None)
def ragged():
    """120 records: 30 bases of 10 .. 200 symbols, each with 1, 2 and 5 edits"""
    rng = np.random.default_rng(9)
    recs = []
    for _ in range(30):
        x = bytes(rng.choice(DNA, int(rng.integers(10, 201))).tolist())
        recs += [x] + [mutated(rng, x, e, DNA) for e in (1, 2, 5)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    return recs, R.edit_matrix_batch(recs)


@functools.lru_cache(maxsize=None)
def mixed():
    """40 records: DNA of 9 .. 32 and of 100 .. 150 symbols in families, interleaved, with two records of 2 000 symbols over 256 byte
    values three edits apart (sigma = 256: their match table does not fit in LDS, the all-columns route beside the list kernel)"""
    rng = np.random.default_rng(4100)
    recs = []
    for k in range(19):
        lo, hi = ((9, 32), (100, 150))[k & 1]
        x = bytes(rng.choice(DNA, int(rng.integers(lo, hi + 1))).tolist())
        recs += [x, mutated(rng, x, int(rng.integers(1, 10)), DNA)]
    big = bytes(rng.integers(0, 256, 2000, dtype=np.int64).astype(np.uint8).tolist())
    recs = [recs[i] for i in rng.permutation(len(recs))]
    recs.insert(7, big)
    recs.insert(29, mutated(rng, big, 3, np.arange(256, dtype=np.uint8)))
    return recs, E.edit_matrix(recs)


RANDOM_SEED = 20261
RANDOM_SETS = 200


@functools.lru_cache(maxsize=None)
def random_sets():
    """RANDOM_SETS of (records, T, band_rows): N <= 48, lengths <= 40, alphabets of 2 .. 4 letters, T in 0 .. 6"""
    rng = np.random.default_rng(RANDOM_SEED)
    out = []
    for _ in range(RANDOM_SETS):
        n = int(rng.integers(1, 49))
        alphabet = DNA[:int(rng.integers(2, 5))]
        nbase = int(rng.integers(1, 6))
        bases = [bytes(rng.choice(alphabet, int(rng.integers(0, 35))).tolist()) for _ in range(nbase)]
        recs = [mutated(rng, bases[int(rng.integers(nbase))], int(rng.integers(0, 6)), alphabet)[:40] for _ in range(n)]
        out.append((recs, int(rng.integers(0, 7)), int(rng.choice([0, 1, 3, 7, 16, 32, 47]))))
    return out


@functools.lru_cache(maxsize=None)
def random_matrices():
    return [E.edit_matrix(recs) for recs, _, _ in random_sets()]
