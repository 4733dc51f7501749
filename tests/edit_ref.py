"""Levenshtein distance over bytes, row by row in NumPy: the yardstick of the edit-distance kernel (K2h).

Independent of Myers' bit-vector algorithm: the classic dynamic programme D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1,
D[i-1][j-1] + (a[i] != b[j])), one row of the table at a time.  The two terms that come from the row above are taken elementwise;
the third runs ALONG the row, D[i][j] = min_k<=j (t[k] + (j - k)), and is resolved with a prefix minimum of t[k] - k
(np.minimum.accumulate), so a row costs a few vector operations.  Unit costs, no case folding, every byte value its own symbol:
what edlib's global distance mode returns for the same bytes (tests/golden/edit_edlib_pairs.json pins that)."""
import numpy as np


def as_bytes(x):
    if isinstance(x, str):
        x = x.encode("latin-1")
    return np.frombuffer(bytes(x), np.uint8)


def edit_distance(a, b):
    a, b = as_bytes(a), as_bytes(b)
    if a.size > b.size:
        a, b = b, a                                    # symmetric; the longer one along the row, so the Python loop is the short one
    n = b.size
    if n == 0:
        return int(a.size)
    idx = np.arange(n + 1, dtype=np.int64)
    row = idx.copy()                                   # D[0][j] = j
    for i in range(a.size):
        t = np.empty(n + 1, np.int64)
        t[0] = i + 1
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i]))
        row = np.minimum.accumulate(t - idx) + idx
    return int(row[n])


def edit_matrix(records):
    """the full symmetric matrix of a list of byte strings, int64 [N][N]"""
    n = len(records)
    d = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = edit_distance(records[i], records[j])
    return d


def triangle(d, r0=0, r1=None):
    """rows [r0, r1) of the strict upper triangle of a square matrix, packed row by row"""
    n = d.shape[0]
    r1 = n if r1 is None else r1
    return np.concatenate([d[i, i + 1:] for i in range(r0, r1)] + [np.empty(0, d.dtype)])
