"""Inputs shared by the truncated-register tests (host, GPU, CLI): signature matrices in the shapes the truncation can get wrong,
and code matrices with the orders a bit-serial comparator can get wrong."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def oph_shaped(rng, N, S, families=4, unrelated=8, empty_rows=0, scale_spread=3.0):
    """densified-OPH-like signatures: positive doubles, exponential within a row and scaled by 1/cardinality; rows of a family share
    most registers; `unrelated` rows share none; `empty_rows` rows are all zero (sketches of inputs without k-mers).
    -> (sigs [N][S], cards [N])"""
    cards = 10.0 ** rng.uniform(3, 3 + scale_spread, N)
    fam = rng.integers(0, families, N)
    fam_card = 10.0 ** rng.uniform(3, 3 + scale_spread, families)
    base = rng.exponential(1.0, (families, S)) / fam_card[:, None]
    own = rng.random((N, S)) < rng.uniform(0.02, 0.6, (N, 1))
    sigs = np.where(own, rng.exponential(1.0, (N, S)) / cards[:, None], base[fam])
    cards = np.where(own.mean(axis=1) < 0.3, fam_card[fam] * rng.uniform(0.8, 1.25, N), cards)
    u = rng.choice(N, min(unrelated, N), replace=False)
    sigs[u] = rng.exponential(1.0, (u.size, S)) / cards[u, None]
    if empty_rows:
        e = rng.choice(np.setdiff1d(np.arange(N), u), empty_rows, replace=False)
        sigs[e] = 0.0
        cards[e] = 0.0
    if N > 4:
        cards[1] = cards[0]                      # equal cardinalities
    assert (sigs >= 0).all() and np.isfinite(sigs).all()
    return np.ascontiguousarray(sigs), cards


def wide_range(rng, N, S):
    """a dynamic range above 1e12, with registers at DBL_MAX (skipped by the min/max scan, still coded) and zeros"""
    sigs = np.exp(rng.uniform(-40.0, -2.0, (N, S)))
    sigs[rng.random((N, S)) < 0.02] = 0.0
    sigs[rng.random((N, S)) < 0.01] = DBL_MAX
    assert sigs[(sigs > 0) & (sigs < DBL_MAX)].max() / sigs[sigs > 0].min() > 1e12
    return sigs


def exp_over_1024(rng, N, S):
    """exponential registers scaled by 1/1024 with the extremes planted several times: the registers equal to minreg and maxreg sit on
    the seam of the code range (the last bit of logl decides between the top code and the one below)"""
    sigs = rng.exponential(1.0, (N, S)) / 1024.0
    flat = sigs.reshape(-1)
    lo, hi = flat.min(), flat.max()
    pos = rng.choice(flat.size, 12, replace=False)
    flat[pos[:6]] = lo
    flat[pos[6:]] = hi
    flat[rng.choice(flat.size, 6, replace=False)] = np.nextafter(lo, 1.0)
    flat[rng.choice(flat.size, 6, replace=False)] = np.nextafter(hi, 0.0)
    return sigs


def gen_codes(rng, N, S, dtype):
    """N x S codes of one width: columns with few distinct values (many equal, many ordered pairs), full-range rows, neighbours that
    differ in the lowest or the highest bit only, zeros against the largest code, and for the wider codes rows that agree in the high
    bytes and differ in the low ones, and the reverse"""
    P = 8 * np.dtype(dtype).itemsize
    top = (1 << P) - 1
    vals = rng.integers(0, top + 1, (4, S), dtype=np.uint64)
    m = vals[rng.integers(0, 4, (N, S)), np.arange(S)[None, :]]
    full = rng.random(N) < 0.3
    m[full] = rng.integers(0, top + 1, (int(full.sum()), S), dtype=np.uint64)
    k = N // 16
    if k:
        idx = rng.permutation(N)[:14 * k].reshape(14, k)
        a = m[idx[0::2]]                                                    # [7][k][S]
        half = rng.random(a.shape[1:]) < 0.5
        m[idx[1]] = a[0]                                                    # identical rows
        lowc = np.minimum(a[1], np.uint64(top - 1))
        m[idx[2]], m[idx[3]] = lowc, lowc + np.uint64(1)                    # one row above the other in every register
        m[idx[5]] = np.where(half, a[2], a[2] ^ np.uint64(1))               # lowest bit only
        m[idx[7]] = np.where(half, a[3], a[3] ^ np.uint64(1 << (P - 1)))    # highest bit only
        m[idx[8]], m[idx[9]] = 0, top                                       # 0 against the largest code
        lo_mask = np.uint64((1 << (P // 2)) - 1)
        hi_mask = np.uint64(top) ^ lo_mask
        m[idx[11]] = (a[5] & hi_mask) | (rng.integers(0, top + 1, a[5].shape, dtype=np.uint64) & lo_mask)    # high half equal
        m[idx[13]] = (a[6] & lo_mask) | (rng.integers(0, top + 1, a[6].shape, dtype=np.uint64) & hi_mask)    # low half equal
    return np.ascontiguousarray(m.astype(dtype))
