"""The model of the bounded edit-distance routes (K2i, d2g_edit_near.hip), on top of edit_ref's dynamic programme.

closeness(d, T) = T + 1 - min(d, T + 1): what d2g_edit_near_dev writes.  within_lists: what d2g_edit_knn returns -- per row the
other records (self excluded by index) sorted by (distance, id), either all of those with d <= T (threshold mode, K == 0) or the K
smallest distances over ALL other records with every tie of the K-th (top-K mode).  topk_lists_from states the top-K lists the way the
library reaches them, from a starting bound that doubles for the rows that are short: the result must not depend on the start.
band_distance is a plain-Python restatement of the diagonal-band recurrence the band kernel runs (Hyyro 2003), 64-bit words."""
import numpy as np

import edit_ref as E

M64 = (1 << 64) - 1


def closeness(d, T):
    return T + 1 - np.minimum(np.asarray(d, np.int64), T + 1)


def _row_list(drow, i, keep):
    js = [j for j in range(len(drow)) if j != i and keep(int(drow[j]))]
    return sorted(js, key=lambda j: (int(drow[j]), j))


def _topk(drow, i, K, bound):
    """the K nearest among those with d <= bound, with every tie of the K-th"""
    js = _row_list(drow, i, lambda d: d <= bound)
    if len(js) > K:
        kth = int(drow[js[K - 1]])
        js = [j for j in js if int(drow[j]) <= kth]
    return js


def topk_lists_from(d, K, start, maxlen):
    """top-K lists as the library finds them: bound = start; a row with fewer than min(K, N - 1) entries runs again with 2 bound + 1,
    until the bound reaches the longest record (every distance is at most that)"""
    n = d.shape[0]
    out = []
    for i in range(n):
        b = min(start, maxlen)
        while True:
            js = _topk(d[i], i, K, b)
            if len(js) >= min(K, n - 1) or b >= maxlen:
                break
            b = min(2 * b + 1, maxlen)
        out.append(js)
    return out


def within_lists(records, K, T, d=None):
    """-> (lists, d): lists[i] = the neighbours of record i by (distance, id); K == 0: those with d <= T; K >= 1: the K nearest of all"""
    d = E.edit_matrix(records) if d is None else d
    n = d.shape[0]
    if K == 0:
        return [_row_list(d[i], i, lambda x: x <= T) for i in range(n)], d
    big = int(d.max()) + 1
    return [_topk(d[i], i, K, big) for i in range(n)], d


def csr_of(lists, d, r0=0, r1=None):
    """(indptr u64, indices u32, data f32) of rows [r0, r1) of the lists"""
    r1 = len(lists) if r1 is None else r1
    indptr = np.zeros(r1 - r0 + 1, np.uint64)
    idx, val = [], []
    for i in range(r0, r1):
        idx += lists[i]
        val += [float(d[i, j]) for j in lists[i]]
        indptr[i - r0 + 1] = len(idx)
    return indptr, np.array(idx, np.uint32), np.array(val, np.float32)


def band_distance(q, t, mx):
    """min(d(q, t), mx + 1) by the band recurrence: q is the query (its match bits are the table), t the column record whose symbols
    are walked, mx <= 31 the bound"""
    q, t = E.as_bytes(q), E.as_bytes(t)
    len1, len2 = int(q.size), int(t.size)
    assert 0 <= mx <= 31
    if abs(len1 - len2) > mx:
        return mx + 1
    if len1 == 0 or len2 == 0:
        return max(len1, len2)
    pm = {}
    for r, ch in enumerate(q.tolist()):
        pm[ch] = pm.get(ch, 0) | (1 << r)
    VP, VN, start = (M64 << (63 - mx)) & M64, 0, mx - 63
    cur, diag, hor = min(mx, len1), 1 << 63, 1 << (62 - max(0, mx - len1))
    brk = 2 * mx + len2 - len1
    for i, ch in enumerate(t.tolist()):
        p = pm.get(ch, 0)
        X = ((p << -start) if start < 0 else (p >> start)) & M64
        D0 = ((((X & VP) + VP) & M64) ^ VP) | X | VN
        HP = VN | (~(D0 | VP) & M64)
        HN = D0 & VP
        if i < len1 - mx:
            cur += 0 if D0 & diag else 1
        else:
            cur += (1 if HP & hor else 0) - (1 if HN & hor else 0)
            hor >>= 1
        if cur > brk:
            return mx + 1
        VP = HN | (~((D0 >> 1) | HP) & M64)
        VN = (D0 >> 1) & HP
        start += 1
    return cur if cur <= mx else mx + 1
