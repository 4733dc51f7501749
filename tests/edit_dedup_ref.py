"""The model of greedy clustering by edit distance (K2j, d2g_edit_dedup.hip), NumPy / Python only.

The rule: records in input order; record i joins the representative r < i with the smallest d(i, r), among equal distances the
smallest r, if that distance is <= T, and founds a cluster (assign[i] = i) otherwise.  A record is compared with representatives only.

greedy_assign       the rule over a full distance matrix (edit_ref.edit_matrix), vectorised per record
greedy_assign_loop  the same, pair by pair over (distance, representative) tuples: the checker's checker
edit_matrix_batch   the distance matrix with edit_ref's recurrence run over all targets of a record at once (the families of several
                    hundred records; test_edit_dedup_ref.py holds it against edit_ref.edit_matrix)
census              what a case exercises
"""
import numpy as np

import edit_ref as E


def greedy_assign(d, T):
    d = np.asarray(d, np.int64)
    n = d.shape[0]
    assign = np.arange(n, dtype=np.uint32)
    reps = []
    for i in range(n):
        if reps:
            v = d[i, reps]
            c = int(np.argmin(v))                       # the smallest distance; the first of equal ones = the smallest representative
            if v[c] <= T:
                assign[i] = reps[c]
                continue
        reps.append(i)
    return assign


def greedy_assign_loop(d, T):
    n = len(d)
    assign = [0] * n
    for i in range(n):
        best = None
        for r in range(i):
            if assign[r] != r:
                continue
            cand = (int(d[i][r]), r)
            if best is None or cand < best:
                best = cand
        assign[i] = best[1] if best is not None and best[0] <= T else i
    return np.array(assign, np.uint32)


def edit_matrix_batch(records):
    """int64 [N][N]; row i: record i against every later record at once, the targets padded to one length with a symbol no record has
    (the table's columns behind a target's end do not reach the column that holds its distance)"""
    n = len(records)
    lens = np.array([len(r) for r in records], np.int64)
    width = int(lens.max()) if n else 0
    tg = np.full((n, width), 256, np.int16)
    for k, r in enumerate(records):
        tg[k, :len(r)] = E.as_bytes(r)
    idx = np.arange(width + 1, dtype=np.int32)[None, :]
    d = np.zeros((n, n), np.int64)
    for i in range(n - 1):
        a = E.as_bytes(records[i])
        k = n - i - 1
        row = np.repeat(idx, k, axis=0)
        for x in range(a.size):
            t = np.empty((k, width + 1), np.int32)
            t[:, 0] = x + 1
            t[:, 1:] = np.minimum(row[:, 1:] + 1, row[:, :-1] + (tg[i + 1:] != a[x]))
            row = np.minimum.accumulate(t - idx, axis=1) + idx
        d[i, i + 1:] = d[i + 1:, i] = row[np.arange(k), lens[i + 1:]]
    return d


def n_clusters(assign):
    return int((np.asarray(assign) == np.arange(len(assign))).sum())


def census(d, T, band):
    """-> dict: clusters; joins to a representative of the row's own band / of an earlier band (bands of `band` rows); rows with a tie
    for the nearest qualifying representative; rows whose nearest earlier record is a non-representative nearer than every
    representative; representatives that have an earlier non-representative within T"""
    d = np.asarray(d, np.int64)
    n = d.shape[0]
    assign = greedy_assign(d, T)
    isrep = assign == np.arange(n)
    out = dict(clusters=int(isrep.sum()), joins_same_band=0, joins_earlier_band=0, ties=0, nearer_nonrep=0, rep_despite_nonrep=0)
    for i in range(1, n):
        reps = np.nonzero(isrep[:i])[0]
        nonreps = np.nonzero(~isrep[:i])[0]
        vr = d[i, reps]
        if not isrep[i]:
            out["joins_same_band" if assign[i] // band == i // band else "joins_earlier_band"] += 1
            out["ties"] += int(np.sum((vr == vr.min()) & (vr <= T)) > 1)
        if nonreps.size and d[i, nonreps].min() < vr.min():
            out["nearer_nonrep"] += 1
        if isrep[i] and nonreps.size and d[i, nonreps].min() <= T:
            out["rep_despite_nonrep"] += 1
    return out
