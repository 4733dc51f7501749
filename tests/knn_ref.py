"""Checker for `cmp --topk` / `--similarity-threshold`: NumPy / Python only, written from the reference's
src/index_build.cpp:166-228 (build_exact_graph), src/cmp_core.cpp:787-793 (the sign flip) and src/emitnn.cpp:7-48 (the files).

knn_intended        the contract this build implements: all ties with the K-th best value are kept (the reference's stated
                    intent, index_build.cpp:206,219)
knn_reference_heap  the reference's loop as written (priority_queue of pairs: push / pop / final trim), which loses some of those
                    ties
Both take the full N x N float32 matrix of compare(i, j) and return CSR (indptr u64 [N+1], indices u32, data f32).
"""
import heapq
import struct

import numpy as np

HEADER_TEXT = b"#Collection\tNeighbor lists -- name:distance, separated by tabs\n"


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.uint64)
    for i, r in enumerate(rows):
        indptr[i + 1] = indptr[i] + np.uint64(len(r))
    indices = np.array([j for r in rows for (_, j) in r], np.uint32)
    data = np.array([v for r in rows for (v, _) in r], np.float32)
    return indptr, indices, data


def knn_intended(values, K=None, T=None, isdist=False, rows=None):
    """every j != i whose value is at least as good as the K-th best of row i (a similarity of 0 never takes part), or every j
    with (double)v >= T (similarities) / <= T (distances); best first, equal values by ascending index"""
    values = np.asarray(values, np.float32)
    N = values.shape[0]
    assert (K is None) != (T is None)
    out = []
    for i in (range(N) if rows is None else range(*rows)):
        v = values[i]
        js = np.array([j for j in range(N) if j != i], np.int64)
        if K is not None:
            assert K >= 1
            if not isdist:
                js = js[v[js] != 0]                                   # index_build.cpp:194
            if js.size > K:
                key = v[js] if isdist else -v[js]
                kth = np.sort(key, kind="stable")[K - 1]
                js = js[key <= kth]                                    # all ties with the K-th value
        else:
            assert T > 0
            js = js[(v[js].astype(np.float64) <= T) if isdist else (v[js].astype(np.float64) >= T)]   # :184-185,211
        key = v[js] if isdist else -v[js]
        order = np.lexsort((js, key))                                  # std::sort of (+-v, id), index_build.h:16
        out.append([(v[j], int(j)) for j in js[order]])
    return _csr(out)


def knn_reference_heap(values, K=None, T=None, isdist=False):
    """build_exact_graph line for line (index_build.cpp:183-222) + the sign flip of cmp_core.cpp:787-793"""
    values = np.asarray(values, np.float32)
    N = values.shape[0]
    knn = K is not None
    num_neighbors = K if knn else -1                                   # Dashing2DistOptions::num_neighbors_
    mult = np.float32(1.0 if isdist else -1.0)
    simt = T if (T is not None and T > 0) else 0.9
    out = []
    for i in range(N):
        nl = []                                                        # std::priority_queue<PairT>: max-heap of (sim, id)

        def push(p):
            heapq.heappush(nl, (-p[0], -p[1]))

        def top():
            return (-nl[0][0], -nl[0][1])

        for rhid in range(N):
            if rhid == i:
                continue
            sim = np.float32(mult * values[i, rhid])
            if knn:
                if not isdist and not sim:
                    continue
                if len(nl) < num_neighbors:
                    push((float(sim), rhid))
                else:
                    oldv = top()[0]
                    if sim < oldv:
                        push((float(sim), rhid))
                        if len(nl) > num_neighbors:
                            heapq.heappop(nl)
                    elif sim == oldv:
                        push((float(sim), rhid))
            else:
                if float(sim) <= float(mult) * simt:
                    push((float(sim), rhid))
        lst = sorted((-a, -b) for a, b in nl)                          # nl.sort()
        if knn and len(lst) > num_neighbors:
            kth_bestv = lst[num_neighbors - 1][0]
            cut = len(lst)
            for p in range(num_neighbors, len(lst)):
                if lst[p][0] > kth_bestv:
                    cut = p
                    break
            lst = lst[:cut]
        out.append([(np.float32(float(mult) * s), j) for s, j in lst])   # emitted values are the plain v
    return _csr(out)


def csr_rows(csr):
    """[(indices, data)] per row"""
    indptr, indices, data = csr
    return [(indices[int(indptr[i]):int(indptr[i + 1])], data[int(indptr[i]):int(indptr[i + 1])]) for i in range(indptr.size - 1)]


def assert_csr_equal(got, exp, what=""):
    """indices equal, values at 0 ulp (bit patterns)"""
    assert np.array_equal(np.asarray(got[0], np.uint64), np.asarray(exp[0], np.uint64)), f"{what}: indptr differs"
    assert np.array_equal(np.asarray(got[1], np.uint32), np.asarray(exp[1], np.uint32)), f"{what}: indices differ"
    assert np.array_equal(np.asarray(got[2], np.float32).view(np.uint32), np.asarray(exp[2], np.float32).view(np.uint32)), f"{what}: values differ"


# ---- the files (emitnn.cpp:7-48) ---------------------------------------------------------------------------------
def csr_bytes(csr):
    """u64 nids, u64 nnz, u64 indptr[nids+1], u32 indices[nnz], f32 data[nnz], native endian (emitnn.cpp:7-11,31-47)"""
    indptr, indices, data = csr
    return (struct.pack("=QQ", indptr.size - 1, indices.size) + np.asarray(indptr, np.uint64).tobytes() +
            np.asarray(indices, np.uint32).tobytes() + np.asarray(data, np.float32).tobytes())


def read_csr_bytes(b):
    """a reader written from the format comment of emitnn.cpp:7-11"""
    nids, nnz = struct.unpack_from("=QQ", b, 0)
    off = 16
    indptr = np.frombuffer(b, np.uint64, nids + 1, off)
    off += 8 * (nids + 1)
    indices = np.frombuffer(b, np.uint32, nnz, off)
    off += 4 * nnz
    data = np.frombuffer(b, np.float32, nnz, off)
    off += 4 * nnz
    assert off == len(b), "trailing bytes"
    assert indptr[0] == 0 and indptr[-1] == nnz and np.all(np.diff(indptr.astype(np.int64)) >= 0)
    return indptr, indices, data


def knn_text(csr, names):
    """the HUMAN_READABLE form (emitnn.cpp:19-29); fmt's {:0.8g} of a float written as C's %.8g"""
    out = [HEADER_TEXT]
    for i, (ix, dt) in enumerate(csr_rows(csr)):
        line = names[i]
        for j, v in zip(ix, dt):
            line += "\t%s:%s" % (names[int(j)], "%.8g" % float(v))
        out.append(line.encode() + b"\n")
    return b"".join(out)


# ---- values from the oracle as it stands ----------------------------------------------------------------------------
def oracle_values(O, sigs, measure, k=31, multiset=False):
    """N x N float32 of compare(i, j): oracle.gtlt_rect -> compare_from_gtlt (set space) or compare_from_neq (multiset space), one
    oracle call per DISTINCT (gt, lt) -- both measures in scope are independent of the cardinalities"""
    sigs = np.ascontiguousarray(sigs, np.float64)
    N, S = sigs.shape
    gt, lt = O.gtlt_rect(sigs, 0, N, 0, N)
    key = gt.astype(np.uint64) << np.uint64(32) | lt.astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.empty(uniq.size, np.float32)
    for n, kk in enumerate(uniq.tolist()):
        g, l = kk >> 32, kk & 0xFFFFFFFF
        vals[n] = (O.compare_from_neq(S - g - l, S, 1.0, 1.0, measure, k) if multiset
                   else O.compare_from_gtlt(g, l, S, 1.0, 1.0, measure, k))
    return vals[inv.reshape(N, N)]


# ---- planted matrices (NumPy) -----------------------------------------------------------------------------------------
def eqcounts(a):
    """blocked NumPy equality counts, N x N int64 (the diagonal holds S)"""
    a = np.ascontiguousarray(a)
    N, S = a.shape
    out = np.empty((N, N), np.int64)
    step = max(1, (1 << 25) // max(1, N * S))
    for r in range(0, N, step):
        out[r:r + step] = (a[r:r + step, None, :] == a[None, :, :]).sum(-1)
    return out


def family_sigs(N, S, seed, fam_lo=5, fam_hi=40):
    """families of fam_lo..fam_hi sketches with graded overlap: member m of a family keeps a member-specific fraction of the
    family's registers and has values of its own elsewhere (doubles in (0, 1), all distinct unless planted equal)"""
    rng = np.random.default_rng(seed)
    sigs = rng.random((N, S)) * 0.5 + 0.25
    i = 0
    while i < N:
        n = int(min(N - i, rng.integers(fam_lo, fam_hi + 1)))
        base = rng.random(S) * 0.5 + 0.25
        for m in range(n):
            keep = rng.random(S) < (0.15 + 0.8 * (m + 1) / n) * rng.choice([1.0, 1.0, 0.5])
            sigs[i + m, keep] = base[keep]
        i += n
    return sigs


def unrelated_sigs(N, S, seed):
    """no two sketches share a register"""
    rng = np.random.default_rng(seed)
    return (rng.permuted(np.tile(np.arange(1, N + 1, dtype=np.float64), (S, 1)), axis=1).T + np.arange(S)[None, :] * (N + 1)) / float((N + 2) * (S + 1))


# ---- the device's contract on COUNTS (include/d2g.h, d2g_cmp_knn_dev) ---------------------------------------------------
def class_table(lut):
    """cls[e] = the smallest count whose value equals that of e (lut monotone in the count)"""
    lut = np.asarray(lut, np.float32)
    cls = np.zeros(lut.size, np.uint32)
    for e in range(1, lut.size):
        cls[e] = cls[e - 1] if lut[e] == lut[e - 1] else e
    return cls


def min_count_for(lut, K=None, T=None, isdist=False):
    """the smallest count that takes part (top-K: a similarity of 0 never does) or passes the threshold; lut.size if none does"""
    lut = np.asarray(lut, np.float32)
    if K is not None:
        ok = np.ones(lut.size, bool) if isdist else lut != 0
    else:
        ok = (lut.astype(np.float64) <= T) if isdist else (lut.astype(np.float64) >= T)
    hit = np.nonzero(ok)[0]
    return int(hit[0]) if hit.size else int(lut.size)


def select_by_count(cnt, K, min_count, cls=None, r0=0, r1=None):
    """rows [r0, r1) of an N x N count matrix -> (rowcnt [n], mask [n][N]): column j != i is listed iff cnt[i, j] >= t_i, with
    t_i = min_count (K == 0), or the K-th largest count >= min_count of the row (min_count if there are fewer than K), lowered
    to the minimum of its value class"""
    cnt = np.asarray(cnt, np.int64)
    N = cnt.shape[0]
    r1 = N if r1 is None else r1
    c = cnt[r0:r1].copy()
    c[np.arange(r1 - r0), np.arange(r0, r1)] = -1                      # the self pair is excluded by index
    t = np.full(r1 - r0, min_count, np.int64)
    if K:
        e = np.where(c >= min_count, c, -1)
        e = -np.sort(-e, axis=1)
        if K <= N:
            kth = e[:, K - 1]
            t = np.where(kth >= 0, kth, min_count)
        if cls is not None:
            t = np.maximum(np.asarray(cls, np.int64)[np.minimum(t, len(cls) - 1)], min_count)
    mask = c >= t[:, None]
    return mask.sum(1).astype(np.uint32), mask
