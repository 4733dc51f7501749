"""Checker for `cmp --greedy T`: NumPy / Python only, written from the reference's src/dedup_core.cpp:262-283 (the exhaustive
branch of dedup_core) and :400-451 (dedup_emit), and from fmt's documented "{}" of a double.

dedup_reference   the loop as written, on the full N x N float32 matrix of compare(i, j): -> (ids, constituents)
assign_of         the same result as the device returns it: the representative of every sketch
clusters_text / clusters_bytes   the two files of dedup_emit
fmt_double        fmt's "{}" of a double
census            what a case exercises (joins across / inside a band, ties, non-representative neighbours), from the REFERENCE result
"""
import struct
from decimal import Decimal

import numpy as np

DEFAULT_T = 0.9                                                        # dedup_core.cpp:264


def simt_of(T):
    """LSHDistType simt = min_similarity > 0 ? min_similarity : 0.9 (a float)"""
    return np.float32(T if T > 0 else DEFAULT_T)


def dedup_reference(values, T):
    """for i in input order: bestc = min over clusters c of (-v(i, rep_c), c); a new cluster if there is none or v_best < simt
    (float comparison), else i is appended to cluster c_best.  -> (ids [C], constituents [C][...])"""
    values = np.asarray(values, np.float32)
    N = values.shape[0]
    simt = simt_of(T)
    ids, constituents = [], []
    for i in range(N):
        best = None
        if ids:
            v = values[i, ids]
            c = int(np.argmax(v))                                      # the largest value; the first of equal ones = the smallest c
            best = (v[c], c)
        if best is None or best[0] < simt:
            ids.append(i)
            constituents.append([])
        else:
            constituents[best[1]].append(i)
    return ids, constituents


def dedup_reference_loop(values, T):
    """the same, pair by pair as the reference's std::min over (mult * v, c) pairs does it (small N only: the checker's checker)"""
    values = np.asarray(values, np.float32)
    simt = simt_of(T)
    ids, constituents = [], []
    for i in range(values.shape[0]):
        bestc = (np.float32(np.finfo(np.float32).max), -1)
        for j, rep in enumerate(ids):
            cand = (np.float32(-values[i, rep]), j)
            if cand < bestc:
                bestc = cand
        if bestc[1] == -1 or np.float32(-bestc[0]) < simt:
            ids.append(i)
            constituents.append([])
        else:
            constituents[bestc[1]].append(i)
    return ids, constituents


def assign_of(ids, constituents, N):
    a = np.full(N, 0xFFFFFFFF, np.uint32)
    for rep, members in zip(ids, constituents):
        a[rep] = rep
        a[members] = rep
    assert not np.any(a == 0xFFFFFFFF)
    return a


def clusters_of(assign):
    """assign -> (ids, constituents): creation order = ascending representative, members in input order"""
    assign = np.asarray(assign)
    ids = [int(i) for i in np.nonzero(assign == np.arange(assign.size))[0]]
    pos = {r: c for c, r in enumerate(ids)}
    constituents = [[] for _ in ids]
    for i, r in enumerate(assign.tolist()):
        if r != i:
            constituents[pos[r]].append(i)
    return ids, constituents


# ---- fmt's "{}" of a double -------------------------------------------------------------------------------------------------
def fmt_double(x):
    """shortest round-trip digits; fixed notation for decimal exponents in [-4, 16), else d[.ddd]e+-XX (at least two exponent
    digits); no trailing ".0" """
    x = float(x)
    if x != x:
        return "nan"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    sign = "-" if (x < 0 or (x == 0 and str(x)[0] == "-")) else ""
    if x == 0:
        return sign + "0"
    t = Decimal(repr(abs(x))).as_tuple()                               # repr: the shortest digits that round-trip
    digits = "".join(map(str, t.digits)).rstrip("0") or "0"
    exp10 = len(t.digits) - 1 + t.exponent                             # exponent of the first digit
    nd = len(digits)
    if -4 <= exp10 < 16:
        if exp10 >= nd - 1:
            return sign + digits + "0" * (exp10 - (nd - 1))
        if exp10 >= 0:
            return sign + digits[:exp10 + 1] + "." + digits[exp10 + 1:]
        return sign + "0." + "0" * (-exp10 - 1) + digits
    return sign + digits[0] + ("." + digits[1:] if nd > 1 else "") + "e" + ("-" if exp10 < 0 else "+") + "%02d" % abs(exp10)


# ---- the files (dedup_emit, dedup_core.cpp:423-449) --------------------------------------------------------------------------
def clusters_text(ids, constituents, names, T):
    N = len(names)
    out = ["#Clustering %d items yielded %d clusters of average size %s, separated by minimum similarity %s\n"
           % (N, len(ids), fmt_double(N / len(ids)), fmt_double(T))]
    for cid, (rep, members) in enumerate(zip(ids, constituents)):
        out.append("Cluster-%d\t%s:%d" % (cid, names[rep], rep) + "".join("\t%s:%d" % (names[m], m) for m in members) + "\n")
    return "".join(out).encode()


def clusters_bytes(ids, constituents):
    """u64 nclusters, u64 nnz, u64 indptr[nclusters+1], then per cluster u32 rep, u32 members... (LSHIDType = u32)"""
    indptr = np.zeros(len(ids) + 1, np.uint64)
    for c, members in enumerate(constituents):
        indptr[c + 1] = indptr[c] + np.uint64(len(members) + 1)
    body = b"".join(np.array([rep] + list(members), np.uint32).tobytes() for rep, members in zip(ids, constituents))
    return struct.pack("=QQ", len(ids), int(indptr[-1])) + indptr.tobytes() + body


def read_clusters_bytes(b):
    nclusters, nnz = struct.unpack_from("=QQ", b, 0)
    indptr = np.frombuffer(b, np.uint64, nclusters + 1, 16)
    indices = np.frombuffer(b, np.uint32, nnz, 16 + 8 * (nclusters + 1))
    assert 16 + 8 * (nclusters + 1) + 4 * nnz == len(b) and indptr[0] == 0 and indptr[-1] == nnz
    return indptr, indices


# ---- what a case exercises, from the reference result alone -----------------------------------------------------------------
def census(values, T, band):
    """-> dict: clusters; joins to a representative of an earlier band / of the row's own band (bands of `band` rows); rows with a
    tie for the best among the qualifying representatives; rows whose best earlier sketch (representative or not) is a
    non-representative with a value above every representative's; representatives with an earlier NON-representative at or above T"""
    values = np.asarray(values, np.float32)
    N = values.shape[0]
    simt = simt_of(T)
    ids, cons = dedup_reference(values, T)
    assign = assign_of(ids, cons, N)
    isrep = assign == np.arange(N)
    out = dict(clusters=len(ids), joins_earlier_band=0, joins_same_band=0, ties=0, better_nonrep=0, rep_despite_nonrep=0)
    for i in range(1, N):
        reps = np.nonzero(isrep[:i])[0]
        nonreps = np.nonzero(~isrep[:i])[0]
        vr = values[i, reps]
        if not isrep[i]:
            out["joins_same_band" if assign[i] // band == i // band else "joins_earlier_band"] += 1
            out["ties"] += int(np.sum((vr == vr.max()) & (vr >= simt)) > 1)
        if nonreps.size and values[i, nonreps].max() > (vr.max() if vr.size else -1):
            out["better_nonrep"] += 1
        if isrep[i] and nonreps.size and values[i, nonreps].max() >= simt:
            out["rep_despite_nonrep"] += 1
    return out
