"""`dashing2 contain` (reference src/contain_main.cpp:133-299): the reference of test_contain_host.py and test_gpu_screen.py (test
infrastructure; held to its own properties by test_contain_ref.py).  No GPU and no library call in here.

    restatement   the reference line by line in Python integers: kmer2ids, a dict key -> [reference ids] in database order (:188-198);
                  per query a dict of the masked k-mers that are database keys -> occurrences (:40-48); the :224-241 loops over it,
                  matches and matchsums in wrapping uint32
    closed_form   the same two integers per (query, reference) from the distinct masked k-mers of a query and their multiplicities
                  (k3_seam_cases.key_counts): matches = #{j : cnt(key[r][j]) > 0}, matchsum = sum_j cnt(key[r][j]) mod 2^32
    epilogue      coverage = float32(float64(1 / S) * matches), depth = float32(matchsum // matches); both 0 where matches == 0
    writers       the text (:252-257 header, :291-294 entries: the scalar arm) and the -b form (:246-249)

The minkmer / maxkmer test of :42 is a shortcut (every key lies between the smallest and the largest key) and appears in neither."""
import numpy as np

import k3_seam_cases as C
import oph_kmers_ref as R

M32 = 0xFFFFFFFF
HEADER = ("#Dashing2 contain - a list of coverage %%s for the set of references, + mean coverage levels.\n"
          "#Each matrix entry consists of <coverage%%:mean depth of coverage>\n"
          "##References:")


# ---------------------------------------------------------------- the two integer forms
def restatement(db_keys, query_streams):
    """db_keys [nrefs][S] masked keys; query_streams: per query the masked k-mers in order -> (matches, matchsums) uint32 [nq][nrefs]"""
    db_keys = np.asarray(db_keys, np.uint64)
    nrefs = db_keys.shape[0]
    kmer2ids = {}
    for i in range(nrefs):                                              # :189-198
        for key in db_keys[i].tolist():
            kmer2ids.setdefault(key, []).append(i)
    matches = np.zeros((len(query_streams), nrefs), np.uint32)
    sums = np.zeros((len(query_streams), nrefs), np.uint32)
    for q, stream in enumerate(query_streams):
        myres = {}
        for kmer in stream:                                             # :40-48
            kmer = int(kmer)
            if kmer not in kmer2ids:
                continue
            myres[kmer] = myres.get(kmer, 0) + 1
        m, s = [0] * nrefs, [0] * nrefs
        for key, value in myres.items():                                # :226-231
            for refid in kmer2ids[key]:
                m[refid] = (m[refid] + 1) & M32
                s[refid] = (s[refid] + value) & M32
        matches[q], sums[q] = m, s
    return matches, sums


def closed_form(db_keys, keys, counts):
    """one query given as its distinct masked k-mers (sorted) and their multiplicities -> (matches, matchsums) uint32 [nrefs]"""
    db_keys = np.asarray(db_keys, np.uint64)
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint64)
    if keys.size == 0 or db_keys.size == 0:
        z = np.zeros(db_keys.shape[0], np.uint32)
        return z, z.copy()
    pos = np.minimum(np.searchsorted(keys, db_keys), keys.size - 1)
    cnt = np.where(keys[pos] == db_keys, counts[pos], np.uint64(0))     # [nrefs][S]
    return (cnt != 0).sum(axis=1).astype(np.uint32), (cnt.sum(axis=1, dtype=np.uint64) & np.uint64(M32)).astype(np.uint32)


def key_counts_of_db(db_keys, keys, counts):
    """what d2g_screen_key_counts returns for that query: the distinct database keys ascending and the query's count of each"""
    d = np.unique(np.asarray(db_keys, np.uint64))
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
    if keys.size == 0 or d.size == 0:
        return d, np.zeros(d.size, np.uint32)
    pos = np.minimum(np.searchsorted(keys, d), keys.size - 1)
    return d, np.where(keys[pos] == d, counts[pos], 0).astype(np.uint32)


def query_closed_form(db_keys, records, k, canon, xormask):
    keys, counts, _ = C.key_counts(tuple(records), k, canon, xormask)
    return closed_form(db_keys, keys, counts)


# ---------------------------------------------------------------- the epilogue
def epilogue(matches, matchsums, S):
    """:221,237-241 -> (coverage, depth) float32, shaped like matches"""
    m = np.asarray(matches, np.uint32)
    s = np.asarray(matchsums, np.uint32)
    ssiv = np.float64(1.0) / np.float64(S)
    cov = np.where(m != 0, (ssiv * m.astype(np.float64)).astype(np.float32), np.float32(0))
    dep = np.where(m != 0, (s // np.maximum(m, 1)).astype(np.float32), np.float32(0))
    return cov.astype(np.float32), dep.astype(np.float32)


# ---------------------------------------------------------------- the text of one value
def fmt_g6(v):
    """fmt "{:0.6g}" of a float32: six significant digits of the value widened to double, trailing zeros dropped"""
    return "%.6g" % float(np.float32(v))


def fmt_float(v):
    """fmt "{}" of a float32 (fmt < 11 layout): the shortest digits that round-trip, fixed notation for exponents in [-4, 16)"""
    v = np.float32(v)
    if v == 0:
        return "-0" if np.signbit(v) else "0"
    if not np.isfinite(v):
        return ("-" if v < 0 else "") + ("inf" if np.isinf(v) else "nan")
    sci = np.format_float_scientific(v, unique=True, trim="-", exp_digits=2)
    mant, exp = sci.split("e")
    e = int(exp)
    if -4 <= e < 16:
        return np.format_float_positional(v, unique=True, trim="-")
    return mant + "e" + exp


def entry(coverage, depth):
    return "\t" + fmt_g6(np.float32(100) * np.float32(coverage)) + "%:" + fmt_float(depth)


# ---------------------------------------------------------------- the writers
def text_bytes(names, queries, coverage, depth):
    coverage, depth = np.asarray(coverage, np.float32), np.asarray(depth, np.float32)
    out = [HEADER + "".join("\t" + n for n in names) + "\n"]
    for q, path in enumerate(queries):
        out.append(path + "".join(entry(coverage[q][r], depth[q][r]) for r in range(len(names))) + "\n")
    return "".join(out).encode()


def binary_bytes(nrefs, coverage, depth):
    coverage, depth = np.ascontiguousarray(coverage, np.float32), np.ascontiguousarray(depth, np.float32)
    nq = coverage.shape[0] if coverage.ndim == 2 else 0
    return np.array([nrefs, nq], np.uint64).tobytes() + coverage.tobytes() + depth.tobytes()


def expected_outputs(db_keys, S, names, queries, query_records, k, canon, xormask):
    """-> (text bytes, binary bytes) of `contain db queries...`: query_records[q] = the ACGT records of query q"""
    nrefs = len(names)
    m = np.zeros((len(queries), nrefs), np.uint32)
    s = np.zeros((len(queries), nrefs), np.uint32)
    for q, recs in enumerate(query_records):
        m[q], s[q] = query_closed_form(db_keys, recs, k, canon, xormask)
    cov, dep = epilogue(m, s, S)
    return text_bytes(names, queries, cov, dep), binary_bytes(nrefs, cov, dep)


def masked_stream(records, k, canon, xormask):
    return R.masked_stream(records, k, canon, xormask)
