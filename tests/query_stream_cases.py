"""Inputs, decoy inputs and expected results for the query-side device entry points on a caller's busy stream
(test_gpu_query_streams.py), and the conditions that make a launch on the wrong stream visible (held to them by
test_query_stream_cases.py).  No GPU and no library kernel in here: NumPy and the existing references only (knn_ref, dedup_ref,
trunc_ref, exact_ref, edit_ref, edit_within_ref, edit_dedup_ref); no new reference algorithm.

A device input comes in two versions: A, whose result is expected, and the DECOY B, which lies in the buffer until a copy queued behind
the ballast replaces it.  Outputs are pre-filled with the byte 0xAB (the word POISON) and filled again behind the ballast, so a launch
that ran ahead of the ballast either read B or had its result overwritten.  What makes that visible:
    Q1  for every device input, expected(A) and expected(B) differ in at least a quarter of their output words
    Q2  every selection expects 0 < nnz < N (N - 1) and has a row that expects more entries than its cap
    Q3  every clustering expects between 2 and N - 1 clusters
    Q4  the edit set has rows of all three launch classes of the pair kernel, and at T = 7 at least 3 changes of route along its rows
    Q5  no word that a call WRITES is expected to equal POISON (the slots behind a row's entries are expected to keep it)

Q4 and D2G_EDIT_STRIP: the pair kernel's classes are 0: blocks <= min(8, strip), 1: 8 < blocks <= strip, 2: blocks > strip (blocks of 32
symbols; d2g_edit.hip).  Under strip = 2 class 1 is empty BY THAT RULE for any set, so the GPU tests run the edit set under strip = 2
(classes 0 and 2: every record above 64 symbols strip by strip) and under EDIT_STRIP_ALL = 9 (all three classes); Q4 is asserted for both.
"""
import functools

import numpy as np

import dedup_ref
import edit_dedup_ref
import edit_ref
import edit_within_ref
import exact_ref
import k3_seam_cases
import knn_ref
import trunc_ref

POISON = 0xABABABAB
POISON64 = 0xABABABABABABABAB
DNA = np.frombuffer(b"ACGT", np.uint8)


def differing_fraction(a, b):
    """Q1: the share of output words in which two expectations differ (a list of arrays each, same shapes)"""
    diff = total = 0
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape
        diff += int((x != y).sum())
        total += x.size
    return diff / total


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------- 1. selection and clustering over sketches
SK_N, SK_S, SK_BAND = 257, 128, 33
SK_K, SK_CAP = 5, 8
SMALL_N, SMALL_S = 67, 64                                     # case 5: the first user of an empty scratch
BIG_N, BIG_S = 1000, 64                                       # case 5: the clustering whose band makes the scratch grow
DEDUP_T = 0.25


@functools.lru_cache(maxsize=None)
def sketches(N, S):
    """(sigs float64 [N][S], counts int64 [N][N]): test_gpu_knn.py's family matrix of the shape"""
    sigs = np.ascontiguousarray(knn_ref.family_sigs(N, S, seed=N * 7 + S))
    return _frozen(sigs, knn_ref.eqcounts(sigs.view(np.uint64)))


def cls_real(S):
    """classes of four counts (test_gpu_knn.py::test_knn_dev_class_table_merges_counts): cls[e] <= e, non-decreasing"""
    return (np.arange(S + 1, dtype=np.uint32) // 4 * 4).astype(np.uint32)


def cls_decoy_select(S):
    """the class table that lists nobody: t_i becomes S + 1 in every row (top-K mode reads cls once per row)"""
    return np.full(S + 1, S + 1, np.uint32)


def cls_decoy_dedup(S):
    """the class table under which no count qualifies for a min_count >= 1: every sketch founds a cluster"""
    return np.zeros(S + 1, np.uint32)


def selection(cnt, K, min_count, cls, cap, r0=0, r1=None):
    """d2g_cmp_knn_dev's contract on a count matrix (knn_ref.select_by_count) as the device lays it out: (rowcnt u32 [n],
    ids u32 [n][cap], counts u32 [n][cap]), a row's columns in ascending j, POISON behind them (test_gpu_knn.py::expected_dev)"""
    N = cnt.shape[0]
    r1 = N if r1 is None else r1
    rowcnt, mask = knn_ref.select_by_count(cnt, K, min_count, cls, r0, r1)
    order = np.argsort(~mask, axis=1, kind="stable")[:, :cap]
    if order.shape[1] < cap:
        order = np.pad(order, ((0, 0), (0, cap - order.shape[1])))
    used = np.arange(cap)[None, :] < np.minimum(rowcnt, cap)[:, None]
    ids = np.where(used, order, POISON).astype(np.uint32)
    cts = np.where(used, np.take_along_axis(np.asarray(cnt[r0:r1]), order, axis=1), POISON).astype(np.uint32)
    return rowcnt.astype(np.uint32), ids, cts


def nnz_of(sel):
    return int(sel[0].astype(np.int64).sum())


def dedup_min_count(S, cls, T=DEDUP_T):
    """the smallest count whose value cls[c] / S reaches simt (float comparison), S + 1 if none does"""
    lut = (cls.astype(np.float64) / S).astype(np.float32)
    hit = np.nonzero(lut >= dedup_ref.simt_of(T))[0]
    return int(hit[0]) if hit.size else S + 1


def clustering(cnt, S, cls, min_count):
    """d2g_cmp_dedup_dev's rule (a count qualifies iff cls[c] >= min_count, the largest cls[c] wins, the smallest representative among
    equals) through dedup_ref.dedup_reference on the values cls[c] / S with the threshold min_count / S: both are exact in float32"""
    values = (cls.astype(np.int64)[np.minimum(cnt, S)] / S).astype(np.float32)
    ids, cons = dedup_ref.dedup_reference(values, np.float32(min_count / S))
    return dedup_ref.assign_of(ids, cons, cnt.shape[0])


def identity(S):
    return np.arange(S + 1, dtype=np.uint32)


PLAIN_CAP = 6                                                 # top-K without a class table: no merged tie classes, narrower rows


@functools.lru_cache(maxsize=None)
def sketch_selections():
    """EVERY selection over sketches that test_gpu_query_streams.py expects, by the name it asks for: name -> (N, S, K, min_count,
    class table or None, cap, the expectation).  test_query_stream_cases.py holds each of them to Q2 and Q5"""
    out = {}
    for name, N, S, K, mc, cls, cap in (("classed topk 257", SK_N, SK_S, SK_K, 1, cls_real(SK_S), SK_CAP),       # cases 1 and 6
                                         ("threshold 257", SK_N, SK_S, 0, SK_S // 4, None, SK_CAP),              # cases 1 and 6
                                         ("plain topk 67", SMALL_N, SMALL_S, SK_K, 1, None, PLAIN_CAP),          # case 5, step 1
                                         ("plain topk 257", SK_N, SK_S, SK_K, 1, None, PLAIN_CAP)):              # case 5, step 5; case 7
        out[name] = (N, S, K, mc, cls, cap, selection(sketches(N, S)[1], K, mc, cls, cap))
    return out


@functools.lru_cache(maxsize=None)
def sketch_clusterings():
    """EVERY clustering over sketches that test_gpu_query_streams.py expects: name -> (N, S, min_count, class table, the expectation)"""
    out = {}
    for name, N, S, cls in (("classed clusters 257", SK_N, SK_S, cls_real(SK_S)),                               # cases 1 and 6
                            ("plain clusters 1000", BIG_N, BIG_S, identity(BIG_S))):                            # case 5, step 3
        mc = dedup_min_count(S, cls)
        out[name] = (N, S, mc, cls, clustering(sketches(N, S)[1], S, cls, mc))
    return out


# ---------------------------------------------------------------- 2. code-plane sets
CODE_N, CODE_S = 257, 100
CODE_K, CODE_CAP, CODE_T = 5, 8, 30


@functools.lru_cache(maxsize=None)
def codes(which):
    """1-byte codes of four values (heavy ties), a block of identical rows; A and B from different seeds"""
    rng = np.random.default_rng({"A": 8, "B": 9}[which])
    c = rng.integers(0, 4, (CODE_N, CODE_S)).astype(np.uint8)
    c[40:60] = c[40]
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def code_expect(which):
    """-> dict: eq u32 [N][N], gt, lt (rows x columns), topk and threshold selections over the equality counts"""
    c = codes(which)
    cnt = knn_ref.eqcounts(c)
    gt, lt = trunc_ref.gtlt_rect(c, 0, CODE_N, 0, CODE_N)
    return {"cnt": cnt, "eq": cnt.astype(np.uint32), "gt": gt, "lt": lt,
            "topk": selection(cnt, CODE_K, 0, None, CODE_CAP), "threshold": selection(cnt, 0, CODE_T, None, CODE_CAP)}


# ---------------------------------------------------------------- 3. exact sets
EXACT_K = 21
EXACT_LENGTHS = [[6000], [4000, 4000], [4000], [], [3000]]


def _periodic(rng, period, n):
    u = k3_seam_cases.random_bases(rng, period)
    return (u * (n // period + 1))[:n]


@functools.lru_cache(maxsize=None)
def exact_batch(which):
    """A: the five genomes of test_gpu_exact_cmp.py::test_sets_from_the_sketch_side_stay_on_the_device.  B: records of the SAME lengths
    (one plan serves both) with other relations and other cardinalities: periodic records (few distinct k-mers), genomes 0 and 1
    unrelated, genomes 2 and 4 of one period"""
    if which == "A":
        rng = np.random.default_rng(4700)
        base = k3_seam_cases.random_bases(rng, 6000)
        genomes = [[base], [base[:4000], base[:4000]], [base[2000:]], [], [k3_seam_cases.random_bases(rng, 3000)]]
    else:
        rng = np.random.default_rng(4701)
        w = _periodic(rng, 800, 4000)
        genomes = [[_periodic(rng, 1500, 6000)], [_periodic(rng, 1000, 4000)] * 2, [w], [], [w[:3000]]]
    assert [[len(r) for r in g] for g in genomes] == EXACT_LENGTHS
    return k3_seam_cases.Batch("qs" + which, EXACT_K, 16, True, 0, genomes)


@functools.lru_cache(maxsize=None)
def exact_expect(which, weighted):
    """(upper triangle u64, square u64 [n][n]) of exact_ref.isz_matrix over the batch's sets"""
    m = exact_ref.isz_matrix(exact_ref.exact_sets(exact_batch(which)), weighted)
    return _frozen(exact_ref.ut(m), m)


HOST_SETS = 9


@functools.lru_cache(maxsize=None)
def host_sets():
    """9 sets of up to 2 500 keys (one empty) drawn from one pool, with counts: the d2g_kset made from host arrays"""
    rng = np.random.default_rng(4800)
    pool = exact_ref.rng_keys(4801, 6000)
    out = []
    for i in range(HOST_SETS):
        m = 0 if i == 3 else int(rng.integers(300, 2501))
        k = np.sort(rng.choice(pool, m, replace=False))
        out.append((k, rng.integers(1, 9, m).astype(np.uint32)))
    return out


@functools.lru_cache(maxsize=None)
def host_expect(weighted):
    m = exact_ref.isz_matrix(host_sets(), weighted)
    return _frozen(exact_ref.ut(m), m)


# ---------------------------------------------------------------- 4. edit distances
# The dispatcher's rules, restated from the constants documented in d2g_edit_near.hip (EDIT_NEAR_FULL_MAX_LEN, EDIT_NEAR_SHORT_T_FACTOR,
# EDIT_NEAR_TINY_LEN), d2g_edit.hip (EDIT_SMALL_BLOCKS), d2g_edit.h (EDIT_LDS_WORDS) and include/d2g.h (D2G_EDIT_BAND_MAX).  A change of
# one of those constants must be followed here: Q4 is a statement about the library's routes, not about these numbers.
EDIT_BAND_MAX, EDIT_NEAR_FULL_MAX_LEN, EDIT_NEAR_SHORT_T_FACTOR, EDIT_NEAR_TINY_LEN = 31, 32, 5, 8
EDIT_SMALL_BLOCKS, EDIT_LDS_WORDS = 8, 16384
EDIT_STRIP_ALL = 9                                            # the D2G_EDIT_STRIP under which the set has rows of all three classes
EDIT_SHORT = [1, 5, 8, 9, 12, 16, 20, 24, 31, 32]
EDIT_MID = [33, 40, 63, 64, 65, 96, 150, 256]
EDIT_LONG = [257, 270, 288, 289, 300, 310]
NEAR_BOUNDS = (7, 31, 32)
WITHIN_BAND, WITHIN_CAP = 7, 2
WITHIN_MODES = ((3, 7), (0, 7), (0, 32))                      # (K, T): top-K over alternating routes, threshold on both routes
EDIT_DEDUP_BAND = 16


def near_takes_the_band_route(length, sigma, T):
    """near_band_row of d2g_edit_near.hip under the dispatcher's own choice (D2G_EDIT_NEAR_ROUTE unset)"""
    if T > EDIT_BAND_MAX:
        return False
    if sigma * ((((length + 31) // 32) + 4) | 1) > EDIT_LDS_WORDS:
        return False
    return length > EDIT_NEAR_FULL_MAX_LEN or length <= EDIT_NEAR_TINY_LEN or EDIT_NEAR_SHORT_T_FACTOR * T < length


def route_changes(lengths, sigma, T):
    r = [near_takes_the_band_route(int(n), sigma, T) for n in lengths]
    return sum(a != b for a, b in zip(r, r[1:]))


def launch_class(length, strip):
    """the class of a row of the pair kernel (edit_rect_window in d2g_edit.hip)"""
    blocks = (length + 31) // 32
    return 0 if blocks <= EDIT_SMALL_BLOCKS and blocks <= strip else 1 if blocks <= strip else 2


def _mutated(rng, x, edits):
    y = list(x)
    for _ in range(edits):
        op = int(rng.integers(3))
        if op == 0:
            y[int(rng.integers(len(y)))] = int(rng.choice(DNA))
        elif op == 1 and len(y) > 1:
            del y[int(rng.integers(len(y)))]
        else:
            y.insert(int(rng.integers(len(y) + 1)), int(rng.choice(DNA)))
    return bytes(y)


@functools.lru_cache(maxsize=None)
def edit_set():
    """48 records: prefixes of one base at 24 lengths (1 .. 32, 33 .. 256, 257 .. 310), each beside a copy with 1, 2, 3 or 5 random
    edits, shuffled: families inside and across lengths.  -> (records, distance matrix int64 [N][N])"""
    rng = np.random.default_rng(8600)
    base = bytes(rng.choice(DNA, 310).tolist())
    recs = []
    for k, n in enumerate(EDIT_SHORT + EDIT_MID + EDIT_LONG):
        recs += [base[:n], _mutated(rng, base[:n], (1, 2, 3, 5)[k % 4])]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    d = edit_ref.edit_matrix(recs)
    d.setflags(write=False)
    return recs, d


def edit_triangle():
    return edit_ref.triangle(edit_set()[1]).astype(np.uint32)


EDIT_RECT = (5, 41, 3, 48)                                    # a block that is neither the square nor aligned to anything


def edit_rect():
    a0, a1, b0, b1 = EDIT_RECT
    return edit_set()[1][a0:a1, b0:b1].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def near(T):
    c = edit_within_ref.closeness(edit_set()[1], T)
    return _frozen(np.asarray(c, np.int64))


@functools.lru_cache(maxsize=None)
def within(K, T, cap=WITHIN_CAP):
    """d2g_edit_within_dev = the selection of d2g_cmp_knn_dev over closeness with min_count = 1 and no class table (include/d2g.h)"""
    return selection(near(T), K, 1, None, cap)


@functools.lru_cache(maxsize=None)
def edit_clusters(T):
    return _frozen(edit_dedup_ref.greedy_assign(edit_set()[1], T))


def n_clusters(assign):
    return edit_dedup_ref.n_clusters(assign)
