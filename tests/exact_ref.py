"""Exact k-mer sets, --set and --countdict, restated without anything the product computes (test infrastructure for test_exact_ref.py,
test_exact_host.py and the test_gpu_exact_*.py files; held to its own properties by test_exact_ref.py).  No GPU in here.

Reference lines restated:
    Counter::finalize(vector&, vector&, thr)     src/counter.h:78-117      -> exact_sets (from k3_seam_cases.key_counts)
    weighted_compare on two files                src/wcompare.cpp:145-187  -> merge_isz, literally; dict_isz is the closed form
    CORRECT_RES and the NaN / Inf rule           src/cmp_core.cpp:518-575  -> measure_value
    the two files and their names                src/fastxsketch.cpp:313-317,462-519, src/fastxmerge.cpp:70-120, src/enums.cpp:28-37

One deliberate difference from the reference: --union-size is card_i + card_j - isz here; CORRECT_RES has no arm for it and
returns isz."""
import math

import numpy as np

SIMILARITY, CONTAINMENT, SYMMETRIC_CONTAINMENT, POISSON_LLR, INTERSECTION, UNION_SIZE = range(6)     # enum Measure, src/cmp_main.h:8-17
MEASURES = (SIMILARITY, CONTAINMENT, SYMMETRIC_CONTAINMENT, POISSON_LLR, INTERSECTION, UNION_SIZE)
LD = np.longdouble


# ---------------------------------------------------------------- E_i
def exact_sets(batch, thr=0.0):
    """per genome of a k3_seam_cases.Batch: (keys uint64 ascending, counts uint32) of the distinct masked k-mers with count > thr"""
    out = []
    for keys, counts, _ in batch.counts():
        keep = counts.astype(np.float64) > thr                             # counter.h:87
        out.append((keys[keep], counts[keep]))
    return out


def card(keys, counts, weighted):
    """--set: |E|; --countdict: the integer sum of the counts (fastxsketch.cpp:439-441)"""
    return int(np.asarray(counts, np.uint64).sum()) if weighted else int(len(keys))


def flat(sets):
    """list of (keys, counts) -> (keys, counts, set_off uint64[n+1], cards uint64[n][2]) as d2g_kmer_sets lays them out"""
    off = np.zeros(len(sets) + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k, _ in sets])
    keys = np.concatenate([np.asarray(k, np.uint64) for k, _ in sets]) if sets else np.empty(0, np.uint64)
    counts = np.concatenate([np.asarray(c, np.uint32) for _, c in sets]) if sets else np.empty(0, np.uint32)
    cards = np.array([[card(k, c, False), card(k, c, True)] for k, c in sets], np.uint64).reshape(len(sets), 2)
    return keys, counts, off, cards


# ---------------------------------------------------------------- the merge, literally
class _Stream:
    """a FILE * over 8-byte elements: fread of one element either succeeds, or fails, leaves its destination alone and sets feof"""

    def __init__(self, items):
        self.items, self.pos, self.eof = list(items), 0, False

    def fread(self, old):
        if self.pos < len(self.items):
            self.pos += 1
            return self.items[self.pos - 1]
        self.eof = True
        return old


UNSET = object()        # an uninitialised uint64_t: reading it is undefined in C++; restated as a value that equals and orders with no key


def merge_isz(lkeys, lcounts, rkeys, rcounts):
    """weighted_compare (wcompare.cpp:145-187) after compare() has read both headers: two cursors, one element per fread, the loop ends
    when EITHER stream has hit its end.  lcounts / rcounts None = no count file (lhc = rhc = 1.).  -> the intersection as an int"""
    lhk, rhk = _Stream(int(x) for x in lkeys), _Stream(int(x) for x in rkeys)
    lhn = None if lcounts is None else _Stream(float(x) for x in lcounts)
    rhn = None if rcounts is None else _Stream(float(x) for x in rcounts)
    st = {"lhv": UNSET, "rhv": UNSET, "lhc": 1.0, "rhc": 1.0}

    def incl():
        st["lhv"] = lhk.fread(st["lhv"])
        if lhn is not None:
            st["lhc"] = lhn.fread(st["lhc"])

    def incr():
        st["rhv"] = rhk.fread(st["rhv"])
        if rhn is not None:
            st["rhc"] = rhn.fread(st["rhc"])

    isz = LD(0)
    incl(); incr()                                                         # incb()
    while True:
        lhv, rhv = st["lhv"], st["rhv"]
        if lhv is UNSET or rhv is UNSET:                                   # an empty side: whatever the comparison does, a read fails next
            incl() if lhv is UNSET else incr()
        elif lhv < rhv:
            incl()
        elif rhv < lhv:
            incr()
        else:
            isz += LD(min(st["rhc"], st["lhc"]))
            incl(); incr()
        if lhk.eof or rhk.eof:
            break
    assert isz == int(isz)
    return int(isz)


def dict_isz(lkeys, lcounts, rkeys, rcounts):
    """closed form: sum over the shared keys of min(w_l, w_r), w = 1 without counts"""
    l = {int(k): (1 if lcounts is None else int(c)) for k, c in zip(lkeys, lkeys if lcounts is None else lcounts)}
    r = {int(k): (1 if rcounts is None else int(c)) for k, c in zip(rkeys, rkeys if rcounts is None else rcounts)}
    return sum(min(w, r[k]) for k, w in l.items() if k in r)


def isz_matrix(sets, weighted):
    """the N x N matrix of dict_isz (Python ints in a uint64 array), by sorted-array intersection"""
    n = len(sets)
    out = np.zeros((n, n), np.uint64)
    for i in range(n):
        for j in range(i, n):
            _, ia, ib = np.intersect1d(sets[i][0], sets[j][0], assume_unique=True, return_indices=True)
            v = int(np.minimum(sets[i][1][ia].astype(np.uint64), sets[j][1][ib].astype(np.uint64)).sum()) if weighted else int(ia.size)
            out[i, j] = out[j, i] = v
    return out


def ut(matrix, r0=0, r1=None):
    """rows [r0, r1) of the condensed upper triangle, (0,1),(0,2)...(1,2)..., of a square matrix"""
    n = matrix.shape[0]
    r1 = n if r1 is None else r1
    return np.array([matrix[i, j] for i in range(r0, r1) for j in range(i + 1, n)], matrix.dtype)


# ---------------------------------------------------------------- the measures
def measure_value(isz, lhc, rhc, measure, k):
    """CORRECT_RES on double res = isz (cmp_core.cpp:519-526,559), assigned to a long double, NaN / Inf -> its maximum (:573-575), cast
    to float.  UNION_SIZE: lhc + rhc - res (not the reference's isz)"""
    with np.errstate(all="ignore"):
        res, lhc, rhc = np.float64(isz), np.float64(lhc), np.float64(rhc)
        if measure == SYMMETRIC_CONTAINMENT:
            res = res / min(lhc, rhc)
        elif measure in (POISSON_LLR, SIMILARITY):
            res = res / (lhc + rhc - res)
            if measure == POISSON_LLR:                                     # sim2dist, :361
                res = np.float64(math.log(2. * res / (1. + res))) * np.float64(-1. / max(1, k)) if res else np.float64(np.inf)
        elif measure == CONTAINMENT:
            res = res / lhc
        elif measure == UNION_SIZE:
            res = lhc + rhc - res
        ret = LD(res)
        if np.isnan(ret) or np.isinf(ret):
            ret = np.finfo(LD).max
        return np.float32(ret)


def measure_ut(iszm, cards, measure, k, r0=0, r1=None):
    n = iszm.shape[0]
    r1 = n if r1 is None else r1
    return np.array([measure_value(int(iszm[i, j]), cards[i], cards[j], measure, k) for i in range(r0, r1) for j in range(i + 1, n)], np.float32)


# ---------------------------------------------------------------- files
def makedest(path, k, canon=True, seed=0, count_threshold=0.0, outprefix=""):
    """makedest (fastxmerge.cpp:70-120) for --set and --countdict alike: <path>[.seed<s>][.rc_canon].k<k>[.ct_threshold<c>].FullMmerSet.DNA.kmerset64"""
    ret = path.split(" ")[0]
    if outprefix:
        ret = outprefix + "/" + path[path.rfind("/") + 1:]                 # trim_folder takes the whole line (enums.cpp:22-26)
    if seed:
        ret += f".seed{seed}"
    if canon:
        ret += ".rc_canon"
    ret += f".k{k}"
    if count_threshold > 0:
        ret += ".ct_threshold" + (f"{count_threshold:f}" if math.fmod(count_threshold, 1.) else str(int(count_threshold)))
    return ret + ".FullMmerSet.DNA.kmerset64"


def counts_path(keyfile):
    """the key file's name up to its last '.' plus .kmercounts.f64 (fastxsketch.cpp:314,317)"""
    return keyfile[:keyfile.rfind(".")] + ".kmercounts.f64"


def key_file_bytes(keys, counts, weighted):
    """[f64 card][u64 h x |E|]; the header is what the reference writes for the mode: |E| or the sum of the counts"""
    return np.float64(card(keys, counts, weighted)).tobytes() + np.asarray(keys, np.uint64).tobytes()


def count_file_bytes(counts):
    """[f64 c x |E|], no header"""
    return np.asarray(counts, np.float64).tobytes()


def read_set(key_bytes, count_bytes=None):
    """the LOADED form: |E| from the size minus the header, counts and their sum from the count file, never from the header
    -> (keys, counts or None, card)"""
    assert len(key_bytes) >= 8 and len(key_bytes) % 8 == 0
    keys = np.frombuffer(key_bytes, np.uint64)[1:]
    if count_bytes is None:
        return keys, None, int(keys.size)
    cf = np.frombuffer(count_bytes, np.float64)
    assert cf.size == keys.size and (cf == np.floor(cf)).all() and (cf >= 1).all() and (cf < 2.0 ** 32).all()
    counts = cf.astype(np.uint32)
    return keys, counts, int(counts.astype(np.uint64).sum())


# ---------------------------------------------------------------- constructed sets (answers known without running anything)
def rng_keys(seed, n, lo=0, hi=2 ** 64):
    """n distinct uniform keys in [lo, hi), ascending"""
    rng = np.random.default_rng(seed)
    span = hi - lo
    out = set()
    while len(out) < n:
        need = n - len(out)
        draw = rng.integers(0, 2 ** 63, need + 16, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, need + 16).astype(object)
        out.update(int(lo + (int(x) % span)) for x in draw)
    return np.sort(np.array(list(out)[:n], np.uint64))
