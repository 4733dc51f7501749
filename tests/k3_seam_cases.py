"""Inputs at the seams of K3, the --multiset path (d2g_k3_bmh.hip), with what they must give (test infrastructure for
test_gpu_k3_seams.py; held to its stated properties, on the reference alone, by test_k3_seam_cases.py).  No GPU in here.

Genomes are lists of plain ACGT records, so no parser decides anything.  The expected (key, count) sets come from a pure-Python
rolling enumerator and the key transform wang64(kmer ^ xormask) in NumPy (k0_ref.wang64), never from the oracle's FASTA walk; the
expected registers and total weights come from oracle.bmh_from_weighted(keys, float64(counts), S), the sequential time-ordered
heap algorithm, over those keys.

The seams (each generator's docstring says what it plants):
    a  the key ~0, which marks a free slot of the LDS count table and so is counted beside the table   (generic path)
    b  the stored word 0xFFFFFFFF of every k-mer that ends in sixteen T                                  (compact path)
    c  one bucket of 1399 .. 5601 keys: one unguarded round, two rounds, four, the once-more split
    d  counts 1, 2, 3, 4 under thresholds on, between and far above them
    e  counts on, below and above the edges of the 65 top-level weight strips
    f  explicit weights: the doubles below, at and above every strip edge

No weight below WEIGHT_FLOOR = 2^-200 is ever emitted, and every explicit set passes d2g_bmh_check_weights: a set that the
library refuses (a total weight so small that the pruning bound could reach +inf) must reach neither a GPU nor the oracle, whose
heap loop does not end on one either."""
import functools
import math
import os
import re

import numpy as np

import k0_ref

M64 = 0xFFFFFFFFFFFFFFFF
WEIGHT_FLOOR = 2.0 ** -200
LETTERS = "ACGT"
_CODE = {c: i for i, c in enumerate(LETTERS)}
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dashing2_amd", "csrc")


def _oracle():
    from oracle import oracle as O
    O.load()
    return O


def _d2g():
    import dashing2_amd as D
    return D


# ---------------------------------------------------------------- the constants of the kernel, read from its source
def k3_constants():
    """K3_ROUND_KEYS, K3_TARGET, K3_SPLIT_MIN, K3_MAXBBITS (d2g_internal.h) and K3_TAB (d2g_k3_bmh.hip)"""
    text = open(os.path.join(_CSRC, "d2g_internal.h")).read() + open(os.path.join(_CSRC, "d2g_k3_bmh.hip")).read()
    out = {}
    for name in ("K3_ROUND_KEYS", "K3_TARGET", "K3_SPLIT_MIN", "K3_MAXBBITS", "K3_TAB"):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9 *]+);", text)
        assert m, name
        out[name] = math.prod(int(f) for f in m.group(1).split("*"))
    return out


def table_rounds(rn, c=None):
    """what k3_bmh_main_kernel does with one bucket of rn keys of a genome that has a single bucket, under the default switches:
    ('split', sub-range bits) when the host splits the bucket once more, else (R rounds, unguarded insert?)"""
    c = c or k3_constants()
    if rn > c["K3_SPLIT_MIN"]:
        return "split", min(c["K3_MAXBBITS"], ((rn + c["K3_TARGET"] - 1) // c["K3_TARGET"] - 1).bit_length())
    R = 1
    while R * c["K3_ROUND_KEYS"] < rn:
        R <<= 1
    return R, R == 1 and rn < c["K3_TAB"]


# ---------------------------------------------------------------- k-mers and keys
def random_bases(rng, n):
    return "".join(LETTERS[i] for i in rng.integers(0, 4, n))


@functools.lru_cache(maxsize=None)
def _record_kmers(record, k, canon):
    """the k-mers of one record, rolled one base at a time: forward value (first base most significant) or the smaller of it and
    its reverse complement"""
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fwd = rc = 0
    out = []
    for j, ch in enumerate(record):
        c = _CODE[ch]
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if j >= k - 1:
            out.append(min(fwd, rc) if canon else fwd)
    return tuple(out)


def kmers_of(records, k, canon):
    return [x for r in records for x in _record_kmers(r, k, canon)]


def key_counts(records, k, canon, xormask):
    """-> (keys uint64 sorted, counts uint32, number of k-mers) of one genome"""
    kmers = np.array(kmers_of(records, k, canon), np.uint64)
    keys, counts = np.unique(k0_ref.wang64(kmers ^ np.uint64(xormask)), return_counts=True)
    return keys, counts.astype(np.uint32), int(kmers.size)


def fasta(records, name="g"):
    return b"".join(b">%s_%d\n%s\n" % (name.encode(), i, r.encode()) for i, r in enumerate(records))


def ones_mask(x0):
    """the xormask under which the masked key of k-mer x0 is ~0"""
    mask = _oracle().wang_inverse(M64) ^ x0
    assert int(k0_ref.wang64(np.array([x0 ^ mask], np.uint64))[0]) == M64
    return mask


class Batch:
    """genomes (lists of ACGT records) that go through K3 in one call, and what must come back"""

    def __init__(self, name, k, S, canon, xormask, genomes, thresholds=(0.0,), note=None):
        self.name, self.k, self.S, self.canon, self.xormask = name, k, S, canon, xormask
        self.genomes, self.thresholds, self.note = genomes, tuple(thresholds), note or {}
        self._counts, self._exp = None, {}

    def __repr__(self):
        return self.name

    def fastas(self):
        return [fasta(g, f"{self.name}{i}") for i, g in enumerate(self.genomes)]

    def nkmers(self):
        return [sum(max(0, len(r) - self.k + 1) for r in g) for g in self.genomes]

    def counts(self):
        """per genome (keys, counts, nk): every distinct key, no threshold"""
        if self._counts is None:
            self._counts = [key_counts(tuple(g), self.k, self.canon, self.xormask) for g in self.genomes]
        return self._counts

    def expected(self, thr):
        """per genome (keys, counts, registers float64[S], total weight) of the elements with float64(count) > thr"""
        if thr not in self._exp:
            O = _oracle()
            out = []
            for keys, counts, _ in self.counts():
                keep = counts.astype(np.float64) > thr
                kk, cc = keys[keep], counts[keep]
                assert cc.size == 0 or cc.min() >= WEIGHT_FLOOR            # counts are weights >= 1
                sig, tw = O.bmh_from_weighted(kk, cc.astype(np.float64), self.S)
                assert tw == float(cc.astype(np.uint64).sum())
                sig.setflags(write=False)
                out.append((kk, cc, sig, tw))
            self._exp[thr] = out
        return self._exp[thr]


# ---------------------------------------------------------------- a. the all-ones key, generic path
@functools.lru_cache(maxsize=None)
def all_ones_generic(which):
    """k = 21, canonical, S = 16: a 20 000-base backbone record and three records of one 40-base unit; the xormask makes the key of
    x0 all ones, x0 = a k-mer of the backbone (count 1) or of the unit (count 3).  Threshold 3.0 drops the count-3 elements."""
    rng = np.random.default_rng(2101)
    k = 21
    backbone, unit = random_bases(rng, 20_000), random_bases(rng, 40)
    records = [backbone, unit, unit, unit]
    x0, count = {"backbone": (_record_kmers(backbone, k, True)[7777], 1), "unit": (_record_kmers(unit, k, True)[5], 3)}[which]
    return Batch(f"ones_{which}", k, 16, True, ones_mask(x0), [records], (0.0, 1.0, 2.0, 3.0), {"x0": x0, "count": count})


@functools.lru_cache(maxsize=None)
def all_ones_only():
    """a poly-A genome whose ONLY element is the key ~0 (canonical poly-A is the k-mer 0; 200 bases: count 180), a genome that
    holds the key in an A-run among other k-mers, and an empty genome"""
    rng = np.random.default_rng(2102)
    k = 21
    with_run = [random_bases(rng, 700) + "C" + "A" * 30 + "G" + random_bases(rng, 500), random_bases(rng, 90)]
    return Batch("ones_only", k, 16, True, ones_mask(0), [["A" * 200], with_run, []], (0.0, 9.0, 10.0, 180.0),
                 {"x0": 0, "counts": (180, 10, None)})


# ---------------------------------------------------------------- b. the all-ones stored word, compact path
@functools.lru_cache(maxsize=None)
def all_ones_compact(k):
    """not canonical (a canonical k-mer that ends in T... has a reverse complement that begins with A... and loses to it).  The stored
    word of the compact path is the k-mer's low 32 bits: 0xFFFFFFFF for every k-mer that ends in sixteen T.  Genome 0: runs of k + 4
    T (five all-T k-mers) and eight random prefixes before sixteen T -- at k > 16 these differ in their high bits, so that several
    buckets get such a word; genome 1: nothing but k + 5 T; genome 2: no such k-mer at all."""
    assert 16 <= k <= 21
    rng = np.random.default_rng(2200 + k)
    g0 = [random_bases(rng, 3000) + "G" + "T" * (k + 4) + "C" + random_bases(rng, 700), "T" * (k + 4)]
    g0 += [random_bases(rng, 60) + "ACG"[i % 3] + "T" * 16 + "G" + random_bases(rng, 45) for i in range(8)]
    g2 = [random_bases(rng, 2500)]
    assert "T" * 16 not in g2[0]
    return Batch(f"compact_k{k}", k, 16, False, 0x1234, [g0, ["T" * (k + 5)], g2], (0.0, 1.0, 9.0, 10.0))


def ends_in_sixteen_t(batch, gi):
    """the keys of genome gi's k-mers whose low 32 bits are all ones"""
    x = np.array(kmers_of(batch.genomes[gi], batch.k, batch.canon), np.uint64)
    x = x[(x & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF)]
    return np.unique(k0_ref.wang64(x ^ np.uint64(batch.xormask)))


# ---------------------------------------------------------------- c. table rounds
ROUND_SIZES = (1399, 1400, 1401, 2047, 2048, 2049, 2799, 2800, 2801, 5600, 5601)
ROUND_ENV = {"D2G_K3_BUCKET_KEYS": "1000000"}                          # one bucket per genome


@functools.lru_cache(maxsize=None)
def table_round_genomes():
    """one genome of nk DISTINCT k-mers per seam size, each a single record (k = 21, canonical, S = 16); with ROUND_ENV every
    genome is one bucket of nk keys"""
    rng = np.random.default_rng(2300)
    k = 21
    return Batch("rounds", k, 16, True, 0, [[random_bases(rng, nk + k - 1)] for nk in ROUND_SIZES])


# ---------------------------------------------------------------- d. count threshold
THRESHOLDS = (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 1e10, 4294967295.0)


@functools.lru_cache(maxsize=None)
def planted_counts():
    """four 60-base units, unit c in c records: 40 k-mers each of count 1, 2, 3, 4 (k = 21, canonical, S = 16); a second genome
    that has only count 2"""
    rng = np.random.default_rng(2400)
    units = [random_bases(rng, 60) for _ in range(4)]
    g0 = [u for c, u in enumerate(units, 1) for _ in range(c)]
    u = random_bases(rng, 333)
    return Batch("thresholds", 21, 16, True, 0, [g0, [u, u]], THRESHOLDS)


# ---------------------------------------------------------------- e. counts at the edges of the top-level strips
TOP_EDGES = [float(t) for t in range(17)] + [2.0 ** j for j in range(5, 54)]       # top_edge(0 .. 65): 65 strips
EDGE_COUNTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4096, 4097)
assert len(TOP_EDGES) == 66


def top_strip_floor(w):
    """lower edge of the highest strip an element of weight w reaches: the largest edge below w"""
    return max(e for e in TOP_EDGES if e < w)


def bmh_guess(W, S):
    """bmh_guess of d2g_k3_bmh.hip"""
    return 1.25 * (float(S) / W) * (math.log(float(S)) + 0.58 + 8.0)


def predicted_light(nkmers, S):
    """the host's rule for the form of the first pass (K3Run::sketch): light unless the strips expected to survive it,
    sum gk min(1, guess), exceed an eighth of the batch's k-mers"""
    etot = sum(gk * min(1.0, bmh_guess(max(gk, 1), S)) for gk in nkmers)
    return etot <= 0.125 * sum(nkmers)


@functools.lru_cache(maxsize=None)
def strip_edge_counts(extra=None):
    """one genome per c in EDGE_COUNTS: c records of one (k + 7)-base unit = eight distinct k-mers of count exactly c (k = 21,
    canonical, S = 64), all in one batch.  extra = 'big': a 300 000-base genome joins them; extra = 'small': only c <= 1025, a
    batch whose first pass the host predicts heavy (the full batch is predicted light)"""
    rng = np.random.default_rng(2503)
    k = 21
    cs = EDGE_COUNTS
    genomes = []
    for c in cs:
        unit = random_bases(rng, k + 7)
        genomes.append([unit] * c)
    if extra == "small":
        genomes = [g for g, c in zip(genomes, cs) if c <= 1025]
        cs = tuple(c for c in cs if c <= 1025)
    if extra == "big":
        genomes.append([random_bases(rng, 300_000)])
    return Batch(f"strip_edges_{extra}", k, 64, True, 0, genomes, note={"counts": cs})


# ---------------------------------------------------------------- f. explicit weights at the level edges
EXTRA_WEIGHTS = (2.0 ** -200, 2.0 ** -64, 0.5, 0.75, 1.5, 15.5, 16.5, 24.0, 3e9)
TOO_LARGE = float(np.nextafter(2.0 ** 53, np.inf))                     # refused on the host


def level_weights():
    """-> (weights, below): for each inner edge and 2^53 the double below, at and above it (above 2^53: refused, not in here),
    then EXTRA_WEIGHTS; below[i] = the next lower edge for a weight that is the double below an edge, else NaN"""
    ws, below = [], []
    for t in range(1, 66):
        e = TOP_EDGES[t]
        for w in (float(np.nextafter(e, 0.0)), e, float(np.nextafter(e, np.inf))):
            if w <= 2.0 ** 53:
                ws.append(w)
                below.append(TOP_EDGES[t - 1] if w < e else math.nan)
    ws += EXTRA_WEIGHTS
    below += [math.nan] * len(EXTRA_WEIGHTS)
    ws = np.array(ws, np.float64)
    assert ws.min() >= WEIGHT_FLOOR and ws.size == 65 * 3 - 1 + len(EXTRA_WEIGHTS)
    return ws, np.array(below, np.float64)


class WeightedSets:
    """explicit sets for d2g_bmh_from_weighted / _ids with the oracle's answer per set"""

    def __init__(self, name, ids, weights, off, S, owners):
        off = np.asarray(off, np.uint64)
        assert weights[weights > 0].min() >= WEIGHT_FLOOR
        _d2g().bmh_check_weights(weights, off, S)                       # raises for a set the library refuses
        self.name, self.ids, self.weights, self.off, self.S, self.owners = name, ids, weights, off, S, owners
        O = _oracle()
        self.sig = np.empty((off.size - 1, S), np.float64)
        self.tw = np.empty(off.size - 1, np.float64)
        self.own = np.empty((off.size - 1, S), np.uint64) if owners else None
        for i in range(off.size - 1):
            lo, hi = int(off[i]), int(off[i + 1])
            if owners:
                self.sig[i], self.tw[i], self.own[i] = O.bmh_from_weighted_ids(ids[lo:hi], weights[lo:hi], S)
            else:
                self.sig[i], self.tw[i] = O.bmh_from_weighted(ids[lo:hi], weights[lo:hi], S)
        for a in (self.ids, self.weights, self.off, self.sig, self.tw):
            a.setflags(write=False)

    def __repr__(self):
        return self.name


def _level_ids():
    return np.random.default_rng(2600).integers(0, 2 ** 63, level_weights()[0].size).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def weights_one_per_set(S):
    """(i) one element per set"""
    ws, _ = level_weights()
    return WeightedSets(f"one_per_set_S{S}", _level_ids(), ws, np.arange(ws.size + 1), S, True)


@functools.lru_cache(maxsize=None)
def weights_one_set():
    """(ii) all of them in one set, S = 64"""
    ws, _ = level_weights()
    return WeightedSets("one_set", _level_ids(), ws, [0, ws.size], 64, True)


CROWD = 2049                                                           # with the seam element: two workgroups of 2048 elements


@functools.lru_cache(maxsize=None)
def weights_in_a_crowd():
    """(iii) every seam weight as the LAST element of a set of 2049 random-weight elements (the second workgroup's only
    element), S = 64; the crowd is the same in every set and weighs about 2300 in all, so that the seam elements from 2^5 or so
    upwards own registers"""
    ws, _ = level_weights()
    rng = np.random.default_rng(2601)
    cid = rng.integers(0, 2 ** 63, CROWD).astype(np.uint64)
    cw = rng.random(CROWD) * 10 ** rng.integers(-3, 2, CROWD).astype(np.float64) + WEIGHT_FLOOR
    ids = np.concatenate([np.concatenate([cid, [i]]) for i in _level_ids()]).astype(np.uint64)
    w = np.concatenate([np.concatenate([cw, [x]]) for x in ws])
    return WeightedSets("in_a_crowd", ids, w, np.arange(ws.size + 1) * (CROWD + 1), 64, False)
