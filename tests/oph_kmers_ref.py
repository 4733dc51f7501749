"""The k-mers and counts behind One-Permutation SetSketch registers (sketch -s / -N): the reference of test_oph_kmers_host.py,
test_gpu_oph_kmers.py and test_gpu_cli_kmers.py (test infrastructure; held to its own properties by test_oph_kmers_ref.py).  No GPU
and no library call in here.

    sequential   LazyOnePermSetSketch::update's plain branch (src/oph.h:176-186,207-209), one k-mer at a time, in Python integers
    closed_form  the same result from the distinct masked k-mers and their multiplicities (k3_seam_cases.key_counts: a pure-Python
                 rolling enumerator and NumPy's wang64): register = the smallest id of its bucket, count = that id's multiplicity
    decode       DHasher::inverse (src/oph.h:50-52,81-83): a NumPy inverse of Thomas Wang's published 64-bit mix
    writers      <out>.kmer64, <out>.kmer64.names.txt, <out>.kmercounts.f64 and the third column of <out>.names.txt as the reference
                 writes them (src/fastxsketch.cpp:245-263,314-317,326,619-622; src/sketch_core.cpp:146-171)

Both forms start from registers ~0 and counts 0 and never treat ~0 specially: a k-mer whose id is 2^64-1 finds `rref > id` false and
`rref == id` true, so it counts and the register stays ~0."""
import numpy as np

import k0_ref
import k3_seam_cases as C

M64 = 0xFFFFFFFFFFFFFFFF
MT_SEED = 0x321b919a61cb41f7                                           # oph.h:142
CEIXOR = 0x533f8c2151b20f97                                            # oph.h:46


def _mt19937_64_first(seed):
    """the first output of std::mt19937_64(seed) (the published MT19937-64 recurrence)"""
    nn, mm = 312, 156
    mt = [0] * nn
    mt[0] = seed & M64
    for i in range(1, nn):
        mt[i] = (6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & M64
    x = (mt[0] & 0xFFFFFFFF80000000) | (mt[1] & 0x7FFFFFFF)
    x = mt[mm] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
    x ^= (x >> 29) & 0x5555555555555555
    x ^= (x << 17) & 0x71D67FFFEDA60000
    x ^= (x << 37) & 0xFFF7EEE000000000
    x ^= x >> 43
    return x & M64


OPHXOR = _mt19937_64_first(MT_SEED) ^ CEIXOR                           # DHasher: seed_ ^ CEIXOR (oph.h:59,70-71)


def oph_m(S):
    return S + (S & 1)                                                 # oph.h:143-146


def wang64_int(k):
    k = (~k + (k << 21)) & M64
    k ^= k >> 24
    k = (k + (k << 3) + (k << 8)) & M64
    k ^= k >> 14
    k = (k + (k << 2) + (k << 4)) & M64
    k ^= k >> 28
    return (k + (k << 31)) & M64


def oph_id_int(masked):
    """hasher_(oid) of oph.h:178 for a masked k-mer maskfn(kmer) = wang64(kmer ^ xormask)"""
    return wang64_int(masked ^ OPHXOR)


def sequential(stream_of_masked_kmers, m, skip_empty=False):
    """update() for every element of the stream, in order -> (registers: list of int, counts: list of int).
    skip_empty = True is the WRONG variant that never counts against an empty register (detection power only)."""
    regs, cnts = [M64] * m, [0] * m
    for oid in stream_of_masked_kmers:
        i = oph_id_int(int(oid))
        idx = (i & 0xFFFFFFFF) % m                                     # Schismatic<uint32_t>::mod: the argument narrowed to 32 bits
        if regs[idx] > i:
            regs[idx], cnts[idx] = i, 1
        elif not (skip_empty and regs[idx] == M64):
            cnts[idx] += regs[idx] == i
    return regs, cnts


def closed_form(keys, counts, m):
    """distinct masked k-mers and their multiplicities -> (registers uint64[m], counts uint32[m])"""
    keys = np.asarray(keys, np.uint64)
    counts = np.asarray(counts, np.uint64)
    regs, cnts = np.full(m, M64, np.uint64), np.zeros(m, np.uint32)
    if keys.size == 0:
        return regs, cnts
    ids = k0_ref.wang64(keys ^ np.uint64(OPHXOR))
    assert np.unique(ids).size == ids.size                             # the mix is a bijection
    idx = ((ids & np.uint64(0xFFFFFFFF)) % np.uint64(m)).astype(np.int64)
    order = np.lexsort((ids, idx))                                     # by bucket, then by id: the first of a bucket is its minimum
    first = np.ones(order.size, bool)
    first[1:] = idx[order][1:] != idx[order][:-1]
    w = order[first]
    regs[idx[w]] = ids[w]
    cnts[idx[w]] = counts[w].astype(np.uint32)
    return regs, cnts


def counts_for(keys, counts, regs):
    """what d2g_oph_count_dev defines for ANY registers: counts[r] = the k-mers whose id equals regs[r] and maps to r"""
    regs = np.asarray(regs, np.uint64)
    m = regs.size
    out = np.zeros(m, np.uint32)
    keys = np.asarray(keys, np.uint64)
    if keys.size:
        ids = k0_ref.wang64(keys ^ np.uint64(OPHXOR))
        idx = ((ids & np.uint64(0xFFFFFFFF)) % np.uint64(m)).astype(np.int64)
        hit = regs[idx] == ids
        out[idx[hit]] = np.asarray(counts, np.uint32)[hit]
    return out


def genome_closed_form(records, k, canon, xormask, S):
    """one genome (a list of ACGT records) -> (registers uint64[m], counts uint32[m])"""
    keys, counts, _ = C.key_counts(tuple(records), k, canon, xormask)
    return closed_form(keys, counts, oph_m(S))


def masked_stream(records, k, canon, xormask):
    """maskfn(kmer) of every k-mer of the genome, in order (for `sequential`)"""
    return [wang64_int(x ^ xormask) for x in C.kmers_of(records, k, canon)]


def wang64_inverse(y):
    """NumPy inverse of the mix, step by step from the last to the first: y = x + (x << s) (and y = ~x + (x << s)) gives s more low
    bits of x per substitution, y = x ^ (x >> s) s more high bits; 21 = 1 + 4 + 16 and 265 = 1 + 8 + 256 are inverted modulo 2^64"""
    y = np.array(y, np.uint64, ndmin=1)
    u = np.uint64
    with np.errstate(over="ignore"):
        x = y.copy()
        for _ in range(3):
            x = y - (x << u(31))
        y = x.copy()
        for _ in range(3):
            x = y ^ (x >> u(28))
        y = x * u(pow(21, -1, 1 << 64))
        x = y.copy()
        for _ in range(5):
            x = y ^ (x >> u(14))
        y = x * u(pow(265, -1, 1 << 64))
        x = y.copy()
        for _ in range(3):
            x = y ^ (x >> u(24))
        y = x.copy()
        x = ~y
        for _ in range(4):
            x = ~(y - (x << u(21)))
    return x


def decode(regs):
    """ids(): the masked k-mer behind every register (any shape), oph.h:264-271"""
    regs = np.asarray(regs, np.uint64)
    return (wang64_inverse(regs.ravel()) ^ np.uint64(OPHXOR)).reshape(regs.shape)


# ---------------------------------------------------------------- the files
def kmer64_bytes(ids, S, k, w, canon, seedseed):
    """<out>.kmer64: u32 dtype = DNA (0) | canon << 8, u32 S, u32 k, u32 w, u64 seedseed, then [n][S] u64 (w: what the writer is given,
    k where the CLI's w_ is negative)"""
    ids = np.ascontiguousarray(ids, np.uint64)
    assert ids.ndim == 2 and ids.shape[1] == S
    return np.array([int(bool(canon)) << 8, S, k, w], np.uint32).tobytes() + np.array([seedseed], np.uint64).tobytes() + ids.tobytes()


def kmer64_names_bytes(lines):
    return b"".join(l.encode() + b"\n" for l in lines)


def kmercounts_bytes(counts, S):
    """<out>.kmercounts.f64: float32 in spite of the name (SketchingResult::kmercounts_ is a std::vector<float>)"""
    counts = np.ascontiguousarray(counts, np.uint32)
    assert counts.ndim == 2 and counts.shape[1] == S
    return counts.astype(np.float32).tobytes()


def cache_name(path, S, k, canon=True, seedseed=0, outprefix=None):
    """makedest (src/fastxmerge.cpp:70-120) for a DNA One-Permutation set sketch without a count threshold"""
    ret = path.split(" ")[0]
    if outprefix:
        ret = outprefix + "/" + ret[ret.rfind("/") + 1:]
    if seedseed:
        ret += ".seed%d" % seedseed
    if canon:
        ret += ".rc_canon"
    return ret + ".sketchsize%d.k%d.SetSpace.DNA.opss" % (S, k)


def kmercounts_column(path, S, k, canon=True, seedseed=0, outprefix=None):
    """the third column of <out>.names.txt with -N: the cache name with its last extension replaced (fastxsketch.cpp:314,317)"""
    d = cache_name(path, S, k, canon, seedseed, outprefix)
    return d[:d.rfind(".")] + ".kmercounts.f64"


def expected_files(paths, genomes, S, k, w, canon=True, seedseed=0, xormask=0):
    """what `-N -o out` writes for `paths` whose genomes are lists of ACGT records:
    -> dict(kmer64, names, kmercounts: bytes; column: list of str; regs, counts: the [n][m] arrays)"""
    m = oph_m(S)
    regs = np.empty((len(genomes), m), np.uint64)
    counts = np.empty((len(genomes), m), np.uint32)
    for i, g in enumerate(genomes):
        regs[i], counts[i] = genome_closed_form(g, k, canon, xormask, S)
    return {"kmer64": kmer64_bytes(decode(regs[:, :S]), S, k, w, canon, seedseed), "names": kmer64_names_bytes(paths),
            "kmercounts": kmercounts_bytes(counts[:, :S], S), "column": [kmercounts_column(p, S, k, canon, seedseed) for p in paths],
            "regs": regs, "counts": counts}
