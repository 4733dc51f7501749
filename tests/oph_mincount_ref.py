"""One-Permutation set sketches over the k-mers seen at least c times (sketch -m c in set space): the reference of
test_oph_mincount_ref.py, test_gpu_oph_mincount.py and test_gpu_cli_mincount.py (test infrastructure; held to its own properties
by test_oph_mincount_ref.py).  No GPU and no library call in here.

    sequential   LazyOnePermSetSketch::update under set_mincount(c) (src/oph.h:154-159,176-211), one k-mer at a time, in Python
                 integers: the per-register map `potentials_` of the ids below the register, the promotion of an id on its c-th
                 occurrence, the erasure of the potentials at or above it; c <= 1 is the plain branch (oph_kmers_ref.sequential)
    closed_form  the same result from the distinct masked k-mers and their multiplicities: register = the smallest id of its bucket
                 among the keys with count >= c (oph_kmers_ref.closed_form over those), count = oph_kmers_ref.counts_for over ALL
                 keys -- every occurrence of the k-mer whose id equals the final register, so a register that stayed ~0 counts a
                 k-mer whose id is 2^64-1 however rarely it occurs
    variants     the two mistakes a kernel could make, for detection power only: 'gt' keeps count > c; 'thresholded_counts' counts
                 only over the keys that passed the threshold
    cases        the inputs of the GPU tests, as k3_seam_cases.Batch objects, with the conditions that make them bite"""
import functools

import numpy as np

import k3_seam_cases as C
import oph_kmers_ref as R

M64 = R.M64
SEEDED = 0x9E3779B97F4A7C15                                            # a "seeded" xormask: any non-zero value is one


def sequential(stream_of_masked_kmers, m, c, variant=None):
    """update() for every element of the stream, in order -> (registers: list of int, counts: list of int)"""
    if not c > 1:                                                      # set_mincount: `if(v > 1.)`
        return R.sequential(stream_of_masked_kmers, m)
    regs, cnts = [M64] * m, [0] * m
    potentials = [dict() for _ in range(m)]
    for oid in stream_of_masked_kmers:
        i = R.oph_id_int(int(oid))
        idx = (i & 0xFFFFFFFF) % m
        if regs[idx] > i:
            pos = potentials[idx]
            pos[i] = pos.get(i, 0) + 1
            if (pos[i] > c) if variant == "gt" else (pos[i] >= c):
                regs[idx], cnts[idx] = i, pos[i]
                for p in [p for p in pos if p >= i]:
                    del pos[p]
        else:
            cnts[idx] += regs[idx] == i
    return regs, cnts


def closed_form(keys, counts, m, c, variant=None):
    """distinct masked k-mers and their multiplicities -> (registers uint64[m], counts uint32[m])"""
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
    if not c > 1:
        return R.closed_form(keys, counts, m)
    keep = counts > c if variant == "gt" else counts >= c
    regs, _ = R.closed_form(keys[keep], counts[keep], m)
    if variant == "thresholded_counts":
        return regs, R.counts_for(keys[keep], counts[keep], regs)
    return regs, R.counts_for(keys, counts, regs)


def expected(batch, S, c, drop=None, variant=None):
    """a Batch -> (registers uint64 [n][m], counts uint32 [n][m]), read-only; drop = keys that a filter removes before anything counts"""
    m = R.oph_m(S)
    regs, cnts = np.empty((len(batch.genomes), m), np.uint64), np.empty((len(batch.genomes), m), np.uint32)
    for g, (keys, counts, _) in enumerate(batch.counts()):
        if drop is not None:
            keep = ~np.isin(keys, drop)
            keys, counts = keys[keep], counts[keep]
        regs[g], cnts[g] = closed_form(keys, counts, m, c, variant)
    regs.setflags(write=False)
    cnts.setflags(write=False)
    return regs, cnts


# ---------------------------------------------------------------- the >= seam, by construction
SEAM_C, SEAM_S, SEAM_K = (2, 3, 4), (1, 7, 64, 1024), (11, 21, 32)
SEAM_GENOMES = 2


def _disjoint_once(parts, k, canon):
    """every part's k-mers occur once in it, and no k-mer is in two parts"""
    sets = [C._record_kmers(p, k, canon) for p in parts]
    flat = [x for s in sets for x in s]
    return len(set(flat)) == len(flat)


@functools.lru_cache(maxsize=None)
def ge_seam(c, S, k, canon):
    """SEAM_GENOMES genomes, each of three disjoint random sequences: A once, B c times, D c - 1 times (records interleaved, B never
    first).  Only B's k-mers reach c, so the registers are the plain sketch of B alone and every count is c (0 where B has no
    k-mer).  The seeds are tried in order until (checked here and again in test_oph_mincount_ref.py) the sequences are disjoint,
    the plain sketch of A + B + D differs from the expected one, and at least one register's plain winner occurs exactly c - 1
    times -- the winner a kernel keeps if it selects with `>` shifted by one or not at all.
    -> (Batch, expected registers [n][m], expected counts [n][m])"""
    m = R.oph_m(S)
    xormask = 0 if canon else SEEDED
    genomes, eregs, ecnts = [], [], []
    seed = 7000 + 1000 * c + 10 * k + int(canon)
    while len(genomes) < SEAM_GENOMES:
        seed += 100_000
        rng = np.random.default_rng(seed + S)
        A, B, D = (C.random_bases(rng, n + k - 1) for n in (260, 200, 230))
        if not _disjoint_once((A, B, D), k, canon):
            continue
        records = [D] * (c - 1) + [A] + [B] * c
        records = [records[i] for i in rng.permutation(len(records))]
        keys, counts, _ = C.key_counts(tuple(records), k, canon, xormask)
        plain_regs, plain_cnts = R.closed_form(keys, counts, m)
        bregs, bcnts = R.genome_closed_form([B], k, canon, xormask, S)
        if np.array_equal(plain_regs, bregs) or not (plain_cnts == c - 1).any():
            continue
        genomes.append(records)
        eregs.append(bregs)
        ecnts.append(bcnts * np.uint32(c))
    batch = C.Batch(f"ge_c{c}_S{S}_k{k}_{'canon' if canon else 'fwd'}", k, S, canon, xormask, genomes)
    return batch, np.array(eregs), np.array(ecnts)


# ---------------------------------------------------------------- planted counts 1 .. 4, an empty genome, one shorter than k
@functools.lru_cache(maxsize=None)
def planted():
    """k3_seam_cases.planted_counts() (40 k-mers each of count 1, 2, 3, 4; a genome that has only count 2), then a genome without a
    record and one whose only record is shorter than k"""
    p = C.planted_counts()
    return C.Batch("planted_mincount", p.k, p.S, p.canon, p.xormask, list(p.genomes) + [[], ["ACGTACGTACGT"]])


# ---------------------------------------------------------------- the id 2^64 - 1
@functools.lru_cache(maxsize=None)
def ones_id():
    """k = 32, not canonical, S = 4, c = 3.  The xormask makes the OPH id of x0 -- a k-mer that occurs once -- all ones; it maps to
    register 0xFFFFFFFF % 4 = 3.  Genome 0: a 300-base record that holds x0 and nothing three times: every register stays ~0, and
    register 3 counts 1 (`rref > id` is false, `rref == id` is true).  Genome 1: the same record and a 70-base unit three times, of
    which at least one k-mer maps to register 3: the register is that winner's id and the count is 3.
    -> (Batch, c, register of the id ~0)"""
    k, S, c = 32, 4, 3
    rng = np.random.default_rng(7700)
    while True:
        rec, unit = C.random_bases(rng, 300), C.random_bases(rng, 70)
        if not _disjoint_once((rec, unit), k, False):
            continue
        x0 = C._record_kmers(rec, k, False)[111]
        masked = int(R.wang64_inverse(np.array([M64], np.uint64))[0]) ^ R.OPHXOR     # the masked k-mer whose id is ~0
        xormask = int(R.wang64_inverse(np.array([masked], np.uint64))[0]) ^ x0
        batch = C.Batch("ones_id", k, S, False, xormask, [[rec], [unit, rec, unit, unit]])
        regs, cnts = expected(batch, S, c)
        r = (M64 & 0xFFFFFFFF) % R.oph_m(S)
        if regs[1][r] != M64:
            return batch, c, r


# ---------------------------------------------------------------- a filter
@functools.lru_cache(maxsize=None)
def filtered(c, canon):
    """one genome: a 500-base backbone once and a 90-base unit c times (k = 21, S = 16).  The filter input is ONE k-mer of the unit,
    the one behind the smallest register of the unfiltered expectation: with the filter it is gone (its register goes to the next
    candidate or to ~0) and every other k-mer of the unit, its neighbours included, stays.
    -> (Batch, filter record, the masked key the filter removes)"""
    k, S = 21, 16
    rng = np.random.default_rng(7800 + c)
    while True:
        backbone, unit = C.random_bases(rng, 500), C.random_bases(rng, 90)
        if not _disjoint_once((backbone, unit), k, True):              # canonical-disjoint is forward-disjoint too
            continue
        batch = C.Batch(f"filtered_c{c}_{'canon' if canon else 'fwd'}", k, S, canon, 0, [[unit] * (c - 1) + [backbone, unit]])
        regs, _ = expected(batch, S, c)
        win = int(regs[0][regs[0] != M64].min())
        key = int(R.decode(np.array([win], np.uint64))[0])
        x = int(R.wang64_inverse(np.array([key], np.uint64))[0]) ^ batch.xormask
        record = "".join(C.LETTERS[(x >> (2 * (k - 1 - j))) & 3] for j in range(k))
        assert C._record_kmers(record, k, canon) == (x,) and x in C._record_kmers(unit, k, canon)
        return batch, record, np.array([key], np.uint64)


# ---------------------------------------------------------------- K3's own seams
def doubled(batch):
    """every record of every genome twice: all counts double, the buckets hold twice the keys"""
    return C.Batch(batch.name + "_x2", batch.k, batch.S, batch.canon, batch.xormask, [list(g) * 2 for g in batch.genomes])
