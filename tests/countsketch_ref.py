"""The count-sketch of `--multiset -c <cells>` (K3k; reference src/counter.h:16-19,68-77,131-137) as a NumPy model: the reference of
test_countsketch_ref.py, test_gpu_countsketch.py and test_gpu_cli_countsketch.py.  No GPU and no library call in here.

    table          per k-mer x: hv = Wang(Wang(x ^ xormask)); table[hv % cells] += +1 if hv's top bit is set else -1  (int64 sums)
    table_float    the reference's own form: one float32 cell array, one add at a time in the order of the k-mers (counter.h:75)
    lists          finalize (counter.h:131-137): the cells with |c| >= threshold and != 0, ascending: (ids uint64, weights float64, total)
    kmers_*        the k-mers a walker mode emits, from the EXISTING enumerators: minimizer_ref (plain DNA and -w), filter_ref (strings),
                   protein_ref; k3_seam_cases.kmers_of (what oph_kmers_ref stands on) is held equal to the first in test_countsketch_ref.py

The two table forms are equal while no cell's running sum passes 2^24 in magnitude: float32 holds every integer up to there."""
import numpy as np

import filter_ref as FR
import k0_ref
import minimizer_ref as MR
import protein_ref as PR

TOP = np.uint64(1) << np.uint64(63)


def hashes(kmers, xormask=0):
    """hv of every k-mer: Wang of the masked key"""
    x = np.asarray(kmers, np.uint64)
    return k0_ref.wang64(k0_ref.wang64(x ^ np.uint64(xormask)))


def cells_and_signs(kmers, cells, xormask=0):
    hv = hashes(kmers, xormask)
    idx = (hv % np.uint64(cells)).astype(np.int64)                      # `%` on uint64: Schismatic<uint64_t>::mod
    sign = np.where((hv & TOP) != 0, 1, -1).astype(np.int64)            # BM64 clear: -1 (counter.h:75)
    return idx, sign


def table(kmers, cells, xormask=0):
    """the signed table, int64[cells] (dense: small tables)"""
    idx, sign = cells_and_signs(kmers, cells, xormask)
    out = np.zeros(cells, np.int64)
    np.add.at(out, idx, sign)
    return out


def table_float(kmers, cells, xormask=0):
    """the reference's float row, added to one k-mer at a time, in order"""
    idx, sign = cells_and_signs(kmers, cells, xormask)
    out = np.zeros(cells, np.float32)
    for i, s in zip(idx.tolist(), sign.tolist()):
        out[i] = np.float32(out[i] + np.float32(s))
    return out


def sparse_table(kmers, cells, xormask=0):
    """the non-zero cells of a table of any size: (cell numbers ascending uint64, signed sums int64)"""
    idx, sign = cells_and_signs(kmers, cells, xormask)
    if not idx.size:
        return np.empty(0, np.uint64), np.empty(0, np.int64)
    u, inv = np.unique(idx, return_inverse=True)
    s = np.zeros(u.size, np.int64)
    np.add.at(s, inv, sign)
    keep = s != 0
    return u[keep].astype(np.uint64), s[keep]


def compact(ids, sums, threshold=0.0):
    """finalize: |c| >= threshold (counter.h:135), a weight of 0 never passed on -> (ids, weights float64, total int)"""
    v = np.abs(np.asarray(sums, np.int64))
    keep = (v >= threshold) & (v > 0)
    return np.asarray(ids, np.uint64)[keep], v[keep].astype(np.float64), int(v[keep].sum())


def lists(kmers, cells, xormask=0, threshold=0.0):
    return compact(*sparse_table(kmers, cells, xormask), threshold)


def lists_dense(tab, threshold=0.0):
    """the same from a dense table (either form)"""
    tab = np.asarray(tab)
    return compact(np.arange(tab.size, dtype=np.uint64), tab.astype(np.int64), threshold)


def batch_lists(kmers_per_genome, cells, xormask=0, threshold=0.0):
    """-> (ids, weights, set_off uint64[n+1], totals uint64[n]) as d2g_countsketch_cells returns them"""
    ids, ws, off, tot = [], [], [0], []
    for km in kmers_per_genome:
        i, w, t = lists(km, cells, xormask, threshold)
        ids.append(i); ws.append(w); off.append(off[-1] + i.size); tot.append(t)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dt)
    return cat(ids, np.uint64), cat(ws, np.float64), np.array(off, np.uint64), np.array(tot, np.uint64)


def collision_free(kmers, cells, xormask=0):
    """no two DISTINCT k-mers of the input share a cell"""
    d = np.unique(np.asarray(kmers, np.uint64))
    idx, _ = cells_and_signs(d, cells, xormask)
    return np.unique(idx).size == d.size


# ---------------------------------------------------------------- the k-mers of every walker mode, from the existing enumerators
def kmers_dna(fasta: bytes, k, canon, w=0):
    """every k-mer (w <= k) or the minimizer of every window position (w > k) of a FASTA buffer, in order"""
    return np.array(MR.fasta_emissions(fasta, k, w, canon, fast=True), np.uint64)


def kmers_filtered(fasta: bytes, filter_fastas, k, canon):
    """the k-mers that survive --filterset, by filter_ref's strings"""
    fset, _ = FR.filter_set(filter_fastas, k, canon)
    return np.array([FR.encode(w) for w in FR.fasta_windows(fasta, k, canon) if w not in fset], np.uint64)


def kmers_protein(fasta: bytes, k, alphabet):
    return PR.fasta_keys(fasta, k, alphabet)


# ---------------------------------------------------------------- the files and the header line
def cache_name(path, S, k, cells, canon=True, alphabet="DNA", seedseed=0, count_threshold=0, w=0):
    """makedest (src/fastxmerge.cpp:70-120) of a multiset sketch under -c: to_string(opts.ct()) is CountMinCounting whenever cells > 0
    (d2.h:207), then the cells; the suffix is this build's .d2gbmh"""
    ret = path.split(" ")[0]
    if seedseed:
        ret += f".seed{seedseed}"
    if canon:
        ret += ".rc_canon"
    ret += f".sketchsize{S}.k{k}"
    if w > k:
        ret += f".w{w}"
    if count_threshold > 0:
        ret += f".ct_threshold{int(count_threshold)}"
    return ret + f".CountMinCounting{cells}.MultisetSpace.{alphabet}.d2gbmh"


def options_tail(cells):
    """what Dashing2Options::to_string appends for -c, line feed included (d2.cpp:33)"""
    return f";counting=countsketch{cells}\n"
