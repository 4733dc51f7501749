"""Inputs for the device-resident sketch entry points (d2g_oph_plan_create + d2g_oph_sketch_dev / d2g_oph_count_dev /
d2g_bmh_sketch_dev), in the layout the benchmark gives them, with what they must return (test infrastructure for
test_gpu_sketch_dev.py; held to its stated properties, without a GPU, by test_sketch_dev_cases.py).  No GPU and no library call
in here.

The layout is one that the host parser never produces: genome g is one run of lens[g] bases that starts at base g * slot_bytes * 4
of a buffer whose EVERY byte is random -- inside the runs, between them and in the 64 bytes behind the last slot.  The bases of a
run are whatever the random bytes decode to (base p = bits [2 (p % 4), +2) of byte p / 4; 0 1 2 3 = A C G T).  The variants read
the same bytes through other tables: unaligned starts, two runs per genome, overlapping genomes, a genome without a run, runs in
descending stream order.

Expected values never come from the library:
    keys and counts      the distinct wang64(kmer ^ xormask) of a genome's runs and how often each occurs.  The k-mers are rolled
                         in NumPy uint64 (`kmers_np`: the pure-Python enumerator of k3_seam_cases takes seconds for the 131 k-mer
                         runs); test_sketch_dev_cases.py holds the result to k3_seam_cases.key_counts over the runs as ACGT strings
    registers, counts    oph_kmers_ref.closed_form over those keys (what oph_kmers_ref.genome_closed_form computes from records)
    BagMinHash           oracle.bmh_from_weighted(keys, float64(counts), S), the sequential heap algorithm, over the elements with
                         float64(count) > threshold

No table in here lets a kernel read outside its buffer: every run ends at least 64 bytes before the end (Layout.check_bounds)."""
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import k0_ref
import k3_seam_cases as C
import oph_kmers_ref as R

PAD = 64                                                               # readable bytes the kernels want behind the last base
SEEDED = 0x9E3779B97F4A7C15                                            # a "seeded" xormask: any non-zero value is one
CHUNK = 64                                                             # K1_CHUNK: k-mers per lane chunk
WG_KMERS = 1024 * CHUNK                                                # K1_BLOCK_CHUNKS chunks: one workgroup's share
SEAM_KMERS = (1, 63, 64, 65, WG_KMERS, WG_KMERS + 1, 2 * WG_KMERS + 1)  # one chunk .. two workgroups and one k-mer in a third
SEAM_SIZES = (1000, 1024, 16384, 16385, 20000)                         # 8 m bytes: LDS up to m = 16 384, HBM from m = 16 386
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _oracle():
    from oracle import oracle as O
    O.load()
    return O


def decode(packed):
    """the base codes of a whole packed buffer: 4 per byte, low bits first"""
    return ((packed[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & np.uint8(3)).reshape(-1)


def slots(seed, lens, slot_bytes):
    """-> ((packed uint8, run_start uint64, run_len uint32, genome_run_off uint64), base codes of every run)"""
    n = len(lens)
    packed = np.random.default_rng(seed).integers(0, 256, n * slot_bytes + PAD, dtype=np.uint8)
    run_start = np.arange(n, dtype=np.uint64) * np.uint64(slot_bytes * 4)
    run_len = np.array(lens, np.uint32)
    codes = decode(packed)
    return ((packed, run_start, run_len, np.arange(n + 1, dtype=np.uint64)),
            [codes[int(s):int(s) + int(l)] for s, l in zip(run_start, run_len)])


def slot_bytes_for(maxlen):
    """the benchmark's slot: the bytes of the longest run, rounded up to 64"""
    return ((maxlen + 3) // 4 + 63) // 64 * 64


def kmers_np(codes, k, canon):
    """the k-mers of one run of base codes: forward value (first base most significant) or the smaller of it and its reverse
    complement, all windows at once"""
    n = codes.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    c = codes.astype(np.uint64)
    fwd, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]                       # k = 32: the first base's bits end at the top, nothing is lost
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return np.minimum(fwd, rc) if canon else fwd


class Layout:
    """one packed buffer with one set of run tables over it, and what its genomes must give"""

    def __init__(self, name, packed, run_start, run_len, genome_run_off, slot_bytes):
        self.name, self.slot_bytes = name, slot_bytes
        self.packed = np.ascontiguousarray(packed, np.uint8)
        self.run_start = np.ascontiguousarray(run_start, np.uint64)
        self.run_len = np.ascontiguousarray(run_len, np.uint32)
        self.genome_run_off = np.ascontiguousarray(genome_run_off, np.uint64)
        for a in (self.packed, self.run_start, self.run_len, self.genome_run_off):
            a.setflags(write=False)
        self.n, self.nrun = self.genome_run_off.size - 1, self.run_start.size
        self._codes = decode(self.packed)
        self._kc, self._oph, self._bmh = {}, {}, {}
        self.check_bounds()

    def __repr__(self):
        return self.name

    def check_bounds(self):
        """every run inside the buffer with PAD readable bytes behind its last base"""
        assert int(self.genome_run_off[0]) == 0 and int(self.genome_run_off[-1]) == self.nrun
        assert (np.diff(self.genome_run_off.astype(np.int64)) >= 0).all()
        if self.nrun:
            end = int((self.run_start.astype(np.int64) + self.run_len.astype(np.int64)).max())
            assert (end + 3) // 4 + PAD <= self.packed.size, self.name

    def tables(self):
        return self.run_start, self.run_len, self.genome_run_off

    def runs_of(self, g):
        return range(int(self.genome_run_off[g]), int(self.genome_run_off[g + 1]))

    def run_codes(self, r):
        s = int(self.run_start[r])
        return self._codes[s:s + int(self.run_len[r])]

    def records(self, g):
        """genome g as plain ACGT records, one per run, in table order"""
        return [_ACGT[self.run_codes(r)].tobytes().decode() for r in self.runs_of(g)]

    def fasta(self, g):
        return C.fasta(self.records(g), f"{self.name}{g}")

    def nkmers(self, k):
        return [sum(max(0, int(self.run_len[r]) - k + 1) for r in self.runs_of(g)) for g in range(self.n)]

    def key_counts(self, k, canon, xormask):
        """per genome (keys uint64 sorted, counts uint32, number of k-mers)"""
        at = (k, bool(canon), xormask)
        if at not in self._kc:
            out = []
            for g in range(self.n):
                kmers = np.concatenate([kmers_np(self.run_codes(r), k, canon) for r in self.runs_of(g)] + [np.zeros(0, np.uint64)])
                keys, counts = np.unique(k0_ref.wang64(kmers ^ np.uint64(xormask)), return_counts=True)
                out.append((keys, counts.astype(np.uint32), int(kmers.size)))
            self._kc[at] = out
        return self._kc[at]

    def oph(self, k, canon, xormask, S):
        """-> (registers uint64 [n][m], counts uint32 [n][m]), read-only"""
        at = (k, bool(canon), xormask, S)
        if at not in self._oph:
            m = R.oph_m(S)
            regs, cnts = np.empty((self.n, m), np.uint64), np.empty((self.n, m), np.uint32)
            for g, (keys, counts, _) in enumerate(self.key_counts(k, canon, xormask)):
                regs[g], cnts[g] = R.closed_form(keys, counts, m)
            regs.setflags(write=False)
            cnts.setflags(write=False)
            self._oph[at] = regs, cnts
        return self._oph[at]

    def bmh(self, k, canon, xormask, S, thr):
        """-> (registers float64 [n][S], total weights float64 [n]) of the elements with float64(count) > thr, read-only"""
        at = (k, bool(canon), xormask, S, thr)
        if at not in self._bmh:
            O = _oracle()
            sig, tw = np.empty((self.n, S), np.float64), np.empty(self.n, np.float64)

            def one(kc):
                keys, counts, _ = kc
                keep = counts.astype(np.float64) > thr
                s, t = O.bmh_from_weighted(keys[keep], counts[keep].astype(np.float64), S)
                assert t == float(counts[keep].astype(np.uint64).sum())
                return s, t
            # the heap algorithm takes a third of a second per genome at S = 2048, whatever the genome's length; each call owns its
            # state and ctypes releases the interpreter lock, so the genomes go through it side by side
            with ThreadPoolExecutor(max(1, min(self.n, 8))) as pool:
                for g, (s, t) in enumerate(pool.map(one, self.key_counts(k, canon, xormask))):
                    sig[g], tw[g] = s, t
            sig.setflags(write=False)
            tw.setflags(write=False)
            self._bmh[at] = sig, tw
        return self._bmh[at]

    def head(self, nb, b0=0):
        """the tables of the first nb one-run genomes: what a plan over nb slots holds.  The same plan applied at the base pointer
        packed + b0 * slot_bytes reads genomes b0 .. b0 + nb - 1 of this layout (checked here to stay inside the buffer)"""
        assert self.nrun == self.n and b0 + nb <= self.n
        assert self.run_start.tolist() == [g * self.slot_bytes * 4 for g in range(self.n)]
        end = int((self.run_start[:nb].astype(np.int64) + self.run_len[:nb].astype(np.int64)).max())
        assert b0 * self.slot_bytes + (end + 3) // 4 + PAD <= self.packed.size
        return self.run_start[:nb], self.run_len[:nb], np.arange(nb + 1, dtype=np.uint64)

    def gaps(self):
        """the byte ranges [lo, hi) that no run touches, the tail behind the last run included"""
        used = np.zeros(self.packed.size + 1, np.int64)
        for r in range(self.nrun):
            s, e = int(self.run_start[r]), int(self.run_start[r]) + int(self.run_len[r])
            used[s // 4] += 1
            used[(e + 3) // 4] -= 1
        free = np.cumsum(used)[:-1] == 0
        edges = np.flatnonzero(np.diff(np.concatenate([[0], free.astype(np.int8), [0]])))
        return list(zip(edges[::2].tolist(), edges[1::2].tolist()))


def bench_layout(name, seed, lens):
    slot = slot_bytes_for(max(lens))
    (packed, rs, rl, go), _ = slots(seed, lens, slot)
    return Layout(name, packed, rs, rl, go, slot)


# ---------------------------------------------------------------- a. the plan's seams
@functools.lru_cache(maxsize=None)
def seams(k, seed=3100):
    """seven genomes of 1, 63, 64, 65 (around one lane chunk), 65 536, 65 537 (one workgroup's share and one k-mer more) and
    131 073 k-mers (two workgroups and a third for the last k-mer: three that merge in HBM).  seed + 1: the same tables over
    other bytes (input B of the stream-order tests)"""
    return bench_layout(f"seams_k{k}_{seed}", seed + 7 * k, [nk + k - 1 for nk in SEAM_KMERS])


# ---------------------------------------------------------------- the variants: other tables over the same bytes
VARIANTS = ("unaligned", "two_runs", "overlap", "no_run", "descending")


@functools.lru_cache(maxsize=None)
def variant(which, k, seed=3200):
    """four slots of 20 480 bytes (81 920 bases) of random bytes, read through
        unaligned    one run per genome that starts 1, 5, 18 and 63 bases into its slot: none at a multiple of 4, let alone of 16
        two_runs     two runs per genome with a gap between them; genome 0's are 40 000 and 41 000 bases long, so that its first
                     workgroup ends inside the second run and a second one takes the rest
        overlap      genome 1 begins inside genome 0's run and genome 2 is a part of genome 1: the same bases in two genomes.
                     Genome 3 is two runs that overlap EACH OTHER by 3000 bases: k-mers of count 2, the only ones a count
                     threshold of 1 keeps
        no_run       genomes 1 and 3 have no run (genome_run_off repeats), the last genome among them
        descending   the runs of `two_runs`, listed from the end of the stream to its start"""
    slot = 20480
    packed = slots(seed, [k] * 4, slot)[0][0]
    base = [g * slot * 4 for g in range(4)]
    if which == "unaligned":
        rs = [base[0] + 1, base[1] + 5, base[2] + 18, base[3] + 63]
        rl = [5000, 4097, 64 + k - 1, 70001]
        go = [0, 1, 2, 3, 4]
    elif which in ("two_runs", "descending"):
        rs = [base[0] + 3, base[0] + 40003 + 777, base[1] + 16, base[1] + 16 + 2000 + 1, base[2], base[2] + 9000, base[3] + 7, base[3] + 30000]
        rl = [40000, 41000, 2000, 3000, k, 4000, 5000, k + 63]
        go = [0, 2, 4, 6, 8]
        if which == "descending":
            rs, rl = rs[::-1], rl[::-1]
    elif which == "overlap":
        rs = [base[0] + 2, base[0] + 6002, base[0] + 8001, base[2] + 9, base[2] + 9 + 5000]
        rl = [10000, 12000, 3000, 8000, 6000]
        go = [0, 1, 2, 3, 5]
    elif which == "no_run":
        rs = [base[0] + 11, base[2] + 4]
        rl = [6000, 7000]
        go = [0, 1, 1, 2, 2]
    else:
        raise KeyError(which)
    return Layout(f"{which}_k{k}", packed, rs, rl, go, slot)


# ---------------------------------------------------------------- b. one plan over several buffers and base pointers
REUSE_LEN = 9000


@functools.lru_cache(maxsize=None)
def reuse_buffer(i):
    """buffer i of three with the same tables: 6 slots of one 9000-base run each (a plan over 3 of them fits at slots 0 and 3)"""
    return bench_layout(f"reuse{i}", 3300 + i, [REUSE_LEN] * 6)


# ---------------------------------------------------------------- d. K3 in the benchmark's layout
K3_K = 21


@functools.lru_cache(maxsize=None)
def multiset_slots(seed=3400):
    """5 slots of one 8000-base run: two batches of 4 genomes through one plan, the second at packed + slot_bytes (five genomes,
    because the oracle's heap algorithm takes a third of a second per genome at S = 2048, whatever the genome's length).  Random
    bases at k = 21 hold no k-mer twice -- but for a 22-base reverse palindrome in genome 4 (a 21-mer and, one base on, its reverse
    complement: one canonical element of count 2) -- so a count threshold of 1 leaves that element in genome 4 and nothing
    elsewhere: +inf registers and weight 0 (the variant `overlap` is the input in which it leaves thousands)"""
    return bench_layout(f"multiset{seed}", seed, [8000] * 5)


@functools.lru_cache(maxsize=None)
def k3_reuse_step(step):
    """the batches that share one context's K3 work state, in the order of the test: 6 x 40 kbp; 2 genomes of which the second has
    no run; 3 x 10 kbp"""
    if step == 0:
        return bench_layout("k3_six", 3500, [40000] * 6)
    if step == 1:
        lay = bench_layout("k3_pair", 3501, [7000, 7000])
        return Layout("k3_one_and_none", lay.packed, lay.run_start[:1], lay.run_len[:1], [0, 1, 1], lay.slot_bytes)
    return bench_layout("k3_three", 3502, [10000] * 3)


# ---------------------------------------------------------------- e. the sub-batch pipeline
def light_min_kmers(S, n=3):
    """the smallest number of k-mers per genome at which a batch of n equal genomes takes the light first pass, and with it the
    sub-batch pipeline.  K3Run::sketch keeps the light form unless sum_g gk min(1, guess_g) > total / 8, with guess = bmh_guess(gk, S)
    = 1.25 (S / gk) (ln S + 8.58).  For equal genomes n cancels: min(1, guess) <= 1/8  <=>  gk >= 10 S (ln S + 8.58).
    S = 64: 640 * 12.73888... = 8152.9, so 8153 k-mers, 8173 bases at k = 21 (8 buckets of ~1019 keys: not split)"""
    gk = math.ceil(10.0 * S * (math.log(float(S)) + 8.58))
    assert C.predicted_light([gk] * n, S) and not C.predicted_light([gk - 1] * n, S)
    return gk


@functools.lru_cache(maxsize=None)
def pipeline_batch(light, seed=3600):
    """three genomes of light_min_kmers(64) k-mers (light = True: the pipelined form runs) or one k-mer fewer (the batch stays
    heavy and is bucketed in one range).  seed + 1: input B"""
    gk = light_min_kmers(64) - (0 if light else 1)
    return bench_layout(f"pipeline_{'light' if light else 'heavy'}_{seed}", seed, [gk + K3_K - 1] * 3)


# ---------------------------------------------------------------- f. empty shapes
@functools.lru_cache(maxsize=None)
def nothing(n):
    """n genomes without a run over 64 random bytes"""
    packed = np.random.default_rng(3700).integers(0, 256, PAD, dtype=np.uint8)
    return Layout(f"nothing{n}", packed, [], [], [0] * (n + 1), 64)
