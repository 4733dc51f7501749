"""A plain model of K0, the device FASTA parser (test infrastructure; pinned against the host packer and the oracle by
test_k0_ref.py, used as the reference by test_gpu_k0_stream.py).

It restates the header comment of d2g_k0.hip as a byte-wise state machine: one byte at a time, three booleans of state, no NumPy in
the walk.  Per file:

    * a line whose first byte is '>' or '@' is a header; every byte of a header sets "break pending";
    * a line whose first byte is '+' makes the input refused (FASTQ quality sections are skipped by length: not K0's business);
    * on every other line 'ACGTacgt' are bases: a base appends its code (A0 C1 G2 T3) to the stream and, if a break is pending or
      it is the file's first base, records its stream index as a run start;
    * a line feed is neutral; ONE carriage return right before a line feed, or as the last byte of the file, is neutral;
    * every other byte sets "break pending";
    * a file that is not empty and does not begin with '>' is refused (the ingest checks this on the host before the upload).

Across files: the files of a batch concatenate; the first base of a file always starts a run; runs shorter than k stay in the
stream as dead bases.  The run table for a given k is the starts whose distance to the next start (or to the end of their file) is
at least k, split at `max_run` as d2g_seqpack::close_run_raw does; a genome owns the runs of its files.

The readback that test_gpu_k0_stream.py uses is restated here too (`window_starts`, `window_hashes`): K1 over one-k-mer genomes
returns wang64(wang64(x) ^ d2g_oph_xor_const()) of every window x, and Wang's mix is a bijection."""
import numpy as np

CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3}
LETTERS = np.frombuffer(b"ACGT", np.uint8)
MAX_RUN = 1 << 30                                                     # D2G_MAX_RUN's default


def parse_file(data):
    """-> (codes: list of 0..3, starts: list of indices into codes, refused: bool)"""
    codes, starts = [], []
    n = len(data)
    refused = n > 0 and data[0] != 0x3E
    line_start, header, pending = True, False, True                   # the first base of a file starts a run
    for i in range(n):
        ch = data[i]
        if line_start:
            header = ch == 0x3E or ch == 0x40                         # '>' '@'
            if ch == 0x2B:                                            # '+'
                refused = True
            line_start = False
        if ch == 0x0A:
            line_start = True
            if header:
                pending = True
            continue
        if header:
            pending = True
            continue
        c = CODE.get(ch)
        if c is not None:
            if pending:
                starts.append(len(codes))
                pending = False
            codes.append(c)
        elif ch == 0x0D and (i + 1 == n or data[i + 1] == 0x0A):
            pass
        else:
            pending = True
    return codes, starts, refused


class Parsed:
    """the k-independent part of a batch: the stream, every run start, the files' extents"""

    def __init__(self, files, genome_nfiles=None):
        self.genome_nfiles = [1] * len(files) if genome_nfiles is None else [int(x) for x in genome_nfiles]
        assert sum(self.genome_nfiles) == len(files)
        codes, self.file_base, self.file_starts, self.refused = [], [0], [], False
        for f in files:
            c, s, r = parse_file(bytes(f))
            self.file_starts.append([len(codes) + x for x in s])
            codes.extend(c)
            self.file_base.append(len(codes))
            self.refused |= r
        self.codes = np.array(codes, np.uint8)
        self.nbases = len(codes)

    def file_runs(self, fi, k, max_run=MAX_RUN):
        """-> (list of (start, len) of file fi's live runs, already split; its k-mer count)"""
        st = self.file_starts[fi] + [self.file_base[fi + 1]]
        runs, nk = [], 0
        for a, b in zip(st[:-1], st[1:]):
            n = b - a
            if n < k:
                continue
            nk += n - k + 1
            while n > max_run:
                runs.append((a, max_run))
                a += max_run - (k - 1)
                n -= max_run - (k - 1)
            runs.append((a, n))
        return runs, nk

    def run_table(self, k, max_run=MAX_RUN):
        """-> (run_start u64, run_len u32, genome_run_off u64, genome_nkmers u64)"""
        rs, rl, go, gnk = [], [], [0], []
        fi = 0
        for nf in self.genome_nfiles:
            nk = 0
            for _ in range(nf):
                runs, n = self.file_runs(fi, k, max_run)
                rs += [r[0] for r in runs]
                rl += [r[1] for r in runs]
                nk += n
                fi += 1
            go.append(len(rs))
            gnk.append(nk)
        return np.array(rs, np.uint64), np.array(rl, np.uint32), np.array(go, np.uint64), np.array(gnk, np.uint64)

    def run_strings(self, fi, k):
        """the live runs of file fi as upper-case bytes (what tests/test_host.py's _decode_runs returns for the host packer)"""
        return [LETTERS[self.codes[a:a + n]].tobytes() for a, n in self.file_runs(fi, k)[0]]

    def bases(self, a, n):
        return LETTERS[self.codes[a:a + n]].tobytes().decode()


# ---------------------------------------------------------------- the readback: one k-mer per window
def wang64(x):
    """Thomas Wang's 64-bit mix on a uint64 array (wraps modulo 2^64)"""
    k = np.array(x, np.uint64, copy=True)
    u = np.uint64
    with np.errstate(over="ignore"):
        k = ~k + (k << u(21))
        k ^= k >> u(24)
        k = k + (k << u(3)) + (k << u(8))
        k ^= k >> u(14)
        k = k + (k << u(2)) + (k << u(4))
        k ^= k >> u(28)
        k += k << u(31)
    return k


def window_starts(nbases, step=32):
    """-> (starts int64, W): windows of W = min(32, nbases) bases at 0, step, 2 step, ... and a last one ending at nbases (no
    window may end past the stream)"""
    W = min(32, nbases)
    if W == 0:
        return np.zeros(0, np.int64), 0
    s = list(range(0, nbases - W + 1, step))
    if s[-1] != nbases - W:
        s.append(nbases - W)
    return np.array(s, np.int64), W


def window_values(codes, starts, W):
    """the W bases from each start as one integer, the first base most significant (the forward k-mer of K1, k = W)"""
    idx = np.asarray(starts, np.int64)[:, None] + np.arange(W)[None, :]
    sh = (2 * (W - 1 - np.arange(W))).astype(np.uint64)
    return np.bitwise_or.reduce(np.asarray(codes, np.uint8)[idx].astype(np.uint64) << sh[None, :], axis=1)


def window_hashes(codes, starts, W, oph_xor_const):
    """what K1 leaves in the smaller of the S = 2 registers of a genome whose only k-mer is the window (canon off, xormask 0)"""
    return wang64(wang64(window_values(codes, starts, W)) ^ np.uint64(oph_xor_const))


def window_table(starts, W):
    """the run table of the readback: one genome per window, one run (start, W) each"""
    n = len(starts)
    return np.asarray(starts, np.uint64), np.full(n, W, np.uint32), np.arange(n + 1, dtype=np.uint64)


def pack_codes(codes):
    """2-bit codes -> the host packer's byte stream (base p at bits [2 (p % 4), +2) of byte p / 4) with the 64-byte tail pad"""
    c = np.asarray(codes, np.uint8)
    n = c.size
    q = np.zeros((n + 3) // 4 * 4, np.uint8)
    q[:n] = c
    q = q.reshape(-1, 4)
    out = np.zeros(q.shape[0] + 64, np.uint8)
    out[:q.shape[0]] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
    return out
