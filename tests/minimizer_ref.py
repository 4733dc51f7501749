"""The windowed-minimizer model (-w > k), in pure Python over the bases of a FASTA buffer (test infrastructure; no GPU, nothing of
the product in here; held to its own properties by test_minimizer_ref.py).

With w > k, q = w - k + 1.  A run is a maximal ACGT stretch inside one record.  Its k-mers x_0 .. x_{nk-1} (canonical when `canon`:
the smaller of the window and its reverse complement, which with A < C < G < T is the smaller 2-bit value) have nk - q + 1 window
positions; position i emits the ONE k-mer of x_i .. x_{i+q-1} with the smallest score x ^ LEX_XOR (compared as unsigned 64-bit),
once per position, duplicates included.  XOR is a bijection, so no tie-break matters.  Nothing spans runs.  w <= k: every k-mer.

`rewrite` turns an input into a FASTA with ONE RECORD OF k BASES PER EMISSION: that file holds exactly the emitted multiset (a record
of k bases has one window, records never join), so the UNCHANGED oracle -- which knows no window -- gives every expected value of a
windowed sketch bit for bit, as tests/filter_ref.py does for --filterset.

Two enumerators that share nothing but the k-mer values: a monotone deque, and a brute-force minimum per window.
"""
from collections import deque

import numpy as np

from filter_ref import records, revcomp

LEX_XOR = 0xe37e28c4271b5a2d
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}
_BASES = b"ACGT"


def runs(seq: bytes):
    """the maximal ACGT stretches of one record's sequence, in order"""
    out, cur = [], bytearray()
    for c in seq:
        if c in _CODE:
            cur.append(c)
        elif cur:
            out.append(bytes(cur)); cur = bytearray()
    if cur:
        out.append(bytes(cur))
    return out


def encode(kmer: bytes) -> int:
    v = 0
    for c in kmer:
        v = (v << 2) | _CODE[c]
    return v


def decode(v: int, k: int) -> bytes:
    return bytes(_BASES[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def run_kmers(run: bytes, k: int, canon: bool):
    """the k-mers of one run as 2-bit values (first base most significant), from the STRINGS: slice, reverse-complement, compare"""
    out = []
    for i in range(len(run) - k + 1):
        s = run[i:i + k]
        if canon:
            r = revcomp(s)
            if r < s:
                s = r
        out.append(encode(s))
    return out


def run_kmers_fast(run: bytes, k: int, canon: bool):
    """the same values by rolling arithmetic (for the long inputs of the GPU tests; test_minimizer_ref.py holds it to run_kmers)"""
    n = len(run) - k + 1
    if n <= 0:
        return []
    codes = np.frombuffer(run.translate(bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")), np.uint8).astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | codes[j:j + n]
        rc = rc | ((np.uint64(3) - codes[j:j + n]) << np.uint64(2 * j))
    return [int(x) for x in (np.minimum(fwd, rc) if canon else fwd)]


def emit_deque(vals, q: int):
    """sliding minimum by score over windows of q values: a monotone deque of (score, value)"""
    out, dq = [], deque()
    for t, v in enumerate(vals):
        s = v ^ LEX_XOR
        while dq and dq[-1][0] >= s:
            dq.pop()
        dq.append((s, t))
        if dq[0][1] <= t - q:
            dq.popleft()
        if t >= q - 1:
            out.append(dq[0][0] ^ LEX_XOR)
    return out


def emit_brute(vals, q: int):
    """the same, one min() per window"""
    return [min(vals[i:i + q], key=lambda v: v ^ LEX_XOR) for i in range(len(vals) - q + 1)]


def window_q(k: int, w: int) -> int:
    return w - k + 1 if w > k else 1


def run_emissions(run: bytes, k: int, w: int, canon: bool, brute=False, fast=False):
    vals = (run_kmers_fast if fast else run_kmers)(run, k, canon)
    q = window_q(k, w)
    if q == 1:
        return vals
    return (emit_brute if brute else emit_deque)(vals, q)


def seq_emissions(seq: bytes, k: int, w: int, canon: bool, **kw):
    out = []
    for r in runs(seq):
        out.extend(run_emissions(r, k, w, canon, **kw))
    return out


def fasta_emissions(fasta: bytes, k: int, w: int, canon: bool, **kw):
    """every emission of a FASTA buffer, in order, as 2-bit values"""
    out = []
    for _, seq in records(fasta):
        out.extend(seq_emissions(seq, k, w, canon, **kw))
    return out


def _as_fasta(vals, k):
    return b"".join(b">s\n" + decode(v, k) + b"\n" for v in vals)


def rewrite(fasta: bytes, k: int, w: int, canon: bool, keep=None) -> bytes:
    """the input as the windowed walker sees it: one k-base record per emission (`keep`: a predicate on the 2-bit value, for filters)"""
    return _as_fasta((v for v in fasta_emissions(fasta, k, w, canon, fast=True) if keep is None or keep(v)), k)


def rewrite_by_record(fasta: bytes, k: int, w: int, canon: bool):
    """--parse-by-seq: -> [(record name, rewritten buffer of that record)]"""
    return [(name, _as_fasta(seq_emissions(seq, k, w, canon, fast=True), k)) for name, seq in records(fasta)]


def wang64(x):
    """Thomas Wang's 64-bit mix over a uint64 array (the library's maskfn is wang64(kmer ^ xormask))"""
    k = np.asarray(x, np.uint64).copy()
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


def masked_counts(vals, xormask=0):
    """the emitted multiset as the exact counter reports it: (masked keys ascending uint64, counts uint32)"""
    if not len(vals):
        return np.empty(0, np.uint64), np.empty(0, np.uint32)
    keys, counts = np.unique(wang64(np.array(vals, np.uint64) ^ np.uint64(xormask)), return_counts=True)
    return keys, counts.astype(np.uint32)
