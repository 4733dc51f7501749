"""The --filterset model, in pure Python and on STRINGS (no 2-bit arithmetic, no hashing).

A k-mer window of an input survives iff its (canonical, when `canon`) string is not among the (canonical) k-mer strings of the
filter.  The survivors are written as a FASTA with ONE RECORD PER SURVIVING OCCURRENCE, each exactly k bases: that file holds
exactly the surviving multiset of k-mers (a record of k bases has one window, records never join), so the UNCHANGED oracle gives
every expected value of a filtered sketch bit for bit -- registers, their counts, k-mer counts, BagMinHash registers, total weights.

Windows follow the sketch inputs' rules: FASTA records ('>' header lines), runs end at every byte that is not one of ACGT and at
record ends.  Canonical = the smaller of the window and its reverse complement as strings; with A < C < G < T and the first base
most significant that is the smaller 2-bit value, which is what the device compares.
"""
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def records(fasta: bytes):
    """-> [(name, sequence bytes)] of a FASTA buffer (sequence lines joined; bytes in front of the first header are ignored)"""
    out = []
    for chunk in fasta.split(b">")[1:]:
        head, _, body = chunk.partition(b"\n")
        out.append((head.split()[0].decode() if head.split() else "", body.replace(b"\n", b"").replace(b"\r", b"")))
    return out


def windows(seq: bytes, k: int, canon: bool):
    """every k-mer window of one sequence, in order, as (canonical) strings; windows that hold a non-ACGT byte do not exist"""
    out = []
    bad = -1                                    # index of the last non-ACGT byte seen
    for i, c in enumerate(seq):
        if c not in _CODE:
            bad = i
        if i >= k - 1 and i - bad >= k:
            w = seq[i - k + 1:i + 1]
            if canon:
                r = revcomp(w)
                if r < w:
                    w = r
            out.append(w)
    return out


def fasta_windows(fasta: bytes, k: int, canon: bool):
    out = []
    for _, seq in records(fasta):
        out.extend(windows(seq, k, canon))
    return out


def filter_set(filter_fastas, k: int, canon: bool):
    """the set of (canonical) k-mer strings of the filter input(s), and the number of OCCURRENCES that went in"""
    s, n = set(), 0
    for f in filter_fastas:
        w = fasta_windows(f, k, canon)
        n += len(w)
        s.update(w)
    return s, n


def _as_fasta(ws):
    return b"".join(b">s\n" + w + b"\n" for w in ws)


def rewrite(fasta: bytes, fset, k: int, canon: bool) -> bytes:
    """the input with the filter applied: one k-base record per surviving window occurrence"""
    return _as_fasta(w for w in fasta_windows(fasta, k, canon) if w not in fset)


def rewrite_by_record(fasta: bytes, fset, k: int, canon: bool):
    """--parse-by-seq: -> [(record name, rewritten buffer of that record)]"""
    return [(name, _as_fasta(w for w in windows(seq, k, canon) if w not in fset)) for name, seq in records(fasta)]


def encode(kmer: bytes) -> int:
    """the 2-bit value of a k-mer string: A0 C1 G2 T3, first base most significant"""
    v = 0
    for c in kmer:
        v = (v << 2) | _CODE[c]
    return v
