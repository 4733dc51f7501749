"""NumPy / pure-Python restatement of the reference's BED sketching (bed2sketch, src/bedsketch.cpp:36-56), written from its text and
independent of libd2g: the line rules, the element ids, the One-Permutation registers one position at a time, and the --multiset
weights by a dictionary filled in line order.  Chromosome hashes come from the recorded digests in tests/golden/xxh3_names.json (the
`xxhash` module where it imports, for names the table lacks)."""
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xxh3_names.json")
OPH_XOR = 0x8f1896f3f85ef4a3 ^ 0x533f8c2151b20f97        # seed_ ^ the constant of oph.h:49 = 0xdc271ad2a9ecfb34
M64 = (1 << 64) - 1
K1_CHUNK = 64
K1_BLOCK_POSITIONS = 256 * 4 * K1_CHUNK                 # positions of one full workgroup (K1_THREADS x K1_CPT chunks)

_table = None


def golden_table():
    """{name bytes: digest}"""
    global _table
    if _table is None:
        with open(GOLDEN) as f:
            _table = {bytes.fromhex(e["hex"]): int(e["xxh3_64"]) for e in json.load(f)["entries"]}
    return _table


def chrom_hash(name: bytes) -> int:
    t = golden_table()
    if name in t:
        return t[name]
    import xxhash                                        # names outside the table need the module
    return xxhash.xxh3_64_intdigest(name)


def strtoul(s: bytes, p: int):
    """C strtoul(s + p, &end, 10) on a NUL-terminated buffer -> (value, end): white space skipped, an optional sign, digits; no digit:
    (0, p); a value beyond 2^64 - 1: 2^64 - 1; a minus sign negates modulo 2^64"""
    n, q = len(s), p
    while q < n and s[q] in b" \t\n\v\f\r":
        q += 1
    neg = False
    if q < n and s[q] in b"+-":
        neg = s[q] == ord("-")
        q += 1
    d0 = q
    v = 0
    while q < n and 48 <= s[q] <= 57:
        v = v * 10 + (s[q] - 48)
        q += 1
    if q == d0:
        return 0, p
    if v > M64:
        return M64, q
    return ((-v) & M64 if neg else v), q


def parse(buf: bytes, trim_chr=True):
    """-> [(name bytes, start, stop)] of the data lines, in order; ValueError("Malformed line: ...") for a line without a tab"""
    out = []
    lines = buf.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                      # std::getline: no line after the last line feed
    for s in lines:
        if not s or s[:1] == b"#":
            continue
        s = s.split(b"\0")[0] if b"\0" in s else s       # strchr / strtoul stop at a NUL
        t = s.find(b"\t")
        if t < 0:
            raise ValueError("Malformed line: " + s.decode(errors="replace"))
        p = 3 if trim_chr and s[:1] in (b"c", b"C") and s[1:3] == b"hr" else 0
        a, q = strtoul(s, t + 1)
        b, _ = strtoul(s, q)
        out.append((s[p:t], a, b))
    return out


def tables(files, trim_chr=True):
    """files: list of BED buffers -> (chrhash, start, stop uint64[nint], file_off uint64[n + 1])"""
    h, a, b, off = [], [], [], [0]
    for buf in files:
        for name, s, e in parse(buf, trim_chr):
            h.append(chrom_hash(name)); a.append(s); b.append(e)
        off.append(len(h))
    return np.array(h, np.uint64), np.array(a, np.uint64), np.array(b, np.uint64), np.array(off, np.uint64)


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


def all_element_ids(h, a, b):
    """the elements of every line, line after line: uint64 arrays [nint] -> uint64[sum of max(stop - start, 0)]"""
    h, a, b = (np.asarray(x, np.uint64) for x in (h, a, b))
    lens = np.where(b > a, b - a, np.uint64(0)).astype(np.int64)
    line = np.repeat(np.arange(lens.size), lens)
    first = np.cumsum(lens) - lens
    off = (np.arange(int(lens.sum()), dtype=np.int64) - first[line]).astype(np.uint64)
    with np.errstate(over="ignore"):
        return h[line] ^ (a[line] + off)


def oph_registers(lines, S):
    """lines: iterable of (chrhash, start, stop) -> registers uint64[m], m = S + (S & 1): OPSetSketch::update per position
    (oph.h:176-211): id = Wang(element ^ OPH_XOR), idx = id & (m - 1) or (uint32)id % m, register = min"""
    m = S + (S & 1)
    regs = np.full(m, M64, np.uint64)
    lines = list(lines)
    if not lines:
        return regs
    h, a, b = zip(*lines)
    ids = wang64(all_element_ids(h, a, b) ^ np.uint64(OPH_XOR))
    idx = (ids & np.uint64(m - 1)) if m & (m - 1) == 0 else ((ids & np.uint64(0xFFFFFFFF)) % np.uint64(m))
    np.minimum.at(regs, idx.astype(np.int64), ids)
    return regs


def oph_registers_files(files, S, trim_chr=True):
    h, a, b, off = tables(files, trim_chr)
    return np.stack([oph_registers(zip(h[off[f]:off[f + 1]], a[off[f]:off[f + 1]], b[off[f]:off[f + 1]]), S) for f in range(len(files))])


def multiset_weights(lines, normalize=False):
    """Counter::add(element, inc) line by line -> {(chrhash, position): weight}, keys in first-touch order.  The key is the PAIR, not
    chrhash ^ position (two chromosomes whose hashes alias under ^ i stay apart, as in the build)."""
    w = {}
    for h, a, b in lines:
        h, a, b = int(h), int(a), int(b)
        if a >= b:
            continue
        inc = 1.0 / float(b - a) if normalize else 1.0
        for i in range(a, b):
            w[(h, i)] = w.get((h, i), 0.0) + inc
    return w


def multiset_lists(lines, normalize=False):
    """-> (ids uint64[], weights float64[], total weight): the elements by (chrhash, position) ascending; the total weight is the sum,
    run by run, of weight x length over the maximal runs of consecutive positions with bit-equal weight"""
    w = multiset_weights(lines, normalize)
    keys = sorted(w)
    ids = np.array([h ^ i for h, i in keys], np.uint64)
    ws = np.array([w[k] for k in keys], np.float64)
    total, r0 = 0.0, 0
    for r in range(1, len(keys) + 1):
        if r == len(keys) or keys[r][0] != keys[r0][0] or keys[r][1] != keys[r - 1][1] + 1 or \
                struct.pack("<d", ws[r]) != struct.pack("<d", ws[r0]):
            total += float(ws[r0]) * float(r - r0)
            r0 = r
    return ids, ws, total


def closed_form_weights(lines):
    """integer-weight closed form: the weight of a position is the NUMBER of lines that cover it -> {(chrhash, position): count}"""
    w = {}
    for h, a, b in lines:
        for i in range(int(a), int(b)):
            w[(int(h), i)] = w.get((int(h), i), 0) + 1
    return w
