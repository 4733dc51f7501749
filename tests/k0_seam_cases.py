"""FASTA inputs that put every oddity of the format ON the structural seams of K0, the device parser (test infrastructure; the model
of k0_ref.py is checked on every one of them by test_k0_ref.py, the device by test_gpu_k0_stream.py).

K0's seams (d2g_k0.hip): the 16-byte chunk of a thread, the 1024-byte share of a wave, the 4096-byte tile of a workgroup, the round of
64 tiles (262144 bytes) of the two carry kernels, the 32-bit output word that neighbouring tiles -- or the last tile of one file and
the first of the next -- share, and the file table.

A SEAM EVENT is a few bytes with one decisive byte; `seam_case` places it so that the decisive byte lands at file offset P + d.  Every
event is placed at P in SEAMS with d in (-1, 0, +1), and once (d = 0) at the carry round; what needs whole tiles (a tile of line feeds,
a header of 64 tiles) is built on its own.  Every input is at most three tiles long except those that have to cross a round.

CASES is the catalogue: Case(name, group, files, genome_nfiles, refused).  No case is special to any test: the model handles all."""
from collections import namedtuple

import numpy as np

TILE = 4096
ROUND = 64 * TILE
SEAMS = (16, 1024, 4096, 8192, 3 * TILE)

Case = namedtuple("Case", "name group files genome_nfiles refused")


def seq(seed, n, lower=False):
    """n random bases"""
    s = np.random.default_rng(seed).choice(np.frombuffer(b"acgt" if lower else b"ACGT", np.uint8), n).tobytes()
    return s


def fill(seed, n, width=61):
    """exactly n bytes of sequence lines: random bases, a line feed after every `width` of them, the last two bytes always bases"""
    if n <= 0:
        assert n == 0
        return b""
    a = np.frombuffer(seq(seed, n), np.uint8).copy()
    i = np.arange(n)
    a[(i % (width + 1) == width) & (i < n - 2)] = 10
    return a.tobytes()


HEAD = b">s\n"


def seam_file(seed, P, d, ev, at, tail=None):
    """a file in which byte `at` of `ev` sits at offset P + d"""
    pre = P + d - len(HEAD) - at
    assert pre >= 0, (P, d, at)
    f = HEAD + fill(seed, pre) + ev + (fill(seed + 1, 45) + b"\n" if tail is None else tail)
    assert f[P + d] == ev[at]
    return f


# name -> (group, event bytes, index of the decisive byte, tail (None: 45 bases and a line feed), refused)
EVENTS = {
    # -- header detection across the seam: the header flag of a line travels in the scan key of the line feed before it
    "nl_gt": ("header", b"\n>hdr ACGT\nGATTACA", 1, None, False),
    "nl_at": ("header", b"\n@hdr ACGT\nGATTACA", 1, None, False),
    "hdr_span_acgt": ("header", b"\n>" + b"ACGT" * 8 + b"\nCATTAG", 10, None, False),
    "hdr_eof": ("header", b"\n>ACGTACGTAC", 6, b"", False),
    "gt_alone": ("header", b"\n>\nTTGACA", 1, None, False),
    "gt_alone_eof": ("header", b"\n>", 1, b"", False),
    "gt_midline": ("header", b"CA>GT", 2, None, False),
    "at_midline": ("header", b"CA@GT", 2, None, False),
    # -- '+' lines
    "plus_line_start": ("plus", b"\n+\nIIII", 1, None, True),
    "plus_midline": ("plus", b"CA+GT", 2, None, False),
    # -- carriage returns: byte 15 of a chunk looks ahead in memory, not in registers
    "cr_then_nl": ("cr", b"CA\r\nGT", 3, None, False),                 # '\r' at P - 1, '\n' at P
    "cr_then_base": ("cr", b"CA\rGT", 3, None, False),                 # '\r' at P - 1, a base at P: a break
    "cr_cr_nl": ("cr", b"CA\r\r\nGT", 3, None, False),                 # the first '\r' is a break, the second belongs to the line end
    "cr_eof": ("cr", b"CA\r", 2, b"", False),
    "cr_nl_eof": ("cr", b"CA\r\n", 3, b"", False),
    # -- a pending break crossing the seam
    "nonbase_then_base": ("pending", b"CAN" + b"GT", 3, None, False),  # 'N' at P - 1, base at P
    "n_nl_base": ("pending", b"CAN\nGT", 4, None, False),
    "nl_n_base": ("pending", b"CA\nNGT", 4, None, False),
    "nl_only": ("pending", b"CA\nGT", 2, None, False),                 # no break: the run goes on across the seam
    "nl_nl_nl": ("pending", b"CA\n\n\nGT", 3, None, False),
    # -- line shapes
    "one_base_lines": ("lines", b"\nA\nC\nG\nT\nA\nC\nG\nT\nA\nC", 5, None, False),
    "last_base_no_lf": ("lines", b"CAGT", 3, b"", False),              # the file ends with the base at P + d
}


def seam_cases():
    out = []
    for si, (name, (group, ev, at, tail, refused)) in enumerate(EVENTS.items()):
        for P in SEAMS:
            for d in (-1, 0, 1):
                out.append(Case(f"{name}@{P}{d:+d}", group, [seam_file(100 * si + d + 1, P, d, ev, at, tail)], None, refused))
        out.append(Case(f"{name}@{ROUND}+0", group, [seam_file(100 * si + 7, ROUND, 0, ev, at, tail)], None, refused))
    return out


def tile_cases():
    """what needs whole tiles"""
    out = []
    add = lambda name, group, *files, nf=None, refused=False: out.append(Case(name, group, list(files), nf, refused))
    LF = b"\n"
    # a header longer than two tiles (a tile that is all header: tile_total == 0) and one longer than 64 tiles, their text ACGT
    for n, nm in ((2 * TILE + 100, "2_tiles"), (ROUND + TILE + 7, "64_tiles")):
        add(f"hdr_longer_than_{nm}", "header", HEAD + fill(1, 50) + b"\n>" + b"ACGT" * (n // 4) + b"\n" + fill(2, 70) + b"\n")
        add(f"first_hdr_longer_than_{nm}", "header", b">" + b"TGCA" * (n // 4) + b"\n" + fill(3, 70))
    # tiles with no class at all inherit the carried state: a break (or none) before, then only line feeds, then a base
    for brk, nm in ((b"N", "break"), (b"", "no_break")):
        for pos in (TILE - 1, TILE, 100):                              # where the first line feed sits
            pre = HEAD + fill(4, pos - len(HEAD) - len(brk)) + brk
            add(f"{nm}_then_lf_tile@{pos}", "pending", pre + LF * (TILE + 1) + fill(5, 40) + LF)
            add(f"{nm}_then_2_lf_tiles@{pos}", "pending", pre + LF * (2 * TILE) + fill(6, 40) + LF)
        pre = HEAD + fill(7, TILE - 40) + brk
        add(f"{nm}_then_lf_round", "pending", pre + LF * (ROUND + 1) + fill(8, 40) + LF)
        add(f"{nm}_then_lf_round_and_tiles", "pending", pre + LF * (ROUND + 3 * TILE) + fill(9, 40) + LF)
    # the state set in one round and used in the next: the last class of round 0 is a break / a base
    add("break_last_in_round", "pending", HEAD + fill(10, ROUND - 4) + b"N" + fill(11, 100) + LF)
    add("base_last_in_round", "pending", HEAD + fill(12, ROUND - 3) + fill(13, 100) + LF)
    # -- word alignment of the output: c bases before the tile seam modulo 16, so that tiles share a word
    for c in (0, 1, 15, 16, 17):
        j = (TILE - len(HEAD) - c) % 16
        for junk, nm in ((b"N", "n"), (LF, "lf")):
            f = HEAD + junk * j + seq(20 + c, TILE - len(HEAD) - j) + seq(30 + c, 2 * TILE - 5) + LF
            add(f"align_c{c}_{nm}", "align", f)
    # every (offset in the word, bases in the chunk): the spill rule of the emit pass.  Chunk by chunk: a chunk of `nw` bases that
    # `o` bases (modulo 16) precede; what is not a base is a line feed (one long run) or an 'N' (a run start per chunk)
    for junk, nm in ((LF, "lf"), (b"N", "n")):
        rng = np.random.default_rng(77)
        chunks, cur = [bytearray(HEAD + b"ACGTTGCAACGTA")], 13         # the first chunk: 13 bases
        for o in range(16):
            for nw in range(1, 17):
                need = (o - cur) % 16
                for nb in ((need, nw) if need else (nw,)):
                    ch = bytearray(junk * 16)
                    for p in sorted(rng.choice(16, nb, replace=False).tolist()):
                        ch[p] = b"ACGT"[int(rng.integers(0, 4))]
                    chunks.append(ch)
                    cur = (cur + nb) % 16
        add(f"chunk_offset_x_count_{nm}", "align", b"".join(bytes(c) for c in chunks))
    # a tile that contributes fewer than 16 bases, all inside the one word it shares with BOTH neighbours (and none at all)
    t0 = HEAD + b"N" * 6 + seq(40, TILE - 9)                            # 4087 bases: 7 modulo 16
    for junk, nm in ((b"N", "n"), (LF, "lf")):
        add(f"five_bases_in_a_shared_word_{nm}", "align", t0 + junk * 2000 + b"GATTA" + junk * 2091 + seq(41, TILE) + LF)
        add(f"no_bases_between_sharers_{nm}", "align", t0 + junk * TILE + seq(42, TILE) + LF)
        add(f"nine_bases_fill_the_shared_word_{nm}", "align", t0 + junk * 4087 + b"GATTACAGA" + seq(43, TILE) + LF)
    # -- line shapes
    add("lower_case", "lines", b">l\n" + fill(50, 2 * TILE + 33).lower() + LF)
    mixed = np.frombuffer(fill(51, 2 * TILE + 34), np.uint8).copy()
    third = np.arange(mixed.size) % 3 == 0
    mixed[third & (mixed != 10)] |= 0x20                               # every third base in lower case
    add("mixed_case", "lines", b">m\n" + mixed.tobytes() + LF)
    add("unwrapped_line_longer_than_64_tiles", "lines", HEAD + seq(52, ROUND + TILE + 11) + LF)
    for n in (TILE, 2 * TILE, ROUND):
        add(f"all_bases_to_the_end_of_a_tile_{n}", "lines", HEAD + seq(53, n - len(HEAD)))
    # -- carriage return as the last byte of a file of 16 k and of 4096 k bytes
    for n in (16, 32, TILE, 2 * TILE):
        add(f"cr_last_byte_of_{n}", "cr", HEAD + fill(54, n - len(HEAD) - 1) + b"\r")
        add(f"cr_cr_last_bytes_of_{n}", "cr", HEAD + fill(55, n - len(HEAD) - 2) + b"\r\r")
    add("crlf_everywhere", "cr", HEAD.replace(LF, b"\r\n") + fill(56, 2 * TILE + 100).replace(LF, b"\r\n") + b"\r\n")
    return out


def sized_file(seed, n, lf=False):
    """a FASTA file of exactly n bytes: a three-byte header line and bases, with or without a last line feed"""
    if n < 2:
        return b">"[:n]
    assert n >= 5
    return b">f\n" + (seq(seed, n - 4) + b"\n" if lf else seq(seed, n - 3))


def file_table_cases():
    out = []
    add = lambda name, files, nf=None: out.append(Case(name, "files", list(files), nf, False))
    L = (0, 1, 15, 16, 17, 4095, 4096, 4097)
    for lf, nm in ((False, ""), (True, "_lf")):
        files = [sized_file(60 + i, n, lf) for i, n in enumerate(L)]
        add(f"sizes_one_file_per_genome{nm}", files)
        add(f"sizes_reversed{nm}", files[::-1])
        add(f"sizes_multi_file_genomes{nm}", files, [3, 1, 4])
        add(f"sizes_one_genome{nm}", files, [8])
        # base totals 12, 13, 14 and 4092 + 4093 + 4094: the next file's first word is shared
        add(f"sizes_shuffled{nm}", [files[i] for i in (5, 2, 0, 7, 4, 1, 6, 3)], [2, 2, 1, 3])
    a, b, c = sized_file(70, 4097), sized_file(71, 15), sized_file(72, 17)
    add("empty_first", [b"", a, b, c])
    add("empty_middle", [a, b"", b"", b, c], [2, 3])
    add("empty_last", [a, b, c, b""], [3, 1])
    add("empty_first_middle_last", [b"", a, b"", b, b"", c, b""], [2, 2, 3])
    add("empty_genomes_between", [a, b"", b, b"", c], [1, 1, 1, 1, 1])
    add("only_empty_files", [b"", b"", b""])
    add("only_empty_files_one_genome", [b"", b"", b""], [3])
    add("one_empty_file", [b""])
    add("no_files_in_some_genomes", [a, b], [0, 1, 0, 1, 0])
    add("only_headers", [b">", b">a\n", b">b", b">c\n>d\n"], [1, 3])
    add("one_base_files", [b">a\nA", b">b\nC\n", b">c\nG", b">d\nT\n"] * 5, [1] * 4 + [16])
    # a file that ends in a header, then one that begins with bases right after its header: nothing carries over
    add("state_does_not_cross_files", [HEAD + fill(73, 100), b">x\n" + fill(74, 100) + b"N", b">y\n" + fill(75, 40) + b"\n>tail"])
    # 17 files of 5 bases: every word of the output is shared by files, in tiles of their own
    add("many_small_files", [b">q\n" + seq(80 + i, 5) + b"\n" for i in range(17)], [17])
    add("small_between_large", [sized_file(76, 2 * TILE + 3), sized_file(77, 16), sized_file(78, TILE + 1)], [3])
    return out


CASES = seam_cases() + tile_cases() + file_table_cases()
GROUPS = ("header", "plus", "cr", "pending", "align", "lines", "files")
assert len({c.name for c in CASES}) == len(CASES) and {c.group for c in CASES} == set(GROUPS)
for _c in CASES:
    assert all(not f or f[:1] == b">" for f in _c.files), _c.name      # what does not begin with '>' never reaches the device


def by_group(group, refused=False):
    return [c for c in CASES if c.group == group and c.refused == refused]


# ---------------------------------------------------------------- reuse of one sketcher (a sequence of ingests, in order)
REUSE = (
    Case("all_T_40kb", "reuse", [HEAD + b"T" * 40_000 + b"\n"], None, False),          # every bit of 10 000 output bytes set
    Case("smaller_after_all_T", "reuse", [HEAD + fill(90, 9000) + b"\n"], None, False),
    Case("tiny_after_that", "reuse", [b">t\nACG"], None, False),
    Case("refused", "reuse", [HEAD + fill(91, 5000) + b"\n+\nIIII\n"], None, True),
    Case("after_a_refusal", "reuse", [HEAD + fill(92, 3000) + b"\n", b">u\n" + b"A" * 777], [2], False),
    Case("all_T_again", "reuse", [HEAD + b"T" * 20_000], None, False),
    Case("all_A_after_all_T", "reuse", [HEAD + b"A" * 19_999 + b"\n"], None, False),
)
