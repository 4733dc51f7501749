"""d2g_edit_ut_dev / d2g_edit_rect_dev (edit_pair_kernel, K2h) against edit_ref's row-by-row dynamic programme and against pairs whose
distance is known by construction.  Everything is compared as exact integers.

The kernel's seams (d2g_edit.hip): a query's rows in blocks of 32, a block per lane; a pair on P = the power of two >= its block count
lanes, 64 / P pairs per wave; rows in three launch classes (<= 8 blocks, one strip, several strips); strips of at most 64 blocks (fewer
where sigma is large; D2G_EDIT_STRIP forces fewer) with the deltas between strips in two LDS planes; tiles of column records taken in
order of length (D2G_EDIT_TILE forces their size); the target read 16 symbols per load.  Outputs lie between guard words pre-filled
with 0xAB."""
import functools

import numpy as np
import pytest

import edit_ref as E

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xAB
SEAMS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 2100]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Out:
    def __init__(self, torch, n):
        self.n = n
        self.t = torch.full(((2 * GUARD + n) * 4,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * 4

    def read(self):
        a, fill = self.t.cpu().numpy().view(np.uint32), np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))
        assert (a[:GUARD] == fill).all() and (a[GUARD + self.n:] == fill).all(), "guard words around the output were written"
        return a[GUARD:GUARD + self.n].astype(np.int64)


def ut_of(gpu_ctx, torch, ss, r0=0, r1=None):
    r1 = ss.N if r1 is None else r1
    out = Out(torch, sum(ss.N - 1 - i for i in range(r0, r1)))
    ss.edit_ut_dev(r0, r1, out.ptr)
    gpu_ctx.sync()
    return out.read()


def rect_of(gpu_ctx, torch, ss, a0, a1, b0, b1):
    out = Out(torch, (a1 - a0) * (b1 - b0))
    ss.edit_rect_dev(a0, a1, b0, b1, out.ptr)
    gpu_ctx.sync()
    return out.read().reshape(a1 - a0, b1 - b0)


def related(rng, base, n, alphabet):
    """a record of n symbols: a prefix of `base` with a few substitutions, deletions and insertions, so that distances are not trivial"""
    x = list(base[:n])
    for _ in range(max(1, n // 20)):
        x[int(rng.integers(len(x)))] = int(rng.choice(alphabet))
    for _ in range(n // 50):
        del x[int(rng.integers(len(x)))]
    while len(x) < n:
        x.insert(int(rng.integers(len(x) + 1)), int(rng.choice(alphabet)))
    return bytes(x)


@functools.lru_cache(maxsize=None)
def seam_set():
    """the seam lengths and 25 ragged ones in 1 .. 300, in shuffled order: every lane-group width 1 .. 64 and the two-strip route occur,
    and waves hold mixed lengths.  -> (records, their distance matrix by the dynamic programme)"""
    rng = np.random.default_rng(7100)
    alphabet = np.frombuffer(b"ACGT", np.uint8)
    base = bytes(rng.choice(alphabet, 2100).tolist())
    lens = SEAMS + [int(v) for v in rng.integers(1, 301, 25)]
    recs = [related(rng, base, n, alphabet) if i % 3 else bytes(rng.choice(alphabet, n).tolist()) for i, n in enumerate(lens)]
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    assert sorted(len(r) for r in recs) == sorted(lens)
    return recs, E.edit_matrix(recs)


def test_seam_lengths_triangle_and_square(gpu_ctx, torch):
    recs, want = seam_set()
    ss = gpu_ctx.seqset(recs)
    try:
        assert ss.N == len(recs) and ss.alphabet_size == 4 and ss.strip_blocks == 64
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss), E.triangle(want), err_msg="upper triangle")
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, 0, ss.N, 0, ss.N), want, err_msg="square")
        np.testing.assert_array_equal(ss.edit_ut(), E.triangle(want), err_msg="host-pointer triangle")
        np.testing.assert_array_equal(ss.edit_rect(3, 9, 0, ss.N), want[3:9], err_msg="host-pointer block")
    finally:
        ss.close()


def test_an_empty_record_yields_the_other_length(gpu_ctx, torch):
    recs, want = seam_set()
    recs = recs[:5] + [b""] + recs[5:]
    lens = np.array([len(r) for r in recs], np.int64)
    w = np.insert(np.insert(want, 5, 0, axis=0), 5, 0, axis=1)
    w[5, :] = lens
    w[:, 5] = lens
    ss = gpu_ctx.seqset(recs)
    try:
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss), E.triangle(w))
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, 4, 7, 0, ss.N), w[4:7])
    finally:
        ss.close()


def test_row_ranges_blocks_and_empty_ranges(gpu_ctx, torch):
    recs, want = seam_set()
    n = len(recs)
    ss = gpu_ctx.seqset(recs)
    try:
        for r0, r1 in [(0, n // 2), (n // 2, n - 1), (n - 1, n), (0, 1), (7, 8)]:
            np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss, r0, r1), E.triangle(want, r0, r1), err_msg=f"rows [{r0}, {r1})")
        for r in (0, n // 2, n):
            assert ut_of(gpu_ctx, torch, ss, r, r).size == 0                          # an empty range: D2G_OK, nothing written
        ss.edit_ut_dev(3, 3, None)
        ss.edit_rect_dev(2, 2, 0, n, None)
        ss.edit_rect_dev(0, n, 5, 5, None)
        for a0, a1, b0, b1 in [(3, 17, 10, n), (0, 1, 0, 1), (n - 1, n, 0, n), (5, 30, 6, 7)]:
            np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, a0, a1, b0, b1), want[a0:a1, b0:b1], err_msg=f"block {a0, a1, b0, b1}")
    finally:
        ss.close()


def test_symmetry_of_a_ragged_set(gpu_ctx, torch):
    recs, want = seam_set()
    n = len(recs)
    ss = gpu_ctx.seqset(recs)
    try:
        sq = rect_of(gpu_ctx, torch, ss, 0, n, 0, n)
        np.testing.assert_array_equal(sq, sq.T)
        assert (np.diag(sq) == 0).all()
        np.testing.assert_array_equal(E.triangle(sq), ut_of(gpu_ctx, torch, ss))
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, 20, n, 0, 20), sq[:20, 20:].T)
    finally:
        ss.close()


@pytest.mark.parametrize("strip", [1, 2, 5])
def test_forced_strips(gpu_ctx, torch, monkeypatch, strip):
    """D2G_EDIT_STRIP: the several-strip route -- the planes in LDS, written by the strip's last lane and read by lane 0 of the next --
    on every record of more than `strip` blocks; with 1 the reader and the writer are the same lane"""
    recs, want = seam_set()
    keep = [i for i, r in enumerate(recs) if len(r) <= (300 if strip == 1 else 2100)]
    monkeypatch.setenv("D2G_EDIT_STRIP", str(strip))
    ss = gpu_ctx.seqset([recs[i] for i in keep])
    try:
        assert ss.strip_blocks == strip
        w = want[np.ix_(keep, keep)]
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss), E.triangle(w))
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, 0, ss.N, 0, ss.N), w)
    finally:
        ss.close()


@pytest.mark.parametrize("tile", [1, 3, 64])
def test_forced_tiles(gpu_ctx, torch, monkeypatch, tile):
    """D2G_EDIT_TILE: several workgroups per row, a last tile that is not full, tiles without a pair of the launch"""
    recs, want = seam_set()
    monkeypatch.setenv("D2G_EDIT_TILE", str(tile))
    ss = gpu_ctx.seqset(recs)
    try:
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss, 4, 31), E.triangle(want, 4, 31))
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, 2, 40, 1, 33), want[2:40, 1:33])
    finally:
        ss.close()


# ---------------------------------------------------------------- alphabets
def alphabet_set(sigma, seed):
    rng = np.random.default_rng(seed)
    if sigma == 256:
        alphabet = np.arange(256, dtype=np.uint8)
    else:
        alphabet = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY"[:sigma], np.uint8)
    lens = [1, 2, 33, 64, 65, 100, 150, 199, 200, 257] + ([1500, 2040, 2100] if sigma == 256 else [])
    base = bytes(rng.choice(alphabet, 2100).tolist())
    recs = [related(rng, base, n, alphabet) if i % 2 else bytes(rng.choice(alphabet, n).tolist()) for i, n in enumerate(lens)]
    if sigma == 256:
        recs[5] = bytes(range(256))[::-1][:100]                                       # bytes 255 ... 156
        recs[6] = bytes(range(150))                                                   # bytes 0 ... 149
        recs[9] = bytes(range(256)) + b"\x00"
    return recs


@pytest.mark.parametrize("sigma", [1, 2, 4, 5, 20, 256])
def test_alphabets(gpu_ctx, torch, sigma):
    recs = alphabet_set(sigma, 7200 + sigma)
    want = E.edit_matrix(recs)
    if sigma == 1:
        lens = np.array([len(r) for r in recs])
        np.testing.assert_array_equal(want, np.abs(lens[:, None] - lens[None, :]))   # a^m against a^n
    ss = gpu_ctx.seqset(recs)
    try:
        assert ss.alphabet_size == sigma
        # sigma = 256 with records of 64 and 66 blocks: the table of 64 blocks alone would fill LDS, so a strip holds 63 and both take the
        # several-strip route without any switch; the record of 47 blocks takes 64 lanes and a table of exactly 64 KiB
        assert ss.strip_blocks == (63 if sigma == 256 else 64)
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss), E.triangle(want))
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ss, 0, ss.N, 0, ss.N), want)
    finally:
        ss.close()


def test_upper_and_lower_case_differ(gpu_ctx, torch):
    recs = [b"ACGT", b"acgt", b"ACGt", b"ACGTNNNN", b"acgtnnnn", b"ACGT"]
    want = E.edit_matrix(recs)
    assert want[0, 1] == 4 and want[0, 2] == 1 and want[3, 4] == 8 and want[0, 5] == 0
    ss = gpu_ctx.seqset(recs)
    try:
        assert ss.alphabet_size == 10
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ss), E.triangle(want))
    finally:
        ss.close()


# ---------------------------------------------------------------- the cap, without a quadratic reference
def test_records_at_the_cap(gpu_ctx, torch, d2g):
    """65 535 symbols: 32 strips of 64 blocks.  x against x: 0; x against x with 4 000 symbols removed from its middle: 4 000 (the length
    difference is a lower bound, the deletions an upper one); disjoint alphabets: max(m, n)"""
    rng = np.random.default_rng(7300)
    n = d2g.EDIT_MAX_LEN
    x = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())
    cut = x[:30000] + x[34000:]
    y = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), n).tolist())
    ss = gpu_ctx.seqset([x, x, cut, y])
    try:
        assert ss.strip_blocks == 64
        got = ut_of(gpu_ctx, torch, ss)
        np.testing.assert_array_equal(got, [0, 4000, n, 4000, n, n])
    finally:
        ss.close()


def test_a_record_above_the_cap_is_unsupported(gpu_ctx, d2g):
    data = np.full(d2g.EDIT_MAX_LEN + 1 + 3, 65, np.uint8)
    off = np.array([0, 3, 3 + d2g.EDIT_MAX_LEN + 1], np.uint64)
    with pytest.raises(d2g.D2GError, match="65536") as e:
        d2g.seqset_check(data, off)
    assert e.value.status == -5
    with pytest.raises(d2g.D2GError, match="record 1") as e:
        gpu_ctx.seqset(data=data, off=off)
    assert e.value.status == -5
    off[2] -= 1
    gpu_ctx.seqset(data=data[:-1], off=off).close()                                # 65 535 is in


def test_a_set_of_another_context_is_refused_before_anything_is_written(gpu_ctx, torch, d2g):
    other = d2g.Context(0)
    ss = other.seqset([b"ACGT", b"AGT", b"T"])
    try:
        out = Out(torch, 3)
        assert d2g.lib().d2g_edit_ut_dev(gpu_ctx._h, ss._h, 0, 3, out.ptr, None) == -1
        assert d2g.lib().d2g_edit_rect_dev(gpu_ctx._h, ss._h, 0, 1, 0, 3, out.ptr, None) == -1
        gpu_ctx.sync()
        assert (out.t.cpu().numpy() == FILL).all()
        np.testing.assert_array_equal(ss.edit_ut(), [1, 3, 2])
    finally:
        ss.close()
        other.close()


def test_kernel_times_are_logged(gpu_ctx, torch, d2g):
    gpu_ctx.set_timing(d2g.TIME_EDIT)
    try:
        ss = gpu_ctx.seqset([b"ACGT" * 20, b"ACGA" * 21, b"T" * 7])
        ut_of(gpu_ctx, torch, ss)
        assert gpu_ctx.kernel_ms("edit")[0] == 1 and gpu_ctx.kernel_ms("editprep")[0] == 1
        ss.close()
    finally:
        gpu_ctx.set_timing(0)
