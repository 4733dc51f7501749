"""d2g_edit_dedup_dev / d2g_edit_dedup (K2j, d2g_edit_dedup.hip) against edit_dedup_ref's model over edit_ref's dynamic programme, and
against cases whose clusters are known by construction.  Everything is compared as exact integers.

Every case first asserts on the CPU that what it expects is not trivial (1 < clusters < N; the cases that are trivial on purpose say
so), runs D2G_EDIT_DEDUP_ROUTE = 0 (the dispatcher), 1 (the list kernel wherever it exists) and 2 (d2g_edit_near_dev over all columns
for every row), asserts that each equals the model, and hands the result to d2g_dedup_clusters.  The seams: the 64-bit band word
(T <= 31 / above), the query's table words, the length filter, empty records, bands of 256 rows and smaller ones, the band's own block
against the representative list of earlier bands, tiles of the list and rounds of 64 lanes, rows of both routes in one band.  The
output lies between guard words pre-filled with 0xAB."""
import numpy as np
import pytest

import dedup_ref as D
import edit_dedup_cases as C
import edit_dedup_ref as R
import edit_ref as E

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xAB
FILLW = int.from_bytes(bytes([FILL]) * 4, "little")


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

    def raw(self):
        a = self.t.cpu().numpy().view(np.uint32)
        assert (a[:GUARD] == FILLW).all() and (a[GUARD + self.n:] == FILLW).all(), "guard words around the output were written"
        return a[GUARD:GUARD + self.n].copy()


def dedup_of(gpu_ctx, torch, ss, T, band_rows=0):
    out = Out(torch, ss.N)
    ss.dedup_dev(out.ptr, T, band_rows)
    gpu_ctx.sync()
    return out.raw()


def check_clusters(d2g, assign):
    """d2g_dedup_clusters accepts the result and gives the model's clusters"""
    indptr, indices = d2g.dedup_clusters(assign)
    ids, cons = D.clusters_of(assign)
    assert len(indptr) == len(ids) + 1
    for c, (rep, members) in enumerate(zip(ids, cons)):
        assert indices[int(indptr[c]):int(indptr[c + 1])].tolist() == [rep] + members


def all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, T, band_rows=0, trivial=False):
    """routes 0, 1, 2 against `want` (and so against each other), then d2g_dedup_clusters"""
    want = np.asarray(want, np.uint32)
    if not trivial:
        assert 1 < R.n_clusters(want) < len(recs), "the case expects a trivial clustering"
    ss = gpu_ctx.seqset(recs)
    try:
        for route in (0, 1, 2):
            monkeypatch.setenv("D2G_EDIT_DEDUP_ROUTE", str(route))
            got = dedup_of(gpu_ctx, torch, ss, T, band_rows)
            np.testing.assert_array_equal(got, want, err_msg=f"route {route}, T = {T}, band_rows = {band_rows}")
        check_clusters(d2g, got)
    finally:
        ss.close()


# ---------------------------------------------------------------- word seams
@pytest.mark.parametrize("band_rows", [1, 32, 0])
@pytest.mark.parametrize("T,clusters", list(zip([0, 1, 2, 15, 30, 31, 32, 33], [57, 48, 39, 21, 8, 8, 9, 8])))
def test_word_seams(gpu_ctx, torch, d2g, monkeypatch, T, clusters, band_rows):
    """T <= 31: the list kernel (routes 0 and 1); T = 32, 33: every route is the all-columns route"""
    recs, d = C.seam_family()
    want = R.greedy_assign(d, T)
    assert R.n_clusters(want) == clusters
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, T, band_rows)


# ---------------------------------------------------------------- what greedy can get wrong
@pytest.mark.parametrize("band_rows", [32, 0])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 8])
def test_chains(gpu_ctx, torch, d2g, monkeypatch, T, band_rows):
    """single-edit walks: ties for the nearest representative, non-representatives nearer than every representative, representatives
    with a non-representative within the bound, joins inside the band and across bands (test_edit_dedup_ref.py has the counts)"""
    recs, d = C.chains()
    c = R.census(d, T, band_rows or 256)
    for k in ("ties", "nearer_nonrep", "rep_despite_nonrep", "joins_same_band") + (("joins_earlier_band",) if band_rows else ()):
        assert c[k] > 0, k
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, R.greedy_assign(d, T), T, band_rows)


# ---------------------------------------------------------------- band seams
@pytest.mark.parametrize("n,clusters", [(1, 1), (2, 2), (255, 108), (256, 108), (257, 108), (513, 129)])
def test_band_seams(gpu_ctx, torch, d2g, monkeypatch, n, clusters):
    """the default band of 256 rows: one band short of full, full, one row into the second (that row joins a representative of the
    first), two bands and a row.  N = 1 and N = 2 are trivial on purpose (two unrelated records)"""
    recs, d = C.band_family()
    want = R.greedy_assign(d[:n, :n], 2)
    assert R.n_clusters(want) == clusters
    if n == 257:
        assert want[256] != 256
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs[:n], want, 2, trivial=n <= 2)


@pytest.mark.parametrize("tile", [32, 64, 200])
def test_list_tiles_and_rounds(gpu_ctx, torch, d2g, monkeypatch, tile):
    """206 representatives at T = 1: the list of the third band spans several tiles of D2G_EDIT_TILE positions, the last one ragged;
    written backwards (D2G_EDIT_DEDUP_REVERSE) the list gives the same clusters: the reduction does not depend on its order"""
    recs, d = C.band_family()
    want = R.greedy_assign(d, 1)
    assert R.n_clusters(want) == 206 and R.n_clusters(want[:512]) % tile != 0
    monkeypatch.setenv("D2G_EDIT_TILE", str(tile))
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, 1)
    monkeypatch.setenv("D2G_EDIT_DEDUP_REVERSE", "1")
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, 1, band_rows=100)


def test_length_filter(gpu_ctx, torch, d2g, monkeypatch):
    """records of 10 to 200 symbols: most tiles of the list hold no record within T of the row's length"""
    recs, d = C.ragged()
    want = R.greedy_assign(d, 3)
    assert R.n_clusters(want) == 58
    for band_rows in (0, 16):
        all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, 3, band_rows)


# ---------------------------------------------------------------- known by construction
@pytest.mark.parametrize("band_rows", [0, 1])
def test_cases_known_by_construction(gpu_ctx, torch, d2g, monkeypatch, band_rows):
    x = b"ACGTACGTAC"
    cases = [
        ([b"AAGTACGTAC", b"ACGTACGTAA", x], 1, [0, 1, 0], False),       # equidistant representatives: the smaller index wins ...
        ([b"ACGTACGTAA", b"AAGTACGTAC", x], 1, [0, 1, 0], False),       # ... in both input orders
        ([b"AAAA", b"AAAT", b"AATT"], 1, [0, 0, 2], False),            # A ~ B ~ C, A !~ C
        ([b"AC", b"AG", b"AC", b"AG", b"AC"], 0, [0, 1, 0, 1, 0], False),   # exact duplicates at T = 0
        ([b"", b"A", b""], 0, [0, 1, 0], False),                       # two empty records and a record of one symbol
        ([b"", b"A", b""], 1, [0, 0, 0], True),                        # ... within one edit of each other: one cluster
        ([b"", b"ACG", b"ACGT"], 3, [0, 0, 2], False),                 # d(x, "") = |x|
    ]
    for recs, T, want, trivial in cases:
        np.testing.assert_array_equal(R.greedy_assign(E.edit_matrix(recs), T), want)
        all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, T, band_rows, trivial=trivial)


@pytest.mark.parametrize("above", [0, 50])
def test_a_bound_of_the_longest_record_gives_one_cluster(gpu_ctx, torch, d2g, monkeypatch, above):
    """complete on purpose: no distance exceeds the longest record"""
    recs, d = C.seam_family()
    T = max(map(len, recs)) + above
    want = R.greedy_assign(d, T)
    assert (want == 0).all()
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, T, trivial=True)


# ---------------------------------------------------------------- rows of both routes in one band
@pytest.mark.parametrize("band_rows", [0, 8])
def test_mixed_bands(gpu_ctx, torch, d2g, monkeypatch, band_rows):
    """two records of 2 000 symbols over 256 byte values (no band kernel: their table does not fit) three edits apart, among DNA of 9 .. 32
    and 100 .. 150 symbols, T = 7.  band_rows = 8: the second long record finds the first through the representatives of an earlier band"""
    recs, d = C.mixed()
    want = R.greedy_assign(d, 7)
    assert want[29] == 7 and want[7] == 7
    all_routes(gpu_ctx, torch, d2g, monkeypatch, recs, want, 7, band_rows)


# ---------------------------------------------------------------- randomised
def test_random_sets(gpu_ctx, torch, d2g, monkeypatch):
    sets, mats = C.random_sets(), C.random_matrices()
    wants = [R.greedy_assign(d, T) for (_, T, _), d in zip(sets, mats)]
    assert sum(1 < R.n_clusters(w) < len(w) for w in wants) >= len(sets) // 2
    for route in (0, 1, 2):
        monkeypatch.setenv("D2G_EDIT_DEDUP_ROUTE", str(route))
        for k, ((recs, T, band_rows), want) in enumerate(zip(sets, wants)):
            ss = gpu_ctx.seqset(recs)
            try:
                got = dedup_of(gpu_ctx, torch, ss, T, band_rows)
                np.testing.assert_array_equal(got, want, err_msg=f"set {k}, route {route}")
            finally:
                ss.close()
    check_clusters(d2g, got)


# ---------------------------------------------------------------- the host form, the shared scratch, refusals
def test_host_form_repeats_and_shared_scratch(gpu_ctx, torch, d2g):
    recs, d = C.chains()
    want = R.greedy_assign(d, 3)
    assert 1 < R.n_clusters(want) < len(recs)
    ss = gpu_ctx.seqset(recs)
    try:
        first = dedup_of(gpu_ctx, torch, ss, 3, 32)
        np.testing.assert_array_equal(first, want)
        np.testing.assert_array_equal(ss.dedup(3, 32), first)                        # the host form
        np.testing.assert_array_equal(dedup_of(gpu_ctx, torch, ss, 3, 32), first)    # a second call: the same words
    finally:
        ss.close()
    # behind within_dev on the same stream: the scratch band they share (T = 32 is the all-columns route, which uses it)
    recs, d = C.seam_family()
    want = R.greedy_assign(d, 32)
    assert 1 < R.n_clusters(want) < len(recs)
    ss = gpu_ctx.seqset(recs)
    try:
        n = ss.N
        cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        out = Out(torch, n)
        ss.within_dev(cnt.data_ptr(), 0, 0, 0, K=0, T=40)
        ss.dedup_dev(out.ptr, 32, 32)
        ss.within_dev(cnt.data_ptr(), 0, 0, 0, K=0, T=3)
        gpu_ctx.sync()
        np.testing.assert_array_equal(out.raw(), want)
        np.testing.assert_array_equal(cnt.cpu().numpy(), (d <= 3).sum(1) - 1)
    finally:
        ss.close()


def test_a_set_of_another_context_is_refused_before_anything_is_written(gpu_ctx, torch, d2g):
    other = d2g.Context(0)
    ss = other.seqset([b"ACGT", b"AGT", b"T"])
    try:
        out = Out(torch, 3)
        assert d2g.lib().d2g_edit_dedup_dev(gpu_ctx._h, ss._h, 2, out.ptr, 0, None) == -1
        assert b"another context" in d2g.lib().d2g_last_error(gpu_ctx._h)
        assert d2g.lib().d2g_edit_dedup_dev(other._h, ss._h, 2, None, 0, None) == -1     # a null output
        host = np.full(3, FILLW, np.uint32)
        assert d2g.lib().d2g_edit_dedup(gpu_ctx._h, ss._h, 2, 0, host.ctypes.data) == -1
        other.sync()
        gpu_ctx.sync()
        assert (out.raw() == FILLW).all() and (host == FILLW).all()
        np.testing.assert_array_equal(ss.dedup(2), R.greedy_assign(E.edit_matrix([b"ACGT", b"AGT", b"T"]), 2))
    finally:
        ss.close()
        other.close()


def test_an_empty_set_does_nothing(gpu_ctx, d2g):
    ss = gpu_ctx.seqset([])
    try:
        assert d2g.lib().d2g_edit_dedup_dev(gpu_ctx._h, ss._h, 2, None, 0, None) == 0
        assert ss.dedup(2).size == 0
    finally:
        ss.close()


def test_kernel_times_are_logged_per_band(gpu_ctx, d2g):
    recs, d = C.seam_family()
    ss = gpu_ctx.seqset(recs)
    gpu_ctx.set_timing(d2g.TIME_EDIT_DEDUP)
    try:
        for name in ("editdedup", "editdedup_list", "editdedup_resolve"):
            gpu_ctx.kernel_ms(name)
        np.testing.assert_array_equal(ss.dedup(2, 32), R.greedy_assign(d, 2))
        for name in ("editdedup", "editdedup_list", "editdedup_resolve"):
            assert gpu_ctx.kernel_ms(name)[0] == 3, name                               # one bracket per band of 32 rows: 70 records
    finally:
        for name in ("editdedup", "editdedup_list", "editdedup_resolve"):
            gpu_ctx.kernel_ms(name)
        gpu_ctx.set_timing(0)
        ss.close()
