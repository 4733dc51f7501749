"""d2g_edit_near_dev / d2g_edit_within_dev / d2g_edit_knn (K2i, d2g_edit_near.hip) against edit_within_ref's model over edit_ref's dynamic
programme, and against pairs whose distance is known by construction.  Everything is compared as exact integers.

The seams: the band word of 64 bits (T <= 31: the band route, above it the full route over K2h's pair kernel and a clamp); the query's
table words of 32 rows, read three at a time at start >> 5; the length filter |len_i - len_j| <= T; empty records; tiles of 512 positions
of the order by length, rounds of 64 lanes; the early exit at 2T + n - m.  Every case checks on the CPU that what it expects is neither
empty nor complete (0 < nnz < N (N - 1)), so that none can pass on an all-zero or an all-pass band; the one case whose bound lets every
pair pass asserts that instead, and that its closeness takes many values.  Outputs lie between guard words pre-filled with 0xAB."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import edit_ref as E
import edit_within_ref as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xAB
FILLW = int.from_bytes(bytes([FILL]) * 4, "little")
SEAMS = [1, 31, 32, 33, 63, 64, 65, 96, 150, 257]
DNA = np.frombuffer(b"ACGT", np.uint8)


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
        return a[GUARD:GUARD + self.n]

    def read(self):
        return self.raw().astype(np.int64)


def near_of(gpu_ctx, torch, ss, T, r0=0, r1=None):
    r1 = ss.N if r1 is None else r1
    out = Out(torch, (r1 - r0) * ss.N)
    ss.near_dev(T, out.ptr, r0, r1)
    gpu_ctx.sync()
    return out.read().reshape(r1 - r0, ss.N)


def mutated(rng, x, edits, alphabet):
    y = list(x)
    for _ in range(edits):
        op = int(rng.integers(3))
        if op == 0 and y:
            y[int(rng.integers(len(y)))] = int(rng.choice(alphabet))
        elif op == 1 and len(y) > 1:
            del y[int(rng.integers(len(y)))]
        else:
            y.insert(int(rng.integers(len(y) + 1)), int(rng.choice(alphabet)))
    return bytes(y)


def inserted(rng, x, k, alphabet):
    y = list(x)
    for _ in range(k):
        y.insert(int(rng.integers(len(y) + 1)), int(rng.choice(alphabet)))
    return bytes(y)


def nnz_of(d, T):
    n = d.shape[0]
    return int((d <= T).sum()) - n


def check_partial(d, T):
    n = d.shape[0]
    assert 0 < nnz_of(d, T) < n * (n - 1), f"the case expects an empty or a complete result at T = {T}"


@functools.lru_cache(maxsize=None)
def seam_family():
    """prefixes of one base at the seam lengths, each twice (duplicates) and with 1, 2, 16, 31 and 34 random edits, shuffled: families inside
    and across lengths, length differences of 1, 2, 31, 32, 33.  -> (records, distance matrix)"""
    rng = np.random.default_rng(8200)
    base = bytes(rng.choice(DNA, 300).tolist())
    recs = []
    for n in SEAMS:
        recs += [base[:n], base[:n]] + [mutated(rng, base[:n], e, DNA) for e in (1, 2, 16, 31, 34)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    return recs, E.edit_matrix(recs)


# ---------------------------------------------------------------- the closeness band
@pytest.mark.parametrize("T", [0, 1, 2, 15, 30, 31, 32, 33])
def test_band_against_the_model_at_the_word_seams(gpu_ctx, torch, T):
    """T <= 31: the band kernel; 32, 33: the pair kernel over the window and the clamp"""
    recs, d = seam_family()
    check_partial(d, T)
    ss = gpu_ctx.seqset(recs)
    try:
        got = near_of(gpu_ctx, torch, ss, T)
        np.testing.assert_array_equal(got, W.closeness(d, T))
        assert (np.diag(got) == T + 1).all()
    finally:
        ss.close()


@pytest.mark.parametrize("T", [7, 16, 31])
def test_band_route_on_short_queries_with_a_wide_bound(gpu_ctx, torch, d2g, monkeypatch, T):
    """D2G_EDIT_NEAR_ROUTE=1: the rows of 9 to 32 symbols with 5T >= their length, which the dispatcher gives to the pair kernel, on the
    band kernel: the band wider than the query (T > m), the score on the last row from the first column on.  The kernel times say that
    the switch was heeded: one bracket of the band kernel and none of the pair kernel, where the dispatcher's own choice runs both"""
    recs, d = seam_family()
    check_partial(d, T)
    ss = gpu_ctx.seqset(recs)
    gpu_ctx.set_timing(d2g.TIME_EDIT_NEAR | d2g.TIME_EDIT)
    try:
        for name in ("editnear", "edit"):
            gpu_ctx.kernel_ms(name)
        near_of(gpu_ctx, torch, ss, T)
        assert gpu_ctx.kernel_ms("edit")[0] >= 1, "the dispatcher sent no row of the family to the pair kernel: the case forces nothing"
        gpu_ctx.kernel_ms("editnear")
        monkeypatch.setenv("D2G_EDIT_NEAR_ROUTE", "1")
        got = near_of(gpu_ctx, torch, ss, T)
        assert gpu_ctx.kernel_ms("editnear")[0] == 1 and gpu_ctx.kernel_ms("edit")[0] == 0
        np.testing.assert_array_equal(got, W.closeness(d, T))
    finally:
        for name in ("editnear", "edit"):
            gpu_ctx.kernel_ms(name)
        gpu_ctx.set_timing(0)
        ss.close()


@functools.lru_cache(maxsize=None)
def long_beside_short():
    """records of about 2 100 symbols (66 blocks: more than a strip of the pair kernel holds, more than 2 048 rows of the band's query)
    beside short ones and an empty one"""
    rng = np.random.default_rng(8201)
    base = bytes(rng.choice(DNA, 2100).tolist())
    recs = [base, mutated(rng, base, 5, DNA), mutated(rng, base, 31, DNA), base[:2080], mutated(rng, base, 45, DNA), base[10:], b""]
    recs += [base[:n] for n in (1, 33, 64, 150)] + [mutated(rng, base[:150], 3, DNA), mutated(rng, base[:64], 2, DNA), base[:31]]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    return recs, E.edit_matrix(recs)


@pytest.mark.parametrize("T", [300, 700])
def test_full_route_with_a_wide_bound(gpu_ctx, torch, T):
    """T = 300 and 700 on the seam family beside records of 700 and of 1 000 symbols: the full route with a window that is most of the
    set, the length filter on the long records"""
    recs, d = seam_family()
    rng = np.random.default_rng(8202 + T)
    x = bytes(rng.choice(DNA, 700).tolist())
    extra = [x, mutated(rng, x, 20, DNA), x + x[:300]]
    de = E.edit_matrix(extra)
    n0 = len(recs)
    full = np.zeros((n0 + 3, n0 + 3), np.int64)
    full[:n0, :n0] = d
    full[n0:, n0:] = de
    for i, r in enumerate(recs):
        for k, e in enumerate(extra):
            full[i, n0 + k] = full[n0 + k, i] = E.edit_distance(r, e)
    check_partial(full, T)
    ss = gpu_ctx.seqset(list(recs) + extra)
    try:
        np.testing.assert_array_equal(near_of(gpu_ctx, torch, ss, T), W.closeness(full, T))
    finally:
        ss.close()


def test_a_bound_above_the_longest_record_lets_every_pair_pass(gpu_ctx, torch):
    """the seam family with an empty record.  T >= the longest record: complete on purpose (the one case that is), far from constant; T = 31: the empty
    record beside the band route, d = the other's length"""
    fam, dfam = seam_family()
    recs = list(fam) + [b""]
    lens = np.array([len(r) for r in recs], np.int64)
    d = np.zeros((len(recs), len(recs)), np.int64)
    d[:-1, :-1] = dfam
    d[-1, :] = lens
    d[:, -1] = lens
    top = int(lens.max())                                                            # (a mutated record of 257 symbols may have grown)
    assert 257 <= top <= 300
    for T in (top, 300):
        want = W.closeness(d, T)
        assert (want > 0).all() and np.unique(want).size > 50
        ss = gpu_ctx.seqset(recs)
        try:
            np.testing.assert_array_equal(near_of(gpu_ctx, torch, ss, T), want)
        finally:
            ss.close()
    check_partial(d, 31)
    ss = gpu_ctx.seqset(recs)
    try:
        got = near_of(gpu_ctx, torch, ss, 31)
        np.testing.assert_array_equal(got, W.closeness(d, 31))
        assert got[-1, -1] == 32 and (got[-1, :-1] == np.maximum(0, 32 - lens[:-1])).all()
    finally:
        ss.close()


# ---------------------------------------------------------------- the bound's edges, by construction
@pytest.mark.parametrize("T", [0, 1, 2, 15, 30, 31, 32, 40])
def test_the_edges_of_the_bound(gpu_ctx, torch, T):
    rng = np.random.default_rng(8300 + T)
    x = bytes(rng.choice(DNA, 100).tolist())
    s = bytes(rng.choice(DNA, 120).tolist())
    h = T // 2
    recs = [x, x,                                     # 0, 1: duplicates, d = 0
            inserted(rng, x, T, DNA),                 # 2: T insertions: d = T, |dlen| = T passes the filter and hugs the band's edge
            inserted(rng, x, T + 1, DNA),             # 3: T + 1 insertions: d = T + 1, filtered by length
            b"x" * h + s, s + b"y" * h,               # 4, 5: d = 2 h, the optimal path runs h off the main diagonal throughout
            b"AC" * 10, b"gt" * 12 + b"g",            # 6, 7: disjoint alphabets: d = 25, the longer length
            bytes(rng.choice(DNA, 100).tolist())]     # 8: unrelated
    d = E.edit_matrix(recs)
    assert d[0, 1] == 0 and d[0, 2] == T and d[0, 3] == T + 1 and d[4, 5] == 2 * h and d[6, 7] == 25
    assert len(recs[2]) - len(x) == T and len(recs[3]) - len(x) == T + 1
    check_partial(d, T)
    ss = gpu_ctx.seqset(recs)
    try:
        got = near_of(gpu_ctx, torch, ss, T)
        np.testing.assert_array_equal(got, W.closeness(d, T))
        assert got[0, 1] == T + 1 and got[0, 2] == 1 and got[2, 0] == 1 and got[0, 3] == 0 and got[3, 0] == 0
        assert got[4, 5] == T + 1 - 2 * h and got[6, 7] == max(0, T + 1 - 25)
    finally:
        ss.close()


# ---------------------------------------------------------------- alphabets
@pytest.mark.parametrize("T", [2, 31])
@pytest.mark.parametrize("sigma", [1, 256])
def test_alphabets(gpu_ctx, torch, sigma, T):
    rng = np.random.default_rng(8400 + sigma)
    if sigma == 1:
        recs = [b"a" * n for n in (1, 2, 3, 31, 32, 33, 34, 60, 64, 65, 96, 97, 150, 152)]
    else:
        alphabet = np.arange(256, dtype=np.uint8)
        base = bytes(range(256)) + bytes(rng.choice(alphabet, 44).tolist())
        recs = [base, base[:150], base[:150]] + [mutated(rng, base[:n], e, alphabet) for n in (33, 64, 150, 257, 300) for e in (1, 3, 20)]
        recs += [bytes(rng.choice(alphabet, n).tolist()) for n in (1, 64, 150)]
    d = E.edit_matrix(recs)
    if sigma == 1:
        lens = np.array([len(r) for r in recs])
        np.testing.assert_array_equal(d, np.abs(lens[:, None] - lens[None, :]))
    check_partial(d, T)
    ss = gpu_ctx.seqset(recs)
    try:
        assert ss.alphabet_size == sigma
        np.testing.assert_array_equal(near_of(gpu_ctx, torch, ss, T), W.closeness(d, T))
    finally:
        ss.close()


def test_upper_and_lower_case_differ(gpu_ctx, torch):
    recs = [b"ACGT", b"acgt", b"ACGt", b"ACGTNNNN", b"acgtnnnn", b"ACGT"]
    d = E.edit_matrix(recs)
    assert d[0, 1] == 4 and d[0, 2] == 1 and d[0, 5] == 0
    for T in (1, 3, 4):
        check_partial(d, T)
        ss = gpu_ctx.seqset(recs)
        try:
            got = near_of(gpu_ctx, torch, ss, T)
            np.testing.assert_array_equal(got, W.closeness(d, T))
            assert got[0, 1] == max(0, T + 1 - 4)
        finally:
            ss.close()


# ---------------------------------------------------------------- strips and classes
@pytest.mark.parametrize("T", [31, 40])
def test_long_records_beside_short_ones(gpu_ctx, torch, T):
    """T = 31: the band route with a query of more than 2 048 rows; T = 40: the pair kernel's several-strip class beside its short classes"""
    recs, d = long_beside_short()
    check_partial(d, T)
    ss = gpu_ctx.seqset(recs)
    try:
        np.testing.assert_array_equal(near_of(gpu_ctx, torch, ss, T), W.closeness(d, T))
    finally:
        ss.close()


CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import dashing2_amd as D
doc = json.load(open(sys.argv[2]))
recs = [bytes.fromhex(h) for h in doc["records"]]
ctx = D.Context(0)
ss = ctx.seqset(recs)
assert ss.strip_blocks == 1
out = {}
for T in doc["bounds"]:
    buf = ctx.malloc(ss.N * ss.N * 4)
    ss.near_dev(T, buf)
    ctx.sync()
    got = np.zeros((ss.N, ss.N), np.uint32)
    ctx.d2h(got, buf)
    ctx.free(buf)
    out[str(T)] = got.tolist()
ss.close()
ctx.close()
print(json.dumps(out))
"""


def test_forced_strips_and_tiles_in_a_fresh_process(tmp_path):
    """D2G_EDIT_STRIP=1 and D2G_EDIT_TILE=3: the full route through the pair kernel's several-strip form on every record of more than 32
    symbols, both routes with tiles of three positions (many workgroups per row, tiles without a pair inside the bound)"""
    recs, d = long_beside_short()
    bounds = [31, 40]
    for T in bounds:
        check_partial(d, T)
    p = tmp_path / "records.json"
    p.write_text(json.dumps({"records": [r.hex() for r in recs], "bounds": bounds}))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(p)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, D2G_EDIT_STRIP="1", D2G_EDIT_TILE="3"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for T in bounds:
        np.testing.assert_array_equal(np.array(got[str(T)], np.int64), W.closeness(d, T), err_msg=f"T = {T}")


# ---------------------------------------------------------------- within_dev's contract
def within_of(gpu_ctx, torch, ss, K, T, cap, r0=0, r1=None, band_rows=0):
    r1 = ss.N if r1 is None else r1
    cnt, ids, cls = Out(torch, r1 - r0), Out(torch, (r1 - r0) * cap), Out(torch, (r1 - r0) * cap)
    ss.within_dev(cnt.ptr, ids.ptr if cap else None, cls.ptr if cap else None, cap, K=K, T=T, r0=r0, r1=r1, band_rows=band_rows)
    gpu_ctx.sync()
    return cnt.read(), ids.raw().reshape(r1 - r0, cap) if cap else None, cls.raw().reshape(r1 - r0, cap) if cap else None


def expect_rows(d, K, T, r0, r1):
    """per row the qualifying columns in ASCENDING j (the device's order) and their closeness"""
    n = d.shape[0]
    rows = []
    for i in range(r0, r1):
        js = [j for j in range(n) if j != i and d[i, j] <= T]
        if K and len(js) > K:
            kth = sorted(int(d[i, j]) for j in js)[K - 1]
            js = [j for j in js if d[i, j] <= kth]
        rows.append((js, [T + 1 - int(d[i, j]) for j in js]))
    return rows


@pytest.mark.parametrize("K,T,band_rows", [(0, 2, 0), (0, 31, 1), (3, 16, 0), (2, 33, 7), (1, 1, 0)])
def test_within_dev_contract(gpu_ctx, torch, K, T, band_rows):
    recs, d = seam_family()
    check_partial(d, T)
    n = len(recs)
    ss = gpu_ctx.seqset(recs)
    try:
        want = expect_rows(d, K, T, 0, n)
        widest = max(len(js) for js, _ in want)
        assert widest >= 2 and any(d[i, j] == 0 for i in range(n) for j in range(n) if i != j)
        for cap in (widest, 1, 0):                                                    # everything fits; rows overflow; counting only
            cnt, ids, cls = within_of(gpu_ctx, torch, ss, K, T, cap, band_rows=band_rows)
            np.testing.assert_array_equal(cnt, [len(js) for js, _ in want], err_msg=f"rowcnt at cap {cap}")
            for i, (js, cs) in enumerate(want if cap else []):
                k = min(len(js), cap)
                assert ids[i, :k].tolist() == js[:k] and cls[i, :k].tolist() == cs[:k], (i, cap)
                assert (ids[i, k:] == FILLW).all() and (cls[i, k:] == FILLW).all(), f"row {i}: written past its list"
                assert i not in js
        for r0, r1 in [(5, 6), (n - 1, n), (3, 29), (n // 2, n)]:                     # sub-ranges, one row among them
            cnt, ids, cls = within_of(gpu_ctx, torch, ss, K, T, widest, r0, r1, band_rows)
            sub = expect_rows(d, K, T, r0, r1)
            np.testing.assert_array_equal(cnt, [len(js) for js, _ in sub])
            for i, (js, cs) in enumerate(sub):
                assert ids[i, :len(js)].tolist() == js and cls[i, :len(js)].tolist() == cs
        cnt, _, _ = within_of(gpu_ctx, torch, ss, K, T, 4, 9, 9)                      # the empty range: D2G_OK, nothing written
        assert cnt.size == 0
        ss.within_dev(None, None, None, 0, K=K, T=T, r0=2, r1=2)
        ss.near_dev(T, None, 4, 4)
    finally:
        ss.close()


def test_a_set_of_another_context_is_refused_before_anything_is_written(gpu_ctx, torch, d2g):
    other = d2g.Context(0)
    ss = other.seqset([b"ACGT", b"AGT", b"T"])
    try:
        out = Out(torch, 9)
        assert d2g.lib().d2g_edit_near_dev(gpu_ctx._h, ss._h, 0, 3, 2, out.ptr, None) == -1
        assert d2g.lib().d2g_edit_within_dev(gpu_ctx._h, ss._h, 0, 3, 0, 2, 3, out.ptr, out.ptr, out.ptr, 0, None) == -1
        assert d2g.lib().d2g_edit_near_dev(other._h, ss._h, 0, 3, 2, None, None) == -1      # a null output
        assert d2g.lib().d2g_edit_near_dev(other._h, ss._h, 2, 4, 2, out.ptr, None) == -1   # rows out of range
        gpu_ctx.sync()
        assert (out.raw() == FILLW).all()
        ip, ix, dt = ss.knn(K=0, T=2)
        assert ip.tolist() == [0, 1, 3, 4] and ix.tolist() == [1, 0, 2, 1] and dt.tolist() == [1.0, 1.0, 2.0, 2.0]
    finally:
        ss.close()
        other.close()


# ---------------------------------------------------------------- knn: the host-pointer form
def assert_csr(got, lists, d, r0=0, r1=None):
    ip, ix, dt = W.csr_of(lists, d, r0, r1)
    np.testing.assert_array_equal(got[0], ip)
    np.testing.assert_array_equal(got[1], ix)
    assert got[2].dtype == np.float32
    np.testing.assert_array_equal(got[2], dt)


@pytest.mark.parametrize("T", [0, 2, 31, 40])
def test_knn_threshold_mode(gpu_ctx, T):
    recs, d = seam_family()
    check_partial(d, T)
    lists, _ = W.within_lists(recs, 0, T, d)
    ss = gpu_ctx.seqset(recs)
    try:
        assert_csr(ss.knn(K=0, T=T), lists, d)
        assert_csr(ss.knn(K=0, T=T, cap=1, band_rows=3), lists, d)                    # most rows overflow the cap and run again
        assert_csr(ss.knn(K=0, T=T, r0=11, r1=30), lists, d, 11, 30)
    finally:
        ss.close()


@pytest.mark.parametrize("K", [1, 3, "N-1", "N+5"])
def test_knn_topk_does_not_depend_on_the_starting_bound(gpu_ctx, K):
    recs, d = seam_family()
    n = len(recs)
    K = {"N-1": n - 1, "N+5": n + 5}.get(K, K)
    lists, _ = W.within_lists(recs, K, 0, d)
    nnz = sum(map(len, lists))
    assert 0 < nnz and (nnz < n * (n - 1) or K >= n - 1)                              # K >= N - 1 lists everybody, by definition
    if K == 1:
        assert any(len(js) > 1 for js in lists), "no row with a tie class at the K-th distance"
    ss = gpu_ctx.seqset(recs)
    try:
        first = None
        for start in (0, 2, 40):
            got = ss.knn(K=K, T=start)
            assert_csr(got, lists, d)
            first = got if first is None else first
            for a, b in zip(first, got):
                assert a.tobytes() == b.tobytes()
    finally:
        ss.close()


def test_knn_keeps_a_tie_class_at_the_kth_distance_whole(gpu_ctx):
    x = b"ACGTACGTACGTACGTACGT"
    recs = [x, x[:-1] + b"A", b"C" + x[1:], x[:9] + x[10:], x + b"A", x, b"TTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
    d = E.edit_matrix(recs)
    assert sorted(d[0, 1:].tolist())[:5] == [0, 1, 1, 1, 1]
    lists, _ = W.within_lists(recs, 2, 0, d)
    assert lists[0] == [5, 1, 2, 3, 4]                                               # the duplicate, then the whole class at distance 1 by id
    ss = gpu_ctx.seqset(recs)
    try:
        for start in (0, 1, 25):
            assert_csr(ss.knn(K=2, T=start), lists, d)
    finally:
        ss.close()


def test_knn_reports_the_size_it_needs(gpu_ctx, d2g):
    import ctypes as C
    recs, d = seam_family()
    lists, _ = W.within_lists(recs, 0, 16, d)
    check_partial(d, 16)
    ip_w, ix_w, dt_w = W.csr_of(lists, d)
    n = len(recs)
    ss = gpu_ctx.seqset(recs)
    try:
        ip, ix, dt = np.zeros(n + 1, np.uint64), np.full(ix_w.size, 7, np.uint32), np.full(ix_w.size, 7, np.float32)
        need = C.c_size_t(0)
        call = lambda cap: d2g.lib().d2g_edit_knn(gpu_ctx._h, ss._h, 0, n, 0, 16, 0, 0, ip.ctypes.data, ix.ctypes.data, dt.ctypes.data, cap, C.byref(need))
        assert call(ix_w.size - 1) == -4 and need.value == ix_w.size                  # D2G_ERR_NOMEM
        assert (ix == 7).all() and (dt == 7).all()
        assert call(need.value) == 0 and need.value == ix_w.size
        np.testing.assert_array_equal(ip, ip_w)
        np.testing.assert_array_equal(ix, ix_w)
        np.testing.assert_array_equal(dt, dt_w)
        assert d2g.lib().d2g_edit_knn(gpu_ctx._h, ss._h, 3, n + 1, 0, 16, 0, 0, ip.ctypes.data, ix.ctypes.data, dt.ctypes.data, ix.size, C.byref(need)) == -1
    finally:
        ss.close()


# ---------------------------------------------------------------- beside the new routes
def test_the_pair_kernel_still_returns_the_matrix(gpu_ctx):
    recs, d = seam_family()
    ss = gpu_ctx.seqset(recs)
    try:
        np.testing.assert_array_equal(ss.edit_ut(), E.triangle(d))
    finally:
        ss.close()


def test_kernel_times_are_logged(gpu_ctx, torch, d2g):
    gpu_ctx.set_timing(d2g.TIME_EDIT_NEAR | d2g.TIME_EDIT | d2g.TIME_KNN)
    try:
        ss = gpu_ctx.seqset([b"ACGT" * 20, b"ACGA" * 21, b"T" * 40])   # every query above 32 symbols: one route per call
        for name in ("editnear", "edit", "knn"):
            gpu_ctx.kernel_ms(name)
        near_of(gpu_ctx, torch, ss, 3)
        assert gpu_ctx.kernel_ms("editnear")[0] == 1 and gpu_ctx.kernel_ms("edit")[0] == 0
        near_of(gpu_ctx, torch, ss, 40)
        assert gpu_ctx.kernel_ms("editnear")[0] == 1 and gpu_ctx.kernel_ms("edit")[0] == 1   # the clamp, behind the pair kernel
        ss.knn(K=0, T=3)
        assert gpu_ctx.kernel_ms("knn")[0] >= 1
        ss.close()
    finally:
        for name in ("editnear", "edit", "editprep", "knn"):                          # leave no bracket behind for the tests that count them
            gpu_ctx.kernel_ms(name)
        gpu_ctx.set_timing(0)
