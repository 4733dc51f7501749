"""d2g_kset_isz_ut_dev and d2g_kset_isz_rect_dev (kset_pair_kernel) on sets CONSTRUCTED so that the answer is known without running
anything -- slices of one sorted pool of distinct keys: disjoint, identical, nested, a shared prefix or suffix of known length -- and on
random sets against exact_ref.isz_matrix (NumPy's intersect1d; nothing the product computed).  Everything is compared as exact u64.

The kernel's seams (d2g_kset_cmp.hip): tiles of 4 x 4 sets, one wave per row set; LDS chunks of 1024 keys per column set; 2^p slices by
the top p key bits (D2G_KSET_PBITS forces p); the slice range split over workgroups that add atomically, or one workgroup per tile that
stores (D2G_KSET_SPLIT forces either).  Outputs lie between guard words pre-filled with 0xAB."""
import functools

import numpy as np
import pytest

import exact_ref as X
import k3_seam_cases as C

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xAB
TW, CHUNK = 4, 1024
U32MAX = 2 ** 32 - 1


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def pool(n=24000, seed=4100, lo=0, hi=2 ** 64):
    p = X.rng_keys(seed, n, lo, hi)
    p.setflags(write=False)
    return p


def ones(keys):
    return np.ones(len(keys), np.uint32)


class Out:
    def __init__(self, torch, n):
        self.n = n
        self.t = torch.full(((2 * GUARD + n) * 8,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * 8

    def read(self):
        a, fill = self.t.cpu().numpy().view(np.uint64), np.uint64(int.from_bytes(bytes([FILL]) * 8, "little"))
        assert (a[:GUARD] == fill).all() and (a[GUARD + self.n:] == fill).all(), "guard words around the output were written"
        return a[GUARD:GUARD + self.n]


def make(gpu_ctx, sets, weighted):
    keys, counts, off, _ = X.flat(sets)
    return gpu_ctx.kset(keys, counts if weighted else None, off)


def ut_of(gpu_ctx, torch, ks, r0=0, r1=None):
    r1 = ks.N if r1 is None else r1
    n = sum(ks.N - 1 - i for i in range(r0, r1))
    out = Out(torch, n)
    ks.isz_ut_dev(r0, r1, out.ptr)
    gpu_ctx.sync()
    return out.read()


def rect_of(gpu_ctx, torch, ks, a0, a1, b0, b1):
    out = Out(torch, (a1 - a0) * (b1 - b0))
    ks.isz_rect_dev(a0, a1, b0, b1, out.ptr)
    gpu_ctx.sync()
    return out.read().reshape(a1 - a0, b1 - b0)


def check_all(gpu_ctx, torch, sets, weighted, want=None):
    """the whole upper triangle and the whole square against `want` (default: exact_ref.isz_matrix)"""
    want = X.isz_matrix(sets, weighted) if want is None else want
    ks = make(gpu_ctx, sets, weighted)
    try:
        np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ks), X.ut(want), err_msg="upper triangle")
        np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ks, 0, ks.N, 0, ks.N), want, err_msg="square")
    finally:
        ks.close()
    return want


# ---------------------------------------------------------------- answers known by construction
def test_disjoint_identical_nested_and_shared_ends(gpu_ctx, torch):
    p = pool()
    sets = [p[0:1000], p[1000:1800], p[0:1000], p[100:300], p[600:1400], p[0:2500], p[2400:2500]]
    want = np.zeros((7, 7), np.uint64)
    spans = [(0, 1000), (1000, 1800), (0, 1000), (100, 300), (600, 1400), (0, 2500), (2400, 2500)]
    for i, (a, b) in enumerate(spans):
        for j, (c, d) in enumerate(spans):
            want[i, j] = max(0, min(b, d) - max(a, c))                    # the pool is strictly ascending: overlap of the index ranges
    assert want[0, 1] == 0 and want[0, 2] == 1000 and want[0, 3] == 200 and want[0, 4] == 400 and want[1, 4] == 400 and want[5, 6] == 100
    got = check_all(gpu_ctx, torch, [(s, ones(s)) for s in sets], False, want)
    np.testing.assert_array_equal(got, X.isz_matrix([(s, ones(s)) for s in sets], False))


# ---------------------------------------------------------------- N around the tile width, rows and blocks that cut tiles
@functools.lru_cache(maxsize=None)
def family(n, seed=4200, lo=0, hi=700):
    """n sets, each a random subset of the first 1500 pool keys, set 2 (if any) empty"""
    rng = np.random.default_rng(seed + n)
    p = pool()[:1500]
    out = []
    for i in range(n):
        m = 0 if i == 2 else int(rng.integers(lo + 1, hi))
        k = np.sort(rng.choice(p, m, replace=False))
        out.append((k, rng.integers(1, 9, m).astype(np.uint32)))
    return out


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
@pytest.mark.parametrize("n", [1, 2, TW - 1, TW, TW + 1, 2 * TW + 1])
def test_n_below_at_and_above_the_tile_width(gpu_ctx, torch, n, weighted):
    want = check_all(gpu_ctx, torch, family(n), weighted)
    assert n < 2 or want.max() > 0
    for i, (k, c) in enumerate(family(n)):
        assert want[i, i] == X.card(k, c, weighted)                       # a set against itself: its cardinality


def test_rows_and_blocks_that_cut_a_tile(gpu_ctx, torch):
    n = 2 * TW + 3
    sets = family(n)
    want = X.isz_matrix(sets, True)
    ks = make(gpu_ctx, sets, True)
    try:
        for r0, r1 in [(0, n), (1, 6), (3, 4), (5, 5), (n - 1, n), (n - 2, n), (4, 8), (0, 1)]:
            np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ks, r0, r1), X.ut(want, r0, r1), err_msg=f"rows [{r0}, {r1})")
        for a0, a1, b0, b1 in [(1, 6, 3, n), (0, 3, 5, n), (5, n, 0, 3), (2, 3, 2, 3), (0, n, 4, 5), (3, 10, 3, 10)]:     # overlapping, disjoint
            np.testing.assert_array_equal(rect_of(gpu_ctx, torch, ks, a0, a1, b0, b1), want[a0:a1, b0:b1], err_msg=f"block [{a0},{a1}) x [{b0},{b1})")
    finally:
        ks.close()


# ---------------------------------------------------------------- slices: empty ones, and the LDS chunk on either side
def test_slices_without_keys_and_an_empty_set_in_a_tile(gpu_ctx, torch, monkeypatch):
    """p = 3: set 0 has keys in every slice, set 1 only below 2^61 (slice 0), set 2 is empty, set 3 only in the top slice"""
    monkeypatch.setenv("D2G_KSET_PBITS", "3")
    lowp, topp = pool(3000, 4300, 0, 2 ** 61), pool(3000, 4301, 7 * 2 ** 61, 2 ** 64)
    allp = np.sort(np.concatenate([lowp[::3], pool()[:2000], topp[::2]]))
    allp = np.unique(allp)
    sets = [(allp, ones(allp)), (lowp[:1500], ones(lowp[:1500])), (lowp[:0], ones(lowp[:0])), (topp[:1700], ones(topp[:1700]))]
    want = check_all(gpu_ctx, torch, sets, False)
    assert want[0, 1] == 500 and want[0, 3] == 850 and want[1, 3] == 0 and (want[2] == 0).all()


CHUNK_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 7)


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_a_slice_below_at_and_above_the_chunk_on_either_side(gpu_ctx, torch, monkeypatch, weighted):
    """p = 0: every set is one slice.  The square puts every size on the row side, on the column side and on both"""
    monkeypatch.setenv("D2G_KSET_PBITS", "0")
    rng = np.random.default_rng(4400)
    p = pool()[:2 * CHUNK + 300]
    sets = []
    for m in CHUNK_SIZES:
        k = np.sort(rng.choice(p, m, replace=False))
        sets.append((k, rng.integers(1, 5, m).astype(np.uint32)))
    want = check_all(gpu_ctx, torch, sets, weighted)
    assert (want[:5, :5] > 300).all()


def test_equal_keys_on_both_sides_of_a_chunk_boundary(gpu_ctx, torch, monkeypatch):
    """the column set's entries 1023 and 1024 are the last of one chunk and the first of the next; the row sets hold exactly those"""
    monkeypatch.setenv("D2G_KSET_PBITS", "0")
    p = pool()[:3 * CHUNK]
    sets = [p, p[CHUNK - 1:CHUNK + 1], p[CHUNK - 5:CHUNK + 5], p[CHUNK:CHUNK + 1], p[CHUNK - 1:CHUNK], p[2 * CHUNK - 1:2 * CHUNK + 1]]
    want = check_all(gpu_ctx, torch, [(s, ones(s)) for s in sets], False)
    assert want[0].tolist() == [3 * CHUNK, 2, 10, 1, 1, 2] and want[1, 2] == 2 and want[3, 4] == 0


def test_sets_whose_sizes_differ_a_thousand_fold(gpu_ctx, torch):
    p = pool()
    small = p[::1000][:20]
    sets = [(p[:20000], ones(p[:20000])), (small, ones(small)), (p[19990:20010], ones(p[19990:20010]))]
    ks = make(gpu_ctx, sets, False)
    assert ks.slice_bits >= 5                                             # 20 000 keys: slices of at most 512 on average
    ks.close()
    want = check_all(gpu_ctx, torch, sets, False)
    assert want[0, 1] == 20 and want[0, 2] == 10 and want[1, 2] == 0


# ---------------------------------------------------------------- weights
def test_min_on_either_side_and_sums_beyond_32_bits(gpu_ctx, torch):
    p = pool()[:3000]
    a = np.where(np.arange(3000) % 2 == 0, U32MAX, 1).astype(np.uint32)
    b = np.where(np.arange(3000) % 3 == 0, U32MAX - 1, 2).astype(np.uint32)
    full = np.full(3000, U32MAX, np.uint32)
    sets = [(p, a), (p, b), (p, full)]
    want = np.zeros((3, 3), np.uint64)
    for i, (_, x) in enumerate(sets):
        for j, (_, y) in enumerate(sets):
            want[i, j] = int(np.minimum(x.astype(object), y.astype(object)).sum())
    assert int(want[0, 1]) == 500 * (U32MAX - 1) + 1000 * 2 + 1500 * 1 and int(want[2, 2]) == 3000 * U32MAX > 2 ** 43
    check_all(gpu_ctx, torch, sets, True, want)


# ---------------------------------------------------------------- the two routes
@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_split_and_one_workgroup_routes_agree(gpu_ctx, torch, monkeypatch, weighted):
    monkeypatch.setenv("D2G_KSET_PBITS", "4")
    sets = family(TW + 2, seed=4500, lo=200, hi=1500)
    got = {}
    for split in ("1", "2", "7", "16", None):
        if split is None:
            monkeypatch.delenv("D2G_KSET_SPLIT")
        else:
            monkeypatch.setenv("D2G_KSET_SPLIT", split)
        got[split] = check_all(gpu_ctx, torch, sets, weighted)
    assert all(np.array_equal(got["1"], g) for g in got.values())


# ---------------------------------------------------------------- random sets, automatic geometry
@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_random_sets_against_the_reference(gpu_ctx, torch, weighted):
    rng = np.random.default_rng(4600)
    p = pool()
    sets = []
    for i in range(13):
        m = int(rng.choice([0, 1, 50, 700, 3000, 9000]))
        k = np.sort(rng.choice(p[:12000], m, replace=False))
        sets.append((k, rng.integers(1, 1000, m).astype(np.uint32)))
    want = check_all(gpu_ctx, torch, sets, weighted)
    assert want.max() > 1000


# ---------------------------------------------------------------- from the sketch side, device to device
def test_sets_from_the_sketch_side_stay_on_the_device(d2g, gpu_ctx, torch):
    """d2g_kmer_sets_dev -> d2g_kset_create_dev -> isz, against exact_ref over the seam cases' enumerator"""
    rng = np.random.default_rng(4700)
    base = C.random_bases(rng, 6000)
    b = C.Batch("family", 21, 16, True, 0, [[base], [base[:4000], base[:4000]], [base[2000:]], [], [C.random_bases(rng, 3000)]])
    sets = X.exact_sets(b)
    sp = d2g.SeqPack(b.k)
    for f in b.fastas():
        sp.add_fastx(f)
    pk, rs, rl, go = sp.arrays()
    n, cap = len(sets), sum(b.nkmers())
    plan = gpu_ctx.oph_plan(rs, rl, go, b.k)
    try:
        packed = torch.from_numpy(np.array(pk, np.uint8)).cuda()
        keys, cnts = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
        off, cards = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(2 * n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.kmer_sets_dev(plan, packed.data_ptr(), keys.data_ptr(), cnts.data_ptr(), cap, off.data_ptr(), cards.data_ptr(), canon=True)
        for weighted in (False, True):
            ks = gpu_ctx.kset_dev(keys.data_ptr(), cnts.data_ptr() if weighted else None, off.data_ptr(), n)
            try:
                want = X.isz_matrix(sets, weighted)
                np.testing.assert_array_equal(ut_of(gpu_ctx, torch, ks), X.ut(want))
                assert want[0, 1] == 3980 and want[0, 3] == 0
            finally:
                ks.close()
    finally:
        plan.close()
