"""K3 (d2g_k3_bmh.hip, the --multiset path) at its own seams: the inputs of k3_seam_cases.py, built by construction, against
expected values that no part of the product computed -- (key, count) sets from a pure-Python k-mer enumerator, registers and
total weights from the oracle's sequential heap algorithm over those keys.  Everything is compared bit for bit, registers as
uint64.  Every genome case checks the three entry points that share the bucketed LDS counting: d2g_kmer_distinct, d2g_kmer_count
(compact_elements applies the count threshold) and d2g_bmh_sketch (the main kernel applies it once more, as an integer).

The D2G_K3_* switches are set with monkeypatch.setenv: the session's context reads them again (conftest.py)."""
import numpy as np
import pytest

import k3_seam_cases as C

pytestmark = pytest.mark.gpu


def check_batch(gpu_ctx, d2g, batch, thresholds=None):
    sp = d2g.SeqPack(batch.k)
    for f in batch.fastas():
        sp.add_fastx(f)
    n = len(batch.genomes)
    assert [sp.nkmers(g) for g in range(n)] == batch.nkmers()
    nd = gpu_ctx.kmer_distinct_seqpack(sp, canon=batch.canon, xormask=batch.xormask)
    assert nd.tolist() == [keys.size for keys, _, _ in batch.counts()], f"{batch}: distinct keys per genome"
    for thr in thresholds or batch.thresholds:
        exp = batch.expected(thr)
        got = gpu_ctx.kmer_count_seqpack(sp, canon=batch.canon, xormask=batch.xormask, count_threshold=thr)
        sig, tw = gpu_ctx.bmh_sketch_seqpack(sp, batch.S, canon=batch.canon, xormask=batch.xormask, count_threshold=thr)
        assert len(got) == n and sig.shape == (n, batch.S)
        for g, (ek, ec, esig, etw) in enumerate(exp):
            what = f"{batch} genome {g} threshold {thr}"
            np.testing.assert_array_equal(got[g][0], ek, err_msg=what + " (keys)")
            np.testing.assert_array_equal(got[g][1], ec, err_msg=what + " (counts)")
            assert tw[g] == etw, what + " (total weight)"
            np.testing.assert_array_equal(sig[g].view(np.uint64), esig.view(np.uint64), err_msg=what + " (registers)")


def set_env(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


# ---------------------------------------------------------------- a. the all-ones key, generic path
GENERIC_SETTINGS = [
    {},
    {"D2G_K3_LIGHT": "0"},                                               # the heavy main kernel walks its survivors in place
    {"D2G_K3_GUESS_SCALE": "0.001"},                                     # failed guesses: the redo passes count the key again
    {"D2G_K3_ROUND_KEYS": "64"},                                         # many table rounds: `ones` is handed over once per round
    {"D2G_K3_SPLIT_MIN": "40", "D2G_K3_ROUND_KEYS": "200"},              # pre-split sub-ranges that still need rounds
    {"D2G_K3_BUCKET_KEYS": "16", "D2G_K3_L1BITS": "3"},                  # 2048 buckets, the key in the last one, behind k3_refine_kernel
    {"D2G_K3_GQ_SCALE": "0.05"},                                         # survivor regions overflow: the pass is repeated in the heavy form
]


def env_id(env):
    return ",".join(f"{k[7:]}={v}" for k, v in env.items()) or "defaults"


@pytest.mark.parametrize("env", GENERIC_SETTINGS, ids=env_id)
@pytest.mark.parametrize("which", ["backbone", "unit"])
def test_all_ones_key_generic(gpu_ctx, d2g, monkeypatch, which, env):
    """EMPTY = ~0 cannot live in the count table: count_round, insert_round, compact_elements and the table walk of the main kernel
    count it in `ones` and attach it again as an element.  The xormask makes it the key of a k-mer seen once / three times."""
    set_env(monkeypatch, env)
    check_batch(gpu_ctx, d2g, C.all_ones_generic(which))


@pytest.mark.parametrize("env", GENERIC_SETTINGS[:4], ids=env_id)
def test_all_ones_key_alone_in_its_genome(gpu_ctx, d2g, monkeypatch, env):
    """a genome whose only element is ~0 (count 180), one that holds it among 1272 others (count 10; threshold 9 leaves it alone),
    an empty genome"""
    set_env(monkeypatch, env)
    check_batch(gpu_ctx, d2g, C.all_ones_only())


# ---------------------------------------------------------------- b. the all-ones stored word, compact path
@pytest.mark.parametrize("env", [{}, {"D2G_K3_ROUND_KEYS": "64"}, {"D2G_K3_SPLIT_MIN": "100000"}], ids=env_id)
@pytest.mark.parametrize("k", [16, 17, 21])
def test_all_ones_stored_word_compact(gpu_ctx, d2g, monkeypatch, k, env):
    """D2G_K3_COMPACT=1 stores a k-mer's low 32 bits: 0xFFFFFFFF, the table's EMPTY, for every k-mer that ends in sixteen T --
    in several buckets at once when k > 16.  SPLIT_MIN=100000: without the sub-range split, so through the table rounds."""
    set_env(monkeypatch, {"D2G_K3_COMPACT": "1", **env})
    check_batch(gpu_ctx, d2g, C.all_ones_compact(k))


# ---------------------------------------------------------------- c. table rounds
@pytest.mark.parametrize("env", [{}, {"D2G_K3_LIGHT": "0"}], ids=env_id)
def test_table_rounds_at_their_size_seams(gpu_ctx, d2g, monkeypatch, env):
    """one bucket of nk distinct keys per genome, nk around every size at which the kernel changes its course: the unguarded
    insert up to K3_ROUND_KEYS, two rounds, the table size itself, four rounds, the once-more split (k3_seam_cases.table_rounds)"""
    set_env(monkeypatch, {**C.ROUND_ENV, **env})
    check_batch(gpu_ctx, d2g, C.table_round_genomes())


# ---------------------------------------------------------------- d. count threshold
@pytest.mark.parametrize("env", [{}, {"D2G_K3_LIGHT": "0"}, {"D2G_K3_COMPACT": "1"}], ids=env_id)
def test_count_threshold_both_implementations(gpu_ctx, d2g, monkeypatch, env):
    """`(double)cc > thr` in compact_elements (count mode) and `cc >= cmin` in the main kernel (sketch mode) must both be
    float64(count) > thr, for thresholds on, between, below and far above the counts 1 .. 4; with nothing left: no keys, total
    weight 0, every register +inf"""
    set_env(monkeypatch, env)
    check_batch(gpu_ctx, d2g, C.planted_counts())


# ---------------------------------------------------------------- e. counts at strip edges
@pytest.mark.parametrize("extra,env", [(None, {}), (None, {"D2G_K3_LIGHT": "0"}), ("big", {}), ("small", {})],
                         ids=["light", "LIGHT=0", "with_300kb", "heavy_by_the_hosts_rule"])
def test_counts_at_the_strip_edges(gpu_ctx, d2g, monkeypatch, extra, env):
    """an element of count c reaches top_count(c) of the 65 top-level strips, whose edges are the integers up to 16 and then
    powers of two: counts on, below and above them, in a first pass of either form"""
    set_env(monkeypatch, env)
    check_batch(gpu_ctx, d2g, C.strip_edge_counts(extra))


# ---------------------------------------------------------------- f. explicit weights at level edges
def check_weighted(gpu_ctx, sets):
    if sets.owners:
        sig, tw, own = gpu_ctx.bmh_from_weighted_ids(sets.ids, sets.weights, sets.off, sets.S)
        np.testing.assert_array_equal(own, sets.own, err_msg=f"{sets} (owners)")
    sig2, tw2 = gpu_ctx.bmh_from_weighted(sets.ids, sets.weights, sets.off, sets.S)
    if sets.owners:
        np.testing.assert_array_equal(sig.view(np.uint64), sig2.view(np.uint64))
        np.testing.assert_array_equal(tw, tw2)
    np.testing.assert_array_equal(tw2, sets.tw, err_msg=f"{sets} (total weights)")
    bad = np.flatnonzero((sig2.view(np.uint64) != sets.sig.view(np.uint64)).any(axis=1))
    assert bad.size == 0, f"{sets}: registers differ for sets {bad[:10]}, seam weights {C.level_weights()[0][bad[:10] % 203]}"


@pytest.mark.parametrize("S", [1, 2, 3, 64, 255])
def test_one_weight_per_set_at_every_level_edge(gpu_ctx, S):
    """the doubles below, at and above every edge of the top-level strips, 2^-200 ... 3e9: top_count's ceil and exponent
    arithmetic, block_hmax with fewer registers than a wavefront, mulhi(r, m) and a guess with ln m = 0 at S = 1"""
    check_weighted(gpu_ctx, C.weights_one_per_set(S))


def test_all_level_edge_weights_in_one_set(gpu_ctx):
    check_weighted(gpu_ctx, C.weights_one_set())


def test_level_edge_weights_behind_a_full_workgroup(gpu_ctx):
    """each seam weight as element 2050 of its set: the second workgroup's only element, against registers the first one fills"""
    check_weighted(gpu_ctx, C.weights_in_a_crowd())


def test_the_weight_above_two_to_the_53_is_refused(gpu_ctx, d2g):
    with pytest.raises(d2g.D2GError, match="2\\^53"):
        gpu_ctx.bmh_from_weighted(np.array([7], np.uint64), np.array([C.TOO_LARGE]), np.array([0, 1], np.uint64), 64)
