"""K1s on a GPU: the resident k-mer database of `dashing2 contain` (d2g_screen), its count walk and its per-reference sums, and the
CLI end to end.  Everything is compared exactly with contain_ref.py: the counters themselves (d2g_screen_key_counts) against the
per-key counts, (matches, matchsums) against the closed form, output bytes against its writers.  Small shapes at the seams: the
capacity doubling of the table, the all-zero and all-ones k-mers at k = 32, keys no walker can produce, the 64-k-mer chunk boundary,
every lane adding to one counter, sketch sizes around the wave width, rows that must not bleed."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import contain_ref as R
import k0_ref
import k3_seam_cases as C
import oph_kmers_ref as K
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
EMPTY_KEY = int(K.decode(np.array([K.M64], np.uint64))[0])              # the masked key of an empty register
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


def mask(raw, xormask=0):
    return k0_ref.wang64(np.asarray(raw, np.uint64) ^ np.uint64(xormask))


def pack(d2g, k, genomes):
    """genomes: lists of ACGT records (a genome may have none that holds a k-mer)"""
    sp = d2g.SeqPack(k)
    for g in genomes:
        sp.add_fastx(C.fasta(g) if g else b">empty\n\n")
    return sp


def screen_once(d2g, ctx, db, k, canon, xormask, genomes, rows=None, nrows=None):
    """one launch over `genomes` -> (Screen, sketcher) with the counters filled"""
    rows = list(range(len(genomes))) if rows is None else rows
    sc = ctx.screen(db, k, canon=canon, xormask=xormask, nrows=(max(rows) + 1 if nrows is None else nrows))
    sk = ctx.sketcher()
    sk.run_screen(pack(d2g, k, genomes), sc, rows, canon=canon)
    return sc, sk


def check_row(sc, row, db, records, k, canon, xormask):
    keys, counts, _ = C.key_counts(tuple(records), k, canon, xormask)
    ekeys, ecnt = R.key_counts_of_db(db, keys, counts)
    gkeys, gcnt = sc.key_counts(row)
    np.testing.assert_array_equal(gkeys, ekeys)
    np.testing.assert_array_equal(gcnt, ecnt)
    em, es = R.closed_form(db, keys, counts)
    m, s = sc.result(row, 1)
    np.testing.assert_array_equal(m[0], em)
    np.testing.assert_array_equal(s[0], es)
    return ecnt


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("D", [2047, 2048, 2049])
def test_table_on_both_sides_of_a_capacity_doubling(d2g, gpu_ctx, D):
    """k = 6, forward k-mers: D of the 4096 6-mers are keys and EVERY 6-mer is asked, so a probe starts at every home slot of the table
    (4096 slots up to 2048 keys, 8192 from 2049 on), the last slot and its wrap-around included"""
    rng = np.random.default_rng(D)
    raw = rng.permutation(4096)[:D].astype(np.uint64)
    db = mask(raw).reshape(1, D)
    every = ["".join(C.LETTERS[(x >> (2 * (5 - j))) & 3] for j in range(6)) for x in range(4096)]
    records = every + [C.random_bases(rng, 3000)]
    sc, sk = screen_once(d2g, gpu_ctx, db, 6, False, 0, [records])
    nd, tbytes, cbytes = sc.info()
    assert nd == D and tbytes == ((4096 if D <= 2048 else 8192) + 1) * 12 and cbytes == 4 * D
    cnt = check_row(sc, 0, db, records, 6, False, 0)
    held = set(raw.tolist())
    assert cnt.min() >= 1 and cnt.sum() == sum(1 for x in C.kmers_of(records, 6, False) if x in held)
    assert sc.fed(0) == 4096 + 2995
    sk.close(); sc.close()


@pytest.mark.parametrize("canon", [False, True])
@pytest.mark.parametrize("seed", [0, 7])
def test_all_zero_and_all_ones_kmers_at_k32(d2g, gpu_ctx, canon, seed):
    """every 64-bit value is a k-mer at k = 32: A x 32 is raw 0, forward T x 32 is raw all ones -- the value of a free slot, held behind
    the slots.  Under canon T x 32 is read as A x 32 and the all-ones key is never hit."""
    xm = K.wang64_int(seed) if seed else 0
    rng = np.random.default_rng(32 + seed)
    g = C.random_bases(rng, 200)
    some = np.array(C.kmers_of([g], 32, canon)[:20], np.uint64)
    raw = np.concatenate([np.array([0, K.M64], np.uint64), some])
    db = mask(raw, xm).reshape(2, 11)
    records = ["A" * 40, "T" * 40, g, "T" * 32]
    sc, sk = screen_once(d2g, gpu_ctx, db, 32, canon, xm, [records])
    check_row(sc, 0, db, records, 32, canon, xm)
    keys, cnt = sc.key_counts(0)
    by_key = dict(zip(keys.tolist(), cnt.tolist()))
    assert by_key[int(mask([0], xm)[0])] == (9 + 10 if canon else 9)
    assert by_key[int(mask([K.M64], xm)[0])] == (0 if canon else 10)
    sk.close(); sc.close()


def test_keys_no_walker_can_produce_are_never_hit(d2g, gpu_ctx):
    """k = 31 under canon: a key whose raw form is >= 4^31, the all-ones raw key, and the NON-canonical form of a k-mer the query holds"""
    rng = np.random.default_rng(31)
    g = C.random_bases(rng, 300)
    fwd = C.kmers_of([g], 31, False)
    can = C.kmers_of([g], 31, True)
    noncanon = next(f for f, c in zip(fwd, can) if f != c)
    raw = np.array([(1 << 62) | can[0], 1 << 63, K.M64, noncanon, can[5], can[6]], np.uint64)
    db = mask(raw).reshape(1, 6)
    sc, sk = screen_once(d2g, gpu_ctx, db, 31, True, 0, [[g]])
    check_row(sc, 0, db, [g], 31, True, 0)
    keys, cnt = sc.key_counts(0)
    by_key = dict(zip(keys.tolist(), cnt.tolist()))
    assert [by_key[int(x)] for x in mask(raw)] == [0, 0, 0, 0, 1, 1]
    m, s = sc.result()
    assert m.tolist() == [[2]] and s.tolist() == [[2]]
    sk.close(); sc.close()


# ---------------------------------------------------------------- the walker
@pytest.fixture(scope="module")
def family():
    """k = 21, canon: a 4000-base genome, its distinct masked k-mers, and a database of three references sketched from it (S = 64)"""
    rng = np.random.default_rng(2121)
    g = C.random_bases(rng, 4000)
    refs = [[g[:2500]], [g[1500:]], [C.random_bases(rng, 2000)]]
    regs = np.stack([K.genome_closed_form(r, 21, True, 0, 64)[0] for r in refs])
    return g, K.decode(regs[:, :64]), rng


def test_runs_around_the_64_kmer_chunk_and_150_base_reads(d2g, gpu_ctx, family):
    g, db, _ = family
    k = 21
    rng = np.random.default_rng(5)
    records = [g[100:100 + k], g[200:200 + k + 63], g[300:300 + k + 64], g[500:500 + k + 65], g[:k - 1]]
    for _ in range(120):                                               # 150-base reads, some on the reverse strand
        p = int(rng.integers(0, len(g) - 150))
        r = g[p:p + 150]
        records.append(r if rng.integers(0, 2) else r[::-1].translate(str.maketrans("ACGT", "TGCA")))
    sc, sk = screen_once(d2g, gpu_ctx, db, k, True, 0, [records])
    cnt = check_row(sc, 0, db, records, k, True, 0)
    assert cnt.max() >= 3 and (cnt == 0).any()
    assert sc.fed(0) == 1 + 64 + 65 + 66 + 120 * 130
    sk.close(); sc.close()


def test_every_lane_adds_to_one_counter(d2g, gpu_ctx):
    """a 5000-base poly-A query against a database that holds A x k: the count is exactly 5000 - k + 1"""
    k = 21
    db = mask(np.array([0, 12345, 99], np.uint64)).reshape(1, 3)       # A x 21 is canonical (its reverse complement is T x 21)
    sc, sk = screen_once(d2g, gpu_ctx, db, k, True, 0, [["A" * 5000]])
    keys, cnt = sc.key_counts(0)
    assert dict(zip(keys.tolist(), cnt.tolist()))[int(mask([0])[0])] == 5000 - k + 1 and cnt.sum() == 5000 - k + 1
    m, s = sc.result()
    assert m.tolist() == [[1]] and s.tolist() == [[5000 - k + 1]]
    sk.close(); sc.close()


# ---------------------------------------------------------------- the reduction
@pytest.fixture(scope="module")
def pool(family):
    """the query of the reduction tests (the family genome twice over a stretch: counts of 1 and 2) and keys to draw databases from"""
    g, _, _ = family
    records = [g, g[1000:1800]]
    keys, counts, _ = C.key_counts(tuple(records), 21, True, 0)
    rng = np.random.default_rng(99)
    strangers = rng.integers(0, 1 << 63, 4000, dtype=np.int64).astype(np.uint64) | np.uint64(1 << 63)
    return records, keys, counts, strangers


@pytest.mark.parametrize("nrefs", [0, 1, 65])
@pytest.mark.parametrize("S", [1, 10, 63, 64, 65, 1000, 1024])
def test_reduction_shapes(d2g, gpu_ctx, pool, S, nrefs):
    """any S >= 1 and any number of references: keys of the query, keys of nobody, the empty register's key repeated inside one reference
    and across references (a reference shorter than S k-mers), the same k-mer in several references"""
    records, keys, counts, strangers = pool
    rng = np.random.default_rng(1000 * S + nrefs)
    db = np.empty((nrefs, S), np.uint64)
    shared = np.concatenate([keys[counts == 2][:1], keys[rng.integers(0, keys.size, 2)]])   # the first: a k-mer the query holds twice
    for r in range(nrefs):
        row = np.where(rng.random(S) < 0.5, keys[rng.integers(0, keys.size, S)], strangers[rng.integers(0, strangers.size, S)])
        if r % 5 == 0:
            row[S // 3:] = EMPTY_KEY                                    # a short reference: empty registers
        row[:min(S, 3)] = shared[:min(S, 3)]                            # the same k-mers in every reference
        db[r] = row
    sc = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=2)
    sk = gpu_ctx.sketcher()
    sk.run_screen(pack(d2g, 21, [records]), sc, [1], canon=True)
    assert sc.info()[0] == np.unique(db).size
    m, s = sc.result()
    em, es = R.closed_form(db, keys, counts)
    assert m.shape == (2, nrefs) and not m[0].any() and not s[0].any()
    np.testing.assert_array_equal(m[1], em)
    np.testing.assert_array_equal(s[1], es)
    if nrefs:
        assert em.min() >= 1 and (es > em).all()
    if S <= 65 and nrefs:                                              # the line-by-line restatement on the small ones
        rm, rs = R.restatement(db, [R.masked_stream(records, 21, True, 0)])
        np.testing.assert_array_equal(m[1], rm[0])
        np.testing.assert_array_equal(s[1], rs[0])
    sk.close(); sc.close()


# ---------------------------------------------------------------- rows
def test_three_queries_in_one_launch_do_not_bleed(d2g, gpu_ctx, family):
    g, db, rng = family
    contained, unrelated, nothing = [g[200:1200]], [C.random_bases(np.random.default_rng(77), 1500)], ["ACGTACGT"]
    sc, sk = screen_once(d2g, gpu_ctx, db, 21, True, 0, [contained, unrelated, nothing], nrows=4)
    check_row(sc, 0, db, contained, 21, True, 0)
    check_row(sc, 1, db, unrelated, 21, True, 0)
    m, s = sc.result()
    assert m[0].sum() > 0 and not m[1].any() and not m[2].any() and not m[3].any() and not s[1:].any()
    assert [sc.fed(r) for r in range(4)] == [980, 1480, 0, 0]
    # several genomes of one launch may share a row
    sc.reset()
    sk.run_screen(pack(d2g, 21, [contained, unrelated, [g[1100:1500]]]), sc, [2, 0, 2], canon=True)
    check_row(sc, 2, db, contained + [g[1100:1500]], 21, True, 0)
    check_row(sc, 0, db, unrelated, 21, True, 0)
    assert not sc.result()[0][1].any()
    sk.close(); sc.close()


def test_a_query_in_two_calls_equals_one_call_and_reset_zeroes(d2g, gpu_ctx, family):
    g, db, _ = family
    records = [g[0:900], g[400:1300], g[2000:2400], g[2100:2300]]
    one, sk = screen_once(d2g, gpu_ctx, db, 21, True, 0, [records])
    two = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=1)
    sk.run_screen(pack(d2g, 21, [records[:2]]), two, [0], canon=True)
    sk.run_screen(pack(d2g, 21, [records[2:]]), two, [0], canon=True)
    assert two.fed(0) == one.fed(0) == sum(len(r) - 20 for r in records)
    for a, b in zip(one.key_counts(0) + one.result(), two.key_counts(0) + two.result()):
        np.testing.assert_array_equal(a, b)
    assert one.key_counts(0)[1].max() >= 2
    two.reset()
    assert two.fed(0) == 0 and not two.key_counts(0)[1].any() and not two.result()[0].any() and not two.result()[1].any()
    sk.run_screen(pack(d2g, 21, [records]), two, [0], canon=True)       # and counts again from zero
    np.testing.assert_array_equal(two.key_counts(0)[1], one.key_counts(0)[1])
    sk.close(); one.close(); two.close()


def test_a_row_never_reaches_two_to_the_32_kmers(d2g, gpu_ctx, family):
    """the guard through the host-side tally alone: a faked count, a call that would take the row to 2^32 is refused before anything runs"""
    g, db, _ = family
    sc = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=2)
    sk = gpu_ctx.sketcher()
    sc.set_fed(1, (1 << 32) - 30)
    with pytest.raises(d2g.D2GError) as e:
        sk.run_screen(pack(d2g, 21, [[g[:50]], [g[:50]]]), sc, [0, 1], canon=True)      # 30 k-mers more: exactly 2^32
    assert e.value.status == ERR_UNSUPPORTED and "2^32" in str(e.value)
    assert sc.fed(0) == 0 and sc.fed(1) == (1 << 32) - 30 and not sc.key_counts(0)[1].any() and not sc.key_counts(1)[1].any()
    sk.run_screen(pack(d2g, 21, [[g[:50]], [g[:49]]]), sc, [0, 1], canon=True)          # 29 more: 2^32 - 1 is allowed
    assert sc.fed(0) == 30 and sc.fed(1) == (1 << 32) - 1
    with pytest.raises(d2g.D2GError) as e:
        sk.run_screen(pack(d2g, 21, [[g[:50]]]), sc, [2], canon=True)                   # a row the screen does not have
    assert e.value.status == ERR_INVALID
    sk.close(); sc.close()


def test_a_screen_of_another_k_or_canon_is_refused_before_anything_is_written(d2g, gpu_ctx, family):
    g, db, _ = family
    sc = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=1)
    sk = gpu_ctx.sketcher()
    for k, canon in ((22, True), (21, False)):
        with pytest.raises(d2g.D2GError) as e:
            sk.run_screen(pack(d2g, k, [[g[:500]]]), sc, [0], canon=canon)
        assert e.value.status == ERR_INVALID
    assert sc.fed(0) == 0 and not sc.key_counts(0)[1].any()
    sk.close(); sc.close()


def test_device_resident_form_and_device_parser_feed_the_same_counters(d2g, gpu_ctx, family):
    """d2g_screen_add_dev over a plan and a device stream, and d2g_sketcher_run_screen over a K0-ingested stream (packed == NULL)"""
    g, db, _ = family
    genomes = [[g[:700], g[650:900]], [g[3000:3300]]]
    want, sk = screen_once(d2g, gpu_ctx, db, 21, True, 0, genomes)
    sp = pack(d2g, 21, genomes)
    packed, rs, rl, go = sp.arrays()
    plan = gpu_ctx.oph_plan(rs, rl, go, 21)
    dptr = gpu_ctx.malloc(packed.size)
    gpu_ctx.h2d(dptr, packed)
    got = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=2)
    got.add_dev(plan, dptr, [0, 1])
    fasta = [C.fasta(x) for x in genomes]
    ing = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=2)
    runs = sk.ingest_fasta(fasta, 21)
    sk.run_screen_ingested(runs, ing, [0, 1], canon=True)
    for other in (got, ing):
        for row in (0, 1):
            np.testing.assert_array_equal(other.key_counts(row)[1], want.key_counts(row)[1])
        np.testing.assert_array_equal(other.result()[1], want.result()[1])
        assert [other.fed(0), other.fed(1)] == [want.fed(0), want.fed(1)]
    assert want.result()[0].sum() > 0
    gpu_ctx.free(dptr)
    plan.close(); sk.close(); want.close(); got.close(); ing.close()


def test_screen_kernels_are_timed(d2g, gpu_ctx, family):
    g, db, _ = family
    gpu_ctx.set_timing(d2g.TIME_SCREEN)
    try:
        sc, sk = screen_once(d2g, gpu_ctx, db, 21, True, 0, [[g[:500]]])
        sc.result()
        assert gpu_ctx.kernel_ms("screenbuild")[0] == 1 and gpu_ctx.kernel_ms("screen")[0] == 1 and gpu_ctx.kernel_ms("screenreduce")[0] == 1
        sk.close(); sc.close()
    finally:
        gpu_ctx.set_timing(False)


# ---------------------------------------------------------------- the CLI, end to end
def _run(args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    r = subprocess.run([EXE] + args, capture_output=True, timeout=120, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _fastq(records):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(records)).encode()


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """five related genomes, and three query files: FASTQ reads of genome 1 (one with an N), a gzipped FASTA of genome 3 with a
    stretch twice and an unrelated record, and a plain FASTA without any k-mer of the database"""
    d = tmp_path_factory.mktemp("contain_cli")
    rng = np.random.default_rng(64)
    base = C.random_bases(rng, 3000)
    genomes = []
    for i in range(5):
        s = list(base)
        for p in rng.integers(0, len(s), 40 * i):
            s[p] = C.LETTERS[(C.LETTERS.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        genomes.append(["".join(s)])
    paths = []
    for i, gnm in enumerate(genomes):
        p = d / f"g{i}.fa"
        p.write_bytes(C.fasta(gnm, f"g{i}"))
        paths.append(str(p))
    g1, g3 = genomes[1][0], genomes[3][0]
    reads = [g1[p:p + 150] for p in range(0, 2800, 37)]
    withn = g1[100:160] + "N" + g1[161:250]
    q1 = d / "reads.fq"
    q1.write_bytes(_fastq(reads + [withn]))
    rec1 = reads + [g1[100:160], g1[161:250]]                          # an N ends a run
    rec2 = [g3[:1200], g3[400:800], C.random_bases(rng, 500)]
    q2 = d / "reads2.fa.gz"
    q2.write_bytes(gzip.compress(C.fasta(rec2, "x")))
    rec3 = [C.random_bases(rng, 700), "ACGT"]
    q3 = d / "other.fa"
    q3.write_bytes(C.fasta(rec3, "o"))
    return d, paths, [str(q1), str(q2), str(q3)], [rec1, rec2, rec3]


@pytest.mark.parametrize("seed", [0, 7])
def test_cli_contain_end_to_end(cli_case, seed):
    d, paths, queries, recs = cli_case
    db = str(d / f"db{seed}")
    _run(["sketch", "-s", "-k", "21", "-S", "64", "-o", db] + (["--seed", str(seed)] if seed else []) + paths)
    raw = open(db + ".kmer64", "rb").read()
    hdr = np.frombuffer(raw[:16], np.uint32)
    assert hdr.tolist() == [1 << 8, 64, 21, 21] and int(np.frombuffer(raw[16:24], np.uint64)[0]) == seed
    keys = np.frombuffer(raw[24:], np.uint64).reshape(5, 64)
    xm = K.wang64_int(seed) if seed else 0                              # seed_mask(seed): the header's seed is what makes queries match
    text, binary = R.expected_outputs(keys, 64, paths, queries, recs, 21, True, xm)
    lines = text.decode().split("\n")
    assert lines[3].split("\t")[2].startswith("100%:") or float(lines[3].split("\t")[2].split("%")[0]) > 80      # reads of g1 cover g1
    assert all(e == "0%:0" for e in lines[5].split("\t")[1:])
    if seed:
        other = R.expected_outputs(keys, 64, paths, queries, recs, 21, True, 0)[0]
        assert other != text                                            # a query masked with another seed matches nothing
    out = str(d / f"out{seed}.txt")
    _run(["contain", "-o", out, db + ".kmer64"] + queries)
    assert open(out, "rb").read() == text
    r = _run(["contain", db + ".kmer64"] + queries)                      # stdout without -o
    assert r.stdout == text
    _run(["contain", "-b", "-o", out + ".bin", db + ".kmer64"] + queries)
    assert open(out + ".bin", "rb").read() == binary
    if seed:
        return
    lst = d / "queries.txt"
    lst.write_text("".join(q + "\n" for q in queries[:2]))
    r = _run(["contain", "-F", str(lst), db + ".kmer64", queries[2]])   # -F first, then the positionals
    assert r.stdout == text
    r = _run(["contain", db + ".kmer64"] + queries, env={"D2G_CONTAIN_ROWS": "2"})      # two groups of rows, a reset between
    assert r.stdout == text
    r = _run(["contain", db + ".kmer64"] + queries, env={"D2G_DEVICE_PARSE": "1"})      # other.fa through the device parser, and only it
    assert r.stdout == text and b"contain: 1 of 3 queries parsed on the device" in r.stderr
    r = _run(["contain", db + ".kmer64", queries[2]], env={"D2G_DEVICE_PARSE": "1"})
    assert r.stdout == R.expected_outputs(keys, 64, paths, queries[2:], recs[2:], 21, True, 0)[0]
    assert b"contain: 1 of 1 queries parsed on the device" in r.stderr
    r = _run(["contain", db + ".kmer64", queries[2]])
    assert b"parsed on the device" not in r.stderr
