"""`dashing2 sketch -m c` / `cmp -m c` in set space on a GPU: the files they write, byte for byte against d2g_oph_finalize and the
reference writers of oph_kmers_ref.py fed with the registers and counts of oph_mincount_ref.py (a pure-Python k-mer enumerator and the
closed form of LazyOnePermSetSketch under set_mincount; nothing the sketch path computed).  Three tiny inputs -- FASTA, FASTQ and
gzipped FASTA -- with k-mers seen once, twice and three times; -k 15 -S 63 (m = 64: the last register of every sketch is dropped)."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import k3_seam_cases as C
import oph_kmers_ref as R
import oph_mincount_ref as Q
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K, S = 15, 63


def _run(args, **kw):
    r = subprocess.run([EXE] + args, capture_output=True, timeout=120, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def fastq(records, name):
    return b"".join(b"@%s_%d\n%s\n+\n%s\n" % (name.encode(), i, r.encode(), b"I" * len(r)) for i, r in enumerate(records))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> (paths, batch, filter path, keys the filter removes): every genome has a part seen once, one seen twice and one seen three
    times (genomes 0 and 1 share theirs); the filter file is the twice-seen part of genome 0"""
    rng = np.random.default_rng(1901)
    genomes = []
    shared = C.random_bases(rng, 400)                                  # seen three times in genomes 0 and 1: what they have in common
    for n1, n2, n3 in ((700, 400, 0), (500, 350, 0), (90, 120, 60)):
        once, twice, thrice = (C.random_bases(rng, n) for n in (n1, n2, n3))
        thrice = thrice or shared
        genomes.append([thrice, once, twice, thrice, twice, thrice])
    d = tmp_path_factory.mktemp("mincount_fa")
    paths = [str(d / "g0.fa"), str(d / "g1.fq"), str(d / "g2.fa.gz")]
    open(paths[0], "wb").write(C.fasta(genomes[0], "g0"))
    open(paths[1], "wb").write(fastq(genomes[1], "g1"))
    with gzip.open(paths[2], "wb") as f:
        f.write(C.fasta(genomes[2], "g2"))
    fpath = str(d / "filter.fa")
    open(fpath, "wb").write(C.fasta([genomes[0][2]], "twice_of_g0"))
    drop = C.key_counts((genomes[0][2],), K, True, 0)[0]
    return paths, C.Batch("cli_mincount", K, S, True, 0, genomes), fpath, drop


def cache_name(path, c=None, outprefix=None):
    d = R.cache_name(path, S, K, outprefix=outprefix)
    return d if c is None else d.replace(".SetSpace", ".ct_threshold%d.SetSpace" % c)


def stacked_bytes(d2g, regs):
    sigs, cards = d2g.oph_finalize(np.array(regs), S)
    return np.array(regs.shape[:1] + (S,), np.uint64).tobytes() + cards.tobytes() + sigs.tobytes(), sigs, cards


def names_bytes(paths, cards, column=None):
    lines = ["#Name\tCardinality"] + [p + "\t%0.24g" % c + ("\t" + column[i] if column else "") for i, (p, c) in enumerate(zip(paths, cards))]
    return ("\n".join(lines) + "\n").encode()


def sketch(d, name, paths, *flags, cmd="sketch", env=None):
    out = d / name
    _run([cmd, "-k", str(K), "-S", str(S), "-o", str(out), "--gpu-stats", str(d / (name + ".json"))] + list(flags) + paths,
         env=dict(os.environ, **(env or {})))
    return out, json.loads((d / (name + ".json")).read_text())


def read(p):
    return open(str(p), "rb").read()


def test_the_inputs_bite(inputs):
    _, batch, _, drop = inputs
    r1, r2, r3, r4 = (Q.expected(batch, S, c)[0] for c in (1, 2, 3, 4))
    for g in range(3):
        assert len({r1[g].tobytes(), r2[g].tobytes(), r3[g].tobytes(), r4[g].tobytes()}) == 4 and (r4[g] == R.M64).all()
    assert not np.array_equal(Q.expected(batch, S, 2, drop=drop)[0][0], r2[0])


def test_sketch_m2_writes_the_sketch_of_what_occurs_twice(d2g, inputs, tmp_path):
    paths, batch, _, _ = inputs
    regs, _ = Q.expected(batch, S, 2)
    pre = str(tmp_path / "cache")
    os.mkdir(pre)
    out, st = sketch(tmp_path, "m2", paths, "-m", "2", "--cache", "--outprefix", pre)
    want, sigs, cards = stacked_bytes(d2g, regs)
    assert read(out) == want
    assert read(str(out) + ".names.txt") == names_bytes(paths, cards)
    assert sorted(os.listdir(pre)) == sorted(os.path.basename(cache_name(p, 2)) for p in paths)
    assert all(".ct_threshold2.SetSpace.DNA.opss" in n for n in os.listdir(pre))
    for i, p in enumerate(paths):
        assert read(cache_name(p, 2, pre)) == cards[i:i + 1].tobytes() + sigs[i].tobytes()
    dev = st["sketch"]["devices"][0]
    assert dev["k3"]["launches"] >= 1 and dev["k1"]["launches"] == 0 and "k1count" not in dev
    # the long spelling, and the caches read back
    out2, st2 = sketch(tmp_path, "m2_again", paths, "--count-threshold", "2", "--cache", "--outprefix", pre)
    assert read(out2) == want and st2["sketch"]["from_cache"] == 3
    # -m 3 is another sketch under another name
    out3, _ = sketch(tmp_path, "m3", paths, "-m", "3", "--cache", "--outprefix", pre)
    assert read(out3) == stacked_bytes(d2g, Q.expected(batch, S, 3)[0])[0] != want
    assert len(os.listdir(pre)) == 6


def test_save_kmercounts_with_m2(d2g, inputs, tmp_path):
    paths, batch, _, _ = inputs
    regs, cnts = Q.expected(batch, S, 2)
    out, st = sketch(tmp_path, "counted", paths, "-N", "-m", "2")
    assert read(out) == stacked_bytes(d2g, regs)[0]
    assert read(str(out) + ".kmer64") == R.kmer64_bytes(R.decode(regs[:, :S]), S, K, K, True, 0)
    assert read(str(out) + ".kmer64.names.txt") == R.kmer64_names_bytes(paths)
    assert read(str(out) + ".kmercounts.f64") == R.kmercounts_bytes(cnts[:, :S], S)
    assert set(np.unique(cnts).tolist()) == {0, 2, 3}
    column = [cache_name(p, 2)[:cache_name(p, 2).rfind(".")] + ".kmercounts.f64" for p in paths]
    assert read(str(out) + ".names.txt") == names_bytes(paths, stacked_bytes(d2g, regs)[2], column)
    dev = st["sketch"]["devices"][0]
    assert dev["k3"]["launches"] >= 1 and dev["k1count"]["launches"] >= 1 and dev["k1"]["launches"] == 0


def test_cmp_m2_phylip(d2g, oracle, inputs, tmp_path):
    from oracle import textfmt
    paths, batch, _, _ = inputs
    phy = tmp_path / "d.phylip"
    _run(["cmp", "-k", str(K), "-S", str(S), "-m", "2", "--phylip", "--cmpout", str(phy)] + paths)
    _, sigs, cards = stacked_bytes(d2g, Q.expected(batch, S, 2)[0])
    dens = np.stack([oracle.densify(s)[0] for s in sigs])
    dist = oracle.allpairs_ut(dens, cards, measure=oracle.SIMILARITY, k=K, nthreads=2)
    assert open(phy).read() == textfmt.render_symmetric(paths, dist, phylip=True)
    plain = tmp_path / "plain.phylip"
    _run(["cmp", "-k", str(K), "-S", str(S), "--phylip", "--cmpout", str(plain)] + paths)
    assert open(plain).read() != open(phy).read()


def test_filterset_composes(d2g, inputs, tmp_path):
    paths, batch, fpath, drop = inputs
    out, _ = sketch(tmp_path, "filtered", paths, "-m", "2", "--filterset", fpath)
    assert read(out) == stacked_bytes(d2g, Q.expected(batch, S, 2, drop=drop)[0])[0]


def test_the_device_parser_gives_the_same_bytes(d2g, inputs, tmp_path):
    paths, batch, _, _ = inputs
    regs, cnts = Q.expected(batch, S, 2)
    out, st = sketch(tmp_path, "devparse", paths, "-N", "-m", "2", env={"D2G_DEVICE_PARSE": "1", "D2G_GROUP_BYTES": "1"})
    assert st["sketch"]["groups_parsed_on_device"] >= 1
    assert read(out) == stacked_bytes(d2g, regs)[0]
    assert read(str(out) + ".kmercounts.f64") == R.kmercounts_bytes(cnts[:, :S], S)


def test_m1_is_the_plain_sketch_under_its_own_name(d2g, inputs, tmp_path):
    paths, batch, _, _ = inputs
    pre = str(tmp_path / "cache")
    os.mkdir(pre)
    out, st = sketch(tmp_path, "m1", paths, "-m", "1", "--cache", "--outprefix", pre)
    plain, _ = sketch(tmp_path, "plain", paths)
    assert read(out) == read(plain) == stacked_bytes(d2g, Q.expected(batch, S, 1)[0])[0]
    assert sorted(os.listdir(pre)) == sorted(os.path.basename(cache_name(p, 1)) for p in paths)
    dev = st["sketch"]["devices"][0]
    assert dev["k1"]["launches"] >= 1 and dev["k3"]["launches"] == 0


def test_parse_by_seq_with_m2_is_refused(inputs):
    paths, _, _, _ = inputs
    for cmd in ("sketch", "cmp"):
        r = subprocess.run([EXE, cmd, "--parse-by-seq", "-m", "2", "-k", str(K), paths[0]], capture_output=True, timeout=120)
        assert r.returncode == 2 and b"--parse-by-seq in set space" in r.stderr and b"whole inputs" in r.stderr


def test_what_was_refused_and_is_not_built_stays_refused(inputs, tmp_path):
    """a sketch job that writes nothing and `cmp --presketched` were refused with -m before there was a min-count sketch, and are still:
    the same exit status, a message that says why"""
    paths, _, _, _ = inputs
    for args, why in ((["sketch", "-m", "2", "-k", str(K)] + paths, b"writes nothing"),
                      (["cmp", "--presketched", "-m", "2", "-k", str(K), str(tmp_path / "none.bin")], b"--presketched")):
        r = subprocess.run([EXE] + args, capture_output=True, timeout=120)
        assert r.returncode == 1 and why in r.stderr and b"outside this build" in r.stderr


def test_multiset_m2_is_what_it_was(oracle, inputs, tmp_path):
    """--multiset keeps its own convention, count > c"""
    _, batch, _, _ = inputs
    paths = []
    for i, f in enumerate(batch.fastas()):
        paths.append(str(tmp_path / f"g{i}.fa"))
        open(paths[-1], "wb").write(f)
    out = tmp_path / "ms.bin"
    _run(["sketch", "--multiset", "-m", "2", "-k", str(K), "-S", "64", "-o", str(out)] + paths)
    esigs, ecards, _ = oracle.bmh_sketch_files(paths, K, 64, count_threshold=2.0)
    assert read(out) == np.array([3, 64], np.uint64).tobytes() + ecards.tobytes() + esigs.reshape(-1).tobytes()
    assert (ecards > 0).all()
