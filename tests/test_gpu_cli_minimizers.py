"""`dashing2 sketch / cmp -w` (and what `contain` does with the header's w) end to end on a GPU, bytes against the model of tests/minimizer_ref.py: the inputs rewritten as one
k-base record per emission and handed to the UNCHANGED oracle (which knows no window), contain_ref.py and exact_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import contain_ref as CR
import exact_ref as X
import minimizer_ref as MR
import oph_kmers_ref as R
from conftest import ROOT
from dashing2_amd import synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K, W, S = 21, 30, 64


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    r = subprocess.run([EXE] + args, capture_output=True, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _stacked(N, S_, cards, sigs):
    return np.array([N, S_], np.uint64).tobytes() + np.asarray(cards, np.float64).tobytes() + np.asarray(sigs, np.float64).tobytes()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """four small inputs -- a genome, a mutated copy, one broken by Ns (a run shorter than w among them) with a second record, one whose
    only run is shorter than w -- and each rewritten under (k, w) = (21, 30)"""
    d = tmp_path_factory.mktemp("win_cli")
    g0 = synth.random_genome(700, 20000)
    g2 = bytearray(synth.random_genome(701, 5000).tobytes())
    g2[900:903] = b"NNN"
    g2[2000:2001] = b"N"
    g2[2000 + W - 1:2000 + W] = b"N"
    fastas = [synth.fasta_bytes("g0", g0), synth.fasta_bytes("g1", synth.mutate(g0, 0.01, 5)),
              b">g2\n" + bytes(g2) + b"\n>g2b\n" + g0[3000:3400].tobytes() + b"\n", b">tiny\n" + g0[:W - 1].tobytes() + b"\n"]
    paths, rpaths, rw = [], [], []
    for i, f in enumerate(fastas):
        p, q = d / f"g{i}.fa", d / f"g{i}.rewritten.fa"
        p.write_bytes(f)
        rw.append(MR.rewrite(f, K, W, True))
        q.write_bytes(rw[-1])
        paths.append(str(p))
        rpaths.append(str(q))
    return d, fastas, paths, rpaths, rw


def _cache_name(path, outprefix=None, w=W):
    plain = R.cache_name(path, S, K, outprefix=outprefix)
    return plain.replace(f".k{K}.", f".k{K}.w{w}.")


def test_sketch_stack_kmer_files_and_cache(oracle, case, tmp_path):
    d, fastas, paths, rpaths, rw = case
    out = tmp_path / "s.bin"
    _run(["sketch", "-k", str(K), "-w", str(W), "-S", str(S), "-N", "--cache", "--outprefix", str(tmp_path), "-o", str(out)] + paths)
    esigs, ecards = oracle.sketch_files(rpaths, k=K, S=S)
    assert out.read_bytes() == _stacked(4, S, ecards, esigs)
    regs = np.stack([oracle.sketch_buffer(b, k=K, S=S)[0] for b in rw])
    counts = np.stack([R.counts_for(*oracle.kmer_count_buffer(b, K, True)[:2], regs[i]) for i, b in enumerate(rw)])
    assert open(str(out) + ".kmer64", "rb").read() == R.kmer64_bytes(R.decode(regs[:, :S]), S, K, W, True, 0)          # the header's w
    assert open(str(out) + ".kmercounts.f64", "rb").read() == R.kmercounts_bytes(counts[:, :S], S) and counts[0].max() >= 2
    assert (regs[3] == R.M64).all()                                    # an input without a window: no k-mers
    names = open(str(out) + ".names.txt").read().splitlines()[1:]
    for i, p in enumerate(paths):
        cn = _cache_name(p, outprefix=str(tmp_path))
        assert f".k{K}.w{W}." in cn and names[i].split("\t")[0] == p and names[i].split("\t")[2] == cn[:cn.rfind(".")] + ".kmercounts.f64"
        blob = np.fromfile(cn, np.float64)
        assert blob[0] == ecards[i] and np.array_equal(blob[1:].view(np.uint64), esigs[i].view(np.uint64))
    assert not os.path.exists(R.cache_name(paths[0], S, K, outprefix=str(tmp_path)))        # never under the unwindowed name
    # the device FASTA parser feeds the same walker: identical bytes
    out2 = tmp_path / "s2.bin"
    _run(["sketch", "-k", str(K), "-w", str(W), "-S", str(S), "-N", "-o", str(out2)] + paths, env={"D2G_DEVICE_PARSE": "1"})
    for suffix in ("", ".kmer64", ".kmercounts.f64"):
        assert open(str(out2) + suffix, "rb").read() == open(str(out) + suffix, "rb").read()
    # w <= k is no window: the unwindowed bytes and names
    out3 = tmp_path / "s3.bin"
    _run(["sketch", "-k", str(K), "-w", str(K), "-S", str(S), "--cache", "--outprefix", str(tmp_path), "-o", str(out3)] + paths[:1])
    psig, pcard = oracle.sketch_files(paths[:1], k=K, S=S)
    assert out3.read_bytes() == _stacked(1, S, pcard, psig) and os.path.exists(R.cache_name(paths[0], S, K, outprefix=str(tmp_path)))


def test_sketch_multiset(oracle, case, tmp_path):
    d, fastas, paths, rpaths, rw = case
    out = tmp_path / "m.bin"
    _run(["sketch", "--multiset", "-k", str(K), "-w", str(W), "-S", str(S), "-o", str(out)] + paths)
    esigs, ecards, _ = oracle.bmh_sketch_files(rpaths, K, S)
    assert out.read_bytes() == _stacked(4, S, ecards, esigs) and ecards[3] == 0 and ecards[0] == 20000 - W + 1     # weights = window positions


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_sketch_set_files(oracle, case, tmp_path, weighted):
    d, fastas, paths, rpaths, rw = case
    pre = str(tmp_path)
    _run(["sketch", "--countdict" if weighted else "--set", "-k", str(K), "-w", str(W), "--outprefix", pre] + paths)
    for p, b in zip(paths, rw):
        keys, counts, _ = oracle.kmer_count_buffer(b, K, True)
        kf = X.makedest(p, K, outprefix=pre).replace(f".k{K}.", f".k{K}.w{W}.")
        assert open(kf, "rb").read() == X.key_file_bytes(keys, counts, weighted), kf
        if weighted and keys.size:                                      # (an input without k-mers has a key file and no count file, window or not)
            assert open(X.counts_path(kf), "rb").read() == X.count_file_bytes(counts)
    assert not os.path.exists(X.makedest(paths[0], K, outprefix=pre))


def test_sketch_parse_by_seq(oracle, case, tmp_path):
    d, fastas, paths, rpaths, rw = case
    multi = fastas[2] + fastas[3] + synth.fasta_bytes("head", synth.random_genome(700, 9000))
    fa, out = tmp_path / "multi.fa", tmp_path / "b.bin"
    fa.write_bytes(multi)
    _run(["sketch", "--parse-by-seq", "-k", str(K), "-w", str(W), "-S", str(S), "-o", str(out), str(fa)])
    sigs, cards, names = [], [], []
    for name, b in MR.rewrite_by_record(multi, K, W, True):
        _, sig, card, _ = oracle.sketch_buffer(b, k=K, S=S)
        card = 0.0 if card != card else card                           # fastxsketchbyseq.cpp:410-414
        if card < 10.0 * S:                                             # :415-430: the exact distinct count
            card = float(oracle.kmer_count_buffer(b, K, True)[0].size)
        sigs.append(sig), cards.append(card), names.append(name)
    assert names == ["g2", "g2b", "tiny", "head"] and cards[2] == 0 and 0 < cards[1] < 400 - W + 1
    assert out.read_bytes() == _stacked(4, S, cards, np.stack(sigs))


def test_sketch_filterset(oracle, case, tmp_path):
    """the filter file is enumerated with the same w: its minimizers are the set, and its size line counts its emissions"""
    d, fastas, paths, rpaths, rw = case
    g0 = fastas[0].split(b"\n", 1)[1].replace(b"\n", b"")
    ffa = b">slice\n" + g0[1000:6000] + b"\n>short\n" + g0[:W - 1] + b"\n"
    fp = tmp_path / "f.fa"
    fp.write_bytes(ffa)
    fem = MR.fasta_emissions(ffa, K, W, True, fast=True)
    fset = set(fem)
    frw = []
    for i, f in enumerate(fastas[:3]):
        q = tmp_path / f"g{i}.filtered.fa"
        q.write_bytes(MR.rewrite(f, K, W, True, keep=lambda v: v not in fset))
        frw.append(str(q))
    out = tmp_path / "f.bin"
    _run(["sketch", "--filterset", str(fp), "-k", str(K), "-w", str(W), "-S", str(S), "-o", str(out)] + paths[:3])
    esigs, ecards = oracle.sketch_files(frw, k=K, S=S)
    assert out.read_bytes() == _stacked(3, S, ecards, esigs)
    assert open(frw[0], "rb").read().count(b">") < rw[0].count(b">")
    r = _run(["cmp", "--filterset", str(fp), "-k", str(K), "-w", str(W), "-S", str(S)] + paths[:2])
    assert f";w:{W};" in r.stdout.decode() and f";canon;FilterSetSortedHashSet-size={len(fem)}\n" in r.stdout.decode() and len(fem) == 5000 - W + 1


def test_cmp_from_inputs(oracle, case, tmp_path):
    d, fastas, paths, rpaths, rw = case
    b = tmp_path / "d.bin"
    _run(["cmp", "-k", str(K), "-w", str(W), "-S", str(S), "--binary-output", "--cmpout", str(b)] + paths[:3])
    esigs, ecards = oracle.sketch_files(rpaths[:3], k=K, S=S)
    dens = np.stack([oracle.densify(s)[0] for s in esigs])
    exp = oracle.allpairs_ut(dens, ecards, measure=oracle.SIMILARITY, k=K)
    assert np.array_equal(np.fromfile(b, np.float32).view(np.uint32), exp.view(np.uint32)) and exp.max() > 0.3
    # cmp's default is no window
    b0 = tmp_path / "d0.bin"
    _run(["cmp", "-k", str(K), "-S", str(S), "--binary-output", "--cmpout", str(b0)] + paths[:3])
    psigs, pcards = oracle.sketch_files(paths[:3], k=K, S=S)
    pexp = oracle.allpairs_ut(np.stack([oracle.densify(s)[0] for s in psigs]), pcards, measure=oracle.SIMILARITY, k=K)
    assert np.array_equal(np.fromfile(b0, np.float32).view(np.uint32), pexp.view(np.uint32)) and not np.array_equal(pexp, exp)


def test_contain_refuses_a_windowed_database_and_takes_a_header_w_of_zero(case, tmp_path):
    """`sketch -s -w 30` writes w = 30 into the database header; `contain` still refuses such a database, by name, before it asks
    for a GPU.  A header w = 0 (hand-made here from an unwindowed database) screens every k-mer, as a header w = k does."""
    d, fastas, paths, rpaths, rw = case
    wdb = str(tmp_path / "wdb")
    _run(["sketch", "-s", "-k", str(K), "-w", str(W), "-S", str(S), "-o", wdb] + paths[:3])
    assert np.frombuffer(open(wdb + ".kmer64", "rb").read()[:16], np.uint32).tolist() == [1 << 8, S, K, W]
    r = subprocess.run([EXE, "contain", wdb + ".kmer64", paths[1]], capture_output=True)
    assert r.returncode == 1 and b"windowed minimizers (window 30, k 21)" in r.stderr and r.stdout == b""
    db = str(tmp_path / "db")
    _run(["sketch", "-s", "-k", str(K), "-S", str(S), "-o", db] + paths[:3])
    raw = bytearray(open(db + ".kmer64", "rb").read())
    assert np.frombuffer(bytes(raw[:16]), np.uint32).tolist() == [1 << 8, S, K, K]
    keys = np.frombuffer(bytes(raw[24:]), np.uint64).reshape(3, S)
    queries = [paths[1], paths[2], paths[3]]
    recs = [[r.decode() for _, seq in MR.records(fastas[i]) for r in MR.runs(seq)] for i in (1, 2, 3)]
    text, binary = CR.expected_outputs(keys, S, paths[:3], queries, recs, K, True, 0)
    assert text.decode().split("\n")[4].split("\t")[3].startswith("100%:")             # g2 holds every sampled k-mer of g2
    assert _run(["contain", db + ".kmer64"] + queries).stdout == text                    # header w = k
    raw[12:16] = np.array([0], np.uint32).tobytes()
    open(db + ".kmer64", "wb").write(raw)
    out = str(tmp_path / "out.txt")
    _run(["contain", "-o", out, db + ".kmer64"] + queries)
    assert open(out, "rb").read() == text
    _run(["contain", "-b", "-o", out + ".bin", db + ".kmer64"] + queries)
    assert open(out + ".bin", "rb").read() == binary
    r = _run(["contain", db + ".kmer64"] + queries, env={"D2G_DEVICE_PARSE": "1"})
    assert r.stdout == text
