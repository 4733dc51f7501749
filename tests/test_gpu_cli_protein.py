"""`dashing2 sketch|cmp --protein / --protein14 / --protein8 / --protein6` on a GPU: the files they write and what they compare, against
the model of tests/protein_ref.py plus the references that already turn (masked key, count) pairs and registers into outputs
(oph_mincount_ref, oph_kmers_ref, exact_ref, the oracle's finalisation and epilogue).  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import exact_ref as X
import oph_kmers_ref as R
import oph_mincount_ref as Q
import protein_ref as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")


def _run(args, env=None):
    e = dict(os.environ)
    for v in ("D2G_DEVICES", "D2G_DEVICE_PARSE", "D2G_HOST_PARSE"):
        e.pop(v, None)
    e.update(env or {})
    r = subprocess.run([EXE] + args, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _finalised(oracle, kc, S):
    """(masked key, count) pairs per input -> (signatures f64 [n][S], OPH cardinalities, registers) by the model's closed form and the
    oracle's x87 finalisation"""
    m = R.oph_m(S)
    regs = np.stack([Q.closed_form(k, c, m, 0)[0] for k, c in kc])
    fin = [oracle.regs_finalize(r) for r in regs]
    return np.stack([f[0][:S] for f in fin]), np.array([f[1] for f in fin]), regs


@pytest.fixture(scope="module")
def proteomes(tmp_path_factory):
    d = tmp_path_factory.mktemp("prot")
    base = bytearray(P.random_protein(40, 6000))
    seqs = [bytes(base)]
    rng = np.random.default_rng(41)
    for rate in (0.02, 0.2):
        b = bytearray(base)
        for i in np.flatnonzero(rng.random(len(b)) < rate):
            b[i] = ord(P.LETTERS20[int(rng.integers(0, 20))])
        seqs.append(bytes(b))
    seqs[1] = seqs[1][:2000] + b"XX" + seqs[1][2000:4000].lower() + b"*" + seqs[1][4000:]
    paths, fastas = [], []
    for i, s in enumerate(seqs):
        p = d / f"p{i}.fa"
        f = P.fa(s[:3000], f"p{i}a") + P.fa(s[3000:], f"p{i}b")
        p.write_bytes(f)
        paths.append(str(p)); fastas.append(f)
    return paths, fastas


def test_parse_by_seq_cmpout(oracle, tmp_path):
    """sketch --protein -k5 -S64 --parse-by-seq --cmpout on a 40-record file: names, stacked sketches (cardinality = the exact distinct
    count: every record is far below 10 S k-mers) and the distance matrix"""
    k, S, a = 5, 64, P.PROTEIN20
    rng = np.random.default_rng(5)
    base = P.random_protein(50, 400)
    recs = [P.fa(base, "base some comment"), P.fa(base[:200] + P.random_protein(51, 200), "half"), b">empty\n\n", P.fa(b"ACDE", "short"),
            P.fa(base[:100] + b"X" + base[100:].lower(), "broken")]
    for i in range(35):
        recs.append(P.fa(P.random_protein(600 + i, int(rng.integers(20, 400))), f"read{i}"))
    fa = tmp_path / "multi.fa"
    fa.write_bytes(b"".join(recs))
    out, dist = tmp_path / "bs.bin", tmp_path / "bs.dist"
    r = _run(["sketch", "--protein", "--parse-by-seq", "-k", str(k), "-S", str(S), "-o", str(out), "--cmpout", str(dist), "--binary-output", str(fa)])
    assert "Parsing 20-character amino acid sequences" in r.stderr
    kc = [P.fasta_counts(rec, k, a) for rec in recs]
    N = len(recs)
    esigs, _, _ = _finalised(oracle, kc, S)
    ecards = np.array([float(ek.size) for ek, _ in kc])
    assert N == 40 and ecards[2] == 0 and ecards[3] == 0 and ecards[0] == len(set(P.run_keys_brute(base, k, a)))
    raw = out.read_bytes()
    assert raw == np.array([N, S], np.uint64).tobytes() + ecards.tobytes() + esigs.tobytes()
    lines = open(str(out) + ".names.txt").read().splitlines()
    assert [l.split("\t")[0] for l in lines[1:]] == ["base", "half", "empty", "short", "broken"] + [f"read{i}" for i in range(35)]
    dens = np.stack([oracle.densify(s)[0] for s in esigs])
    want = oracle.allpairs_ut(dens, ecards, measure=oracle.SIMILARITY, k=k, nthreads=2)
    got = np.fromfile(dist, np.float32)
    assert got.size == N * (N - 1) // 2 and got.tobytes() == want.astype(np.float32).tobytes()
    assert got[0] > 0.2                                                # base and half share 200 residues


def test_save_kmers_and_counts(oracle, proteomes, tmp_path):
    """sketch --protein14 -s -N -o: the .kmer64 header word carries the alphabet id (4) and no canon bit, names, the third column"""
    paths, fastas = proteomes
    S, a = 64, P.PROTEIN_14
    k = P.max_k(a)                                                     # no -k: the alphabet's largest
    out = tmp_path / "st.bin"
    r = _run(["sketch", "--protein14", "-N", "-S", str(S), "-o", str(out)] + paths)
    assert "Parsing amino acid sequences with 14-letter compressed alphabet." in r.stderr
    kc = [P.fasta_counts(f, k, a) for f in fastas]
    esigs, ecards, regs = _finalised(oracle, kc, S)
    assert out.read_bytes() == np.array([len(paths), S], np.uint64).tobytes() + ecards.tobytes() + esigs.tobytes()
    counts = np.stack([R.counts_for(ek, ec, regs[i]) for i, (ek, ec) in enumerate(kc)])
    kmer64 = (tmp_path / "st.bin.kmer64").read_bytes()
    assert np.frombuffer(kmer64[:4], np.uint32)[0] == 4 and kmer64[:24] == P.kmer64_header(a, S, k)
    assert kmer64[24:] == R.decode(regs[:, :S]).tobytes()
    assert (tmp_path / "st.bin.kmer64.names.txt").read_bytes() == R.kmer64_names_bytes(paths)
    assert (tmp_path / "st.bin.kmercounts.f64").read_bytes() == R.kmercounts_bytes(counts[:, :S], S)
    lines = (tmp_path / "st.bin.names.txt").read_text().splitlines()
    assert [l.split("\t")[2] for l in lines[1:]] == [P.kmercounts_column(p, S, k, a) for p in paths]
    assert not any(".rc_canon" in l or ".DNA" in l for l in lines)
    # -C changes nothing, --filterset parses the filter file under the same alphabet: the first input's own k-mers vanish
    out2 = tmp_path / "st2.bin"
    _run(["sketch", "--protein14", "-C", "-S", str(S), "-o", str(out2), "--filterset", paths[0]] + paths)
    fkeys = kc[0][0]
    kept = [(ek[~np.isin(ek, fkeys)], ec[~np.isin(ek, fkeys)]) for ek, ec in kc]
    fsigs, fcards, _ = _finalised(oracle, kept, S)
    assert kept[0][0].size == 0 and 0 < kept[1][0].size < kc[1][0].size
    assert out2.read_bytes() == np.array([len(paths), S], np.uint64).tobytes() + fcards.tobytes() + fsigs.tobytes()


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_cmp_exact_sets_from_two_inputs(proteomes, tmp_path, weighted):
    """cmp --protein6 --set / --countdict from inputs: the key (and count) files under the new names, and the exact value"""
    paths, fastas = proteomes
    a, k = P.PROTEIN_6, 12
    two = paths[:2]
    out = tmp_path / "e.bin"
    pre = str(tmp_path)
    _run(["cmp", "--protein6", "--countdict" if weighted else "--set", "-k", str(k), "--outprefix", pre, "--binary-output", "--cmpout", str(out)] + two)
    sets = [P.fasta_counts(f, k, a) for f in fastas[:2]]
    iszm = X.isz_matrix(sets, weighted)
    cards = [X.card(ek, ec, weighted) for ek, ec in sets]
    want = X.measure_ut(iszm, cards, X.SIMILARITY, k)
    assert out.read_bytes() == np.asarray(want, np.float32).tobytes() and 0 < float(np.asarray(want)[0]) < 1
    for p, (ek, ec) in zip(two, sets):
        kf = os.path.join(pre, os.path.basename(P.set_name(p, k, a)))
        assert open(kf, "rb").read() == X.key_file_bytes(ek, ec, weighted)
        if weighted:
            assert open(X.counts_path(kf), "rb").read() == X.count_file_bytes(ec)
    assert not [f for f in os.listdir(pre) if ".DNA." in f or ".rc_canon" in f]


def test_cache_round_trip_under_the_new_names(oracle, proteomes, tmp_path):
    paths, fastas = proteomes
    S, k, a = 64, 8, P.PROTEIN_3BIT
    pre = str(tmp_path / "cache")
    os.mkdir(pre)
    first, second = tmp_path / "a.bin", tmp_path / "b.bin"
    _run(["sketch", "--protein8", "--cache", "-k", str(k), "-S", str(S), "--outprefix", pre, "-o", str(first)] + paths)
    kc = [P.fasta_counts(f, k, a) for f in fastas]
    esigs, ecards, _ = _finalised(oracle, kc, S)
    names = [P.cache_name(p, S, k, a, outprefix=pre) for p in paths]
    assert sorted(os.listdir(pre)) == sorted(os.path.basename(n) for n in names)
    for i, n in enumerate(names):
        assert open(n, "rb").read() == np.array([ecards[i]]).tobytes() + esigs[i].tobytes()
    # loaded, not sketched again: a cache file changed by hand shows in the second job's output
    marked = esigs[0].copy()
    marked[0] = 0.123
    with open(names[0], "wb") as f:
        f.write(np.array([7.0]).tobytes() + marked.tobytes())
    r = _run(["sketch", "--protein8", "--cache", "-k", str(k), "-S", str(S), "--outprefix", pre, "-o", str(second), "-v"] + paths)
    raw = second.read_bytes()
    assert raw[16:24] == np.array([7.0]).tobytes() and raw[16 + 8 * len(paths):][:8] == np.array([0.123]).tobytes()
    assert raw[24:16 + 8 * len(paths)] == ecards[1:].tobytes()


def test_device_parse_note(proteomes, tmp_path):
    """D2G_DEVICE_PARSE=1 is ignored with one stderr line and the host parser runs: the same bytes"""
    paths, _ = proteomes
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    _run(["sketch", "--protein", "-k", "5", "-S", "64", "-o", str(a)] + paths)
    r = _run(["sketch", "--protein", "-k", "5", "-S", "64", "-o", str(b)] + paths, env={"D2G_DEVICE_PARSE": "1"})
    assert r.stderr.count("D2G_DEVICE_PARSE ignored with PROTEIN20") == 1
    assert a.read_bytes() == b.read_bytes()
