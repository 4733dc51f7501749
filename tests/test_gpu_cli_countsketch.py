"""`dashing2 sketch / cmp --multiset -c <cells>` end to end on a GPU: the stacked file against the library and against BagMinHash of
the model's lists (tests/countsketch_ref.py), the cache name, cmp from inputs, the options line with its line feed, the device parser,
set space, --gpu-stats."""
import json
import os
import subprocess

import numpy as np
import pytest

import countsketch_ref as CS
from conftest import ROOT
from dashing2_amd import synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K, S, CELLS = 21, 64, 4096


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
    """a genome, a mutated copy, one broken by Ns with a second record, one without a k-mer"""
    d = tmp_path_factory.mktemp("cs_cli")
    g0 = synth.random_genome(900, 30000)
    g2 = bytearray(synth.random_genome(901, 5000).tobytes())
    g2[900:903] = b"NNN"
    g2[2000:2300] = b"A" * 300
    fastas = [synth.fasta_bytes("g0", g0), synth.fasta_bytes("g1", synth.mutate(g0, 0.01, 5)),
              b">g2\n" + bytes(g2) + b"\n>g2b\n" + g0[3000:3400].tobytes() + b"\n", b">tiny\n" + g0[:K - 1].tobytes() + b"\n"]
    paths = []
    for i, f in enumerate(fastas):
        p = d / f"g{i}.fa"
        p.write_bytes(f)
        paths.append(str(p))
    return d, fastas, paths


def _library(d2g, gpu_ctx, fastas, cells=CELLS, thr=0.0, seed=0):
    sp = d2g.SeqPack(K)
    for f in fastas:
        sp.add_fastx(f)
    return gpu_ctx.bmh_sketch_cs_seqpack(sp, S, cells, canon=True, xormask=d2g.seed_mask(seed), count_threshold=thr)


def test_sketch_stack_against_the_library_and_the_model(d2g, gpu_ctx, case, tmp_path):
    d, fastas, paths = case
    for flag in ("-c", "--countsketch-size", "--countmin-size"):
        out = tmp_path / "s.bin"
        _run(["sketch", "--multiset", flag, str(CELLS), "-k", str(K), "-S", str(S), "-o", str(out)] + paths)
        sig, tw = _library(d2g, gpu_ctx, fastas)
        assert out.read_bytes() == _stacked(4, S, tw, sig), flag
    kms = [CS.kmers_dna(f, K, True) for f in fastas]
    ids, w, off, tot = CS.batch_lists(kms, CELLS, d2g.seed_mask(0))
    esig, etw = gpu_ctx.bmh_from_weighted(ids, w, off, S)
    assert np.array_equal(tw, etw) and np.array_equal(sig.view(np.uint64), esig.view(np.uint64)) and tw[3] == 0 and tw[0] > 0
    # -m c keeps the cells with |count| >= c; --seed moves the cells
    for extra, thr, seed in ((["-m", "2"], 2.0, 0), (["-m", "1"], 1.0, 0), (["--seed", "7"], 0.0, 7)):
        out = tmp_path / "m.bin"
        _run(["sketch", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S), "-o", str(out)] + extra + paths)
        msig, mtw = _library(d2g, gpu_ctx, fastas, thr=thr, seed=seed)
        assert out.read_bytes() == _stacked(4, S, mtw, msig), extra
        e = CS.batch_lists(kms, CELLS, d2g.seed_mask(seed), thr)
        assert np.array_equal(mtw, e[3].astype(np.float64))
    assert not np.array_equal(mtw, tw)
    # -c 0 is the exact mode, bit for bit
    a, b = tmp_path / "e0.bin", tmp_path / "e1.bin"
    _run(["sketch", "--multiset", "-c", "0", "-k", str(K), "-S", str(S), "-o", str(a)] + paths)
    _run(["sketch", "--multiset", "-k", str(K), "-S", str(S), "-o", str(b)] + paths)
    assert a.read_bytes() == b.read_bytes() != (tmp_path / "s.bin").read_bytes()
    # the device FASTA parser feeds the same walker: identical bytes
    out2 = tmp_path / "s2.bin"
    _run(["sketch", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S), "-o", str(out2)] + paths, env={"D2G_DEVICE_PARSE": "1"})
    assert out2.read_bytes() == (tmp_path / "s.bin").read_bytes()


def test_cache_is_written_under_the_countmin_name_and_reloaded(d2g, gpu_ctx, case, tmp_path):
    d, fastas, paths = case
    pre = str(tmp_path)
    out = tmp_path / "c.bin"
    args = ["sketch", "--multiset", "--countmin-size", str(CELLS), "-k", str(K), "-S", str(S), "--cache", "--outprefix", pre, "-o", str(out)] + paths
    _run(args)
    sig, tw = _library(d2g, gpu_ctx, fastas)
    names = [os.path.join(pre, CS.cache_name(os.path.basename(p), S, K, CELLS)) for p in paths]
    assert names[0].endswith(f"g0.fa.rc_canon.sketchsize{S}.k{K}.CountMinCounting{CELLS}.MultisetSpace.DNA.d2gbmh")
    for i, cn in enumerate(names):
        blob = np.fromfile(cn, np.float64)
        assert blob[0] == tw[i] and np.array_equal(blob[1:].view(np.uint64), sig[i].view(np.uint64))
    assert not any(f.endswith(".ExactCounting.MultisetSpace.DNA.d2gbmh") for f in os.listdir(pre))
    first = out.read_bytes()
    # reloaded: a card changed in the cache file shows in the next run's stack
    blob = np.fromfile(names[1], np.float64)
    blob[0] = 12345.0
    blob.tofile(names[1])
    _run(args)
    cards = np.frombuffer(out.read_bytes()[16:16 + 32], np.float64)
    assert cards[1] == 12345.0 and cards[0] == tw[0] and out.read_bytes()[48:] == first[48:]


def _options_line(extra=""):
    return f"#Dashing2Options: Dashing2Options;k:{K};parsebyfile;trimchr;sketchsize:{S};sketchtype:{extra}"


def test_cmp_from_inputs_the_broken_header_and_presketched(case, tmp_path):
    d, fastas, paths = case
    stack = tmp_path / "s.bin"
    _run(["sketch", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S), "-o", str(stack)] + paths)
    for measure in ([], ["--mash-distance"], ["--containment"]):
        a, b = tmp_path / "a.bin", tmp_path / "b.bin"
        _run(["cmp", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S), "--binary-output", "--cmpout", str(a)] + measure + paths)
        _run(["cmp", "--presketched", "--multiset", "-k", str(K), "-S", str(S), "--binary-output", "--cmpout", str(b)] + measure + [str(stack)])
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) == 6 * 4, measure
    assert np.fromfile(tmp_path / "a.bin", np.float32).max() > 0
    # the TSV header: to_string() carries the line feed of d2.cpp:33, so the options line breaks after the cells
    text = _run(["cmp", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S)] + paths).stdout.decode()
    want = _options_line("bagminhash;Fastx") + CS.options_tail(CELLS) + ";canon\n#Sources\t"
    assert want in text and f";counting=countsketch{CELLS}\n;canon\n" in text, text[:600]
    assert text.splitlines()[1].endswith(f";counting=countsketch{CELLS}") and text.splitlines()[2] == ";canon"
    # --presketched ignores -c apart from that line
    p0 = _run(["cmp", "--presketched", "--multiset", "-k", str(K), "-S", str(S), str(stack)]).stdout.decode()
    p1 = _run(["cmp", "--presketched", "--multiset", "-c", "77", "-k", str(K), "-S", str(S), str(stack)]).stdout.decode()
    assert CS.options_tail(77) in p1 and p1.replace(CS.options_tail(77), "") == p0


def test_set_space_changes_only_the_options_line(case, tmp_path):
    d, fastas, paths = case
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    _run(["sketch", "-c", "100", "-k", str(K), "-S", str(S), "-o", str(a)] + paths)
    _run(["sketch", "-k", str(K), "-S", str(S), "-o", str(b)] + paths)
    assert a.read_bytes() == b.read_bytes()
    t1 = _run(["cmp", "-c", "100", "-k", str(K), "-S", str(S)] + paths).stdout.decode()
    t0 = _run(["cmp", "-k", str(K), "-S", str(S)] + paths).stdout.decode()
    assert CS.options_tail(100) in t1 and t1.replace(CS.options_tail(100), "") == t0
    # cache names of set sketches carry no counting type
    pre = tmp_path / "pre"
    pre.mkdir()
    _run(["sketch", "-c", "100", "-k", str(K), "-S", str(S), "--cache", "--outprefix", str(pre)] + paths[:1])
    assert os.listdir(pre) == [f"g0.fa.rc_canon.sketchsize{S}.k{K}.SetSpace.DNA.opss"]


def test_gpu_stats_has_the_new_keys(case, tmp_path):
    d, fastas, paths = case
    js = tmp_path / "stats.json"
    _run(["sketch", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S), "-o", str(tmp_path / "s.bin"), "--gpu-stats", str(js)] + paths)
    st = json.loads(js.read_text())
    dev = st["sketch"]["devices"][0]
    for name in ("k3k", "k3kcompact", "k3kbmh"):
        assert dev[name]["launches"] >= 1 and dev[name]["total_ms"] > 0, name
    cs = st["countsketch"]
    assert cs["cells"] == CELLS and cs["table_bytes"] == 3 * 4 * CELLS and cs["table_groups"] >= 1 and cs["batches"] >= 1
    assert "count-sketch" in st["sketch"]["space"] and dev["k3"]["launches"] == 0
    # in groups of genomes: one row at a time
    _run(["sketch", "--multiset", "-c", str(CELLS), "-k", str(K), "-S", str(S), "-o", str(tmp_path / "g.bin"), "--gpu-stats", str(js)] + paths,
         env={"D2G_CS_TABLE_BYTES": str(4 * CELLS)})
    st = json.loads(js.read_text())
    assert st["countsketch"]["table_bytes"] == 4 * CELLS and st["countsketch"]["table_groups"] == 3
    assert (tmp_path / "g.bin").read_bytes() == (tmp_path / "s.bin").read_bytes()
    # the exact mode reports none of them
    _run(["sketch", "--multiset", "-k", str(K), "-S", str(S), "-o", str(tmp_path / "e.bin"), "--gpu-stats", str(js)] + paths)
    st = json.loads(js.read_text())
    assert "countsketch" not in st and "k3k" not in st["sketch"]["devices"][0]
