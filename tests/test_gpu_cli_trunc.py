"""`dashing2 cmp --presketched --fastcmp <1|2|4> [--bbit-sigs]` and `sketch -F/-Q --fastcmp ...` end to end: the binary output equals the
NumPy restatement of the reference's truncated-register path (tests/trunc_ref.py, computed live) applied to the same sketches, bit
for bit; the text outputs equal oracle.textfmt of those floats; --fastcmp 8 changes nothing; stderr carries the reference's
"Truncated via setsketch" line with the restatement's a and b."""
import os
import subprocess

import numpy as np
import pytest

import trunc_cases as TC
import trunc_ref as R
from conftest import ROOT
from dashing2_amd import synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K = 21
MEASURES = [([], R.SIMILARITY), (["--distance"], R.POISSON_LLR), (["--intersection"], R.INTERSECTION), (["--containment"], R.CONTAINMENT),
            (["--symmetric-containment"], R.SYMMETRIC_CONTAINMENT), (["--union-size"], R.UNION_SIZE)]


def _run(args, **kw):
    r = subprocess.run([EXE] + args, capture_output=True, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _ld_text(fmt, x):
    """printf("%0.20Lg") of a long double: through the C library, as the reference prints it"""
    import ctypes as C
    libc = C.CDLL(None)
    buf = C.create_string_buffer(128)
    libc.snprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_longdouble]
    raw = np.array([x], np.longdouble).tobytes()
    libc.snprintf(buf, 128, fmt.encode(), C.c_longdouble.from_buffer_copy(raw))
    return buf.value.decode()


@pytest.fixture(scope="module")
def stacked(tmp_path_factory, oracle):
    """a stacked sketch file of 300 un-densified OPH-shaped sketches (S = 100: not a power of two), families, unrelated and empty
    rows; -> (path, densified signatures, cardinalities)"""
    d = tmp_path_factory.mktemp("trunc")
    rng = np.random.default_rng(99)
    sigs, cards = TC.oph_shaped(rng, 300, 100, families=4, unrelated=12, empty_rows=2)
    sigs[rng.random(sigs.shape) < 0.03] = 0.0                 # empty buckets: cmp densifies them (cmp_core.cpp:686-718)
    path = d / "stack.bin"
    with open(path, "wb") as f:
        np.array(sigs.shape, np.uint64).tofile(f)
        cards.tofile(f)
        sigs.tofile(f)
    dens = np.stack([oracle.densify(s)[0] for s in sigs])
    assert not np.array_equal(dens, sigs)
    return str(path), dens, cards


@pytest.mark.parametrize("bbit", [False, True])
@pytest.mark.parametrize("regbytes", [1, 2, 4])
def test_cli_fastcmp_triangle_and_square(stacked, tmp_path, regbytes, bbit):
    from oracle import textfmt
    path, dens, cards = stacked
    N, S = dens.shape
    names = [str(i) for i in range(N)]
    opt = f"Dashing2Options;k:{K};parsebyfile;trimchr;sketchsize:{S};sketchtype:onepermsetsketch;Fastx;canon"
    trunc = ["--fastcmp", str(regbytes)] + (["--bbit-sigs"] if bbit else [])
    b = tmp_path / "o.bin"
    for flags, meas in MEASURES:
        exp, a, base = R.dist_ut(dens, cards, regbytes, bbit, meas, K)
        r = _run(["cmp", "--presketched", "-k", str(K), "--binary-output", "--cmpout", str(b)] + trunc + flags + [path])
        np.testing.assert_array_equal(np.fromfile(b, np.uint32), exp.view(np.uint32), err_msg=str(flags))
        err = r.stderr.decode()
        if bbit:
            assert "Truncated via setsketch" not in err
        else:
            line = "Truncated via setsketch, a = %s and b = %s from min, max regs " % (_ld_text("%0.20Lg", a), _ld_text("%0.24Lg", base))
            assert line in err, err[-600:]
    # text outputs of one measure, tiny row batches included; the aliases of the flag
    exp, _, _ = R.dist_ut(dens, cards, regbytes, bbit, R.CONTAINMENT, K)
    r = _run(["cmp", "--presketched", "-k", str(K), "--containment"] + trunc + [path])
    assert r.stdout.decode() == textfmt.render_symmetric(names, exp, phylip=False, options_string=opt)
    alias = ["--regsize" if regbytes == 2 else "--regbytes", str(regbytes)] + (["--bbit-sigs"] if bbit else [])
    r = _run(["cmp", "--presketched", "-k", str(K), "--containment", "--phylip"] + alias + [path], env=dict(os.environ, D2G_CMP_SLOT_VALUES="700"))
    assert r.stdout.decode() == textfmt.render_symmetric(names, exp, phylip=True)
    # --square: compare(i, j) for every ordered pair
    sq, _, _ = R.dist_rect(dens, cards, regbytes, bbit, R.CONTAINMENT, K, 0, N, 0, N)
    _run(["cmp", "--presketched", "-k", str(K), "--square", "--containment", "--binary-output", "--cmpout", str(b)] + trunc + [path])
    np.testing.assert_array_equal(np.fromfile(b, np.uint32), sq.reshape(-1).view(np.uint32))
    if regbytes == 2:
        r = _run(["cmp", "--presketched", "-k", str(K), "--square", "--containment"] + trunc + [path], env=dict(os.environ, D2G_CMP_SLOT_VALUES="1000"))
        assert r.stdout.decode() == textfmt.render_rect(names, names, sq, "Asymmetric pairwise", opt)


def test_cli_fastcmp_8_changes_nothing(stacked, tmp_path):
    path, _, _ = stacked
    outs = []
    for extra in ([], ["--fastcmp", "8"], ["--regbytes", "8", "--bbit-sigs"], ["--bbit-sigs"]):
        b = tmp_path / "o.bin"
        r = _run(["cmp", "--presketched", "-k", str(K), "--union-size", "--binary-output", "--cmpout", str(b)] + extra + [path])
        assert b"Truncated via setsketch" not in r.stderr
        outs.append(b.read_bytes())
    assert outs[1] == outs[0] and outs[2] == outs[0] and outs[3] == outs[0]
    r = _run(["cmp", "--presketched", "-k", str(K), "--union-size", "--fastcmp", "2", "--binary-output", "--cmpout", str(tmp_path / "t.bin"), path])
    assert (tmp_path / "t.bin").read_bytes() != outs[0]


@pytest.mark.parametrize("regbytes,bbit", [(1, False), (2, True), (4, False)])
def test_cli_fastcmp_panel_and_multiset(oracle, tmp_path, regbytes, bbit):
    """-F/-Q panel from FASTA (rows = references, columns = queries), and the same flags on --multiset sketches: the compressed branch
    ignores the sketch space.  Two devices asked for: one is used, and a note says so."""
    d = tmp_path / "fa"
    d.mkdir()
    base = synth.random_genome(5, 30000)
    paths = []
    for i, rate in enumerate([0.0, 0.002, 0.02, 0.1, 0.3]):
        p = d / f"g{i}.fa"
        synth.write_fasta(p, f"g{i}", synth.mutate(base, rate, seed=i) if rate else base)
        paths.append(str(p))
    for i in range(3):
        p = d / f"o{i}.fa"
        synth.write_fasta(p, f"o{i}", synth.random_genome(50 + i, 20000 + 5000 * i))
        paths.append(str(p))
    refs, qs = paths[:5], paths[5:] + paths[1:2]
    allp = refs + qs
    S = 96
    trunc = ["--fastcmp", str(regbytes)] + (["--bbit-sigs"] if bbit else [])
    ff, qf = tmp_path / "refs.txt", tmp_path / "qs.txt"
    ff.write_text("\n".join(refs) + "\n")
    qf.write_text("\n".join(qs) + "\n")
    esigs, ecards = oracle.sketch_files(allp, k=K, canon=True, xormask=oracle.load().d2o_seed_mask(0), S=S, nthreads=2)
    dens = np.stack([oracle.densify(s)[0] for s in esigs])
    nf = len(refs)
    b = tmp_path / "p.bin"
    for flags, meas in MEASURES[3:]:
        exp, _, _ = R.dist_rect(dens, ecards, regbytes, bbit, meas, K, 0, nf, nf, len(allp))
        r = _run(["sketch", "-k", str(K), "-S", str(S), "-F", str(ff), "-Q", str(qf), "--binary-output", "--cmpout", str(b)] + trunc + flags,
                 env=dict(os.environ, D2G_DEVICES="0,0"))
        np.testing.assert_array_equal(np.fromfile(b, np.uint32), exp.reshape(-1).view(np.uint32), err_msg=str(flags))
        assert b"D2G_DEVICES ignored for this job (truncated registers" in r.stderr
    # --multiset: BagMinHash registers, truncated and compared the same way
    st = tmp_path / "m.bin"
    _run(["sketch", "-k", str(K), "-S", str(S), "--multiset", "-o", str(st)] + allp)
    raw = np.fromfile(st, np.uint8)
    n = len(allp)
    mcards = raw[16:16 + 8 * n].view(np.float64)
    msigs = raw[16 + 8 * n:].view(np.float64).reshape(n, S)
    exp, _, _ = R.dist_ut(msigs, mcards, regbytes, bbit, R.INTERSECTION, K)
    _run(["sketch", "-k", str(K), "-S", str(S), "--multiset", "--intersection", "--binary-output", "--cmpout", str(b)] + trunc + allp)
    np.testing.assert_array_equal(np.fromfile(b, np.uint32), exp.view(np.uint32))


def test_cli_fastcmp_gpu_stats(stacked, tmp_path):
    import json
    path, dens, cards = stacked
    js = tmp_path / "s.json"
    _run(["cmp", "--presketched", "-k", str(K), "--fastcmp", "1", "--gpu-stats", str(js), "--binary-output", "--cmpout", str(tmp_path / "o.bin"), path])
    c = json.loads(js.read_text())["cmp"]
    _, a, b, _, _ = R.truncate(dens, 1, False)
    assert c["algo"] == "planes" and c["regbytes"] == 1 and c["truncation"] == "setsketch"
    assert c["a"] == float(a) and c["b"] == float(b)          # 21 significant digits in the file: the nearest double is the same
    _run(["cmp", "--presketched", "-k", str(K), "--fastcmp", "2", "--bbit-sigs", "--gpu-stats", str(js), "--binary-output", "--cmpout", str(tmp_path / "o.bin"), path])
    c = json.loads(js.read_text())["cmp"]
    assert c["algo"] == "planes" and c["regbytes"] == 2 and c["truncation"] == "bbit" and c["a"] is None and c["b"] is None
    _run(["cmp", "--presketched", "-k", str(K), "--gpu-stats", str(js), "--binary-output", "--cmpout", str(tmp_path / "o.bin"), path])
    c = json.loads(js.read_text())["cmp"]
    assert c["regbytes"] == 8 and c["truncation"] is None and c["algo"] == "direct"
