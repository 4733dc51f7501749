"""The host side of amino-acid k-mers (K1a) without a GPU: the alphabet helpers, the byte-per-residue packer against the model of
tests/protein_ref.py, the packer / d2g_plan_check_tail / d2g_key_bits under ASan + UBSan as a stand-alone program, and the command
line up to the point where it asks for a GPU."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import protein_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(P.PROTEIN20, 1), (P.PROTEIN20, 5), (P.PROTEIN20, 14), (P.PROTEIN_14, 16), (P.PROTEIN_3BIT, 21), (P.PROTEIN_6, 24)]


def test_alphabet_helpers(d2g):
    for a in P.ALPHABETS:
        assert d2g.alphabet_size(a) == P.size(a) and d2g.alphabet_max_k(a) == P.max_k(a) and d2g.alphabet_name(a) == P.NAMES[a]
        t = P.code_table(a)
        assert [d2g.alphabet_code(a, b) for b in range(256)] == t.tolist()
        for k in range(1, P.max_k(a) + 1):
            assert d2g.key_bits(k, a) == P.key_bits(k, a)
        assert d2g.key_bits(P.max_k(a) + 1, a) == 0
    assert (d2g.alphabet_size(0), d2g.alphabet_max_k(0), d2g.alphabet_name(0)) == (4, 32, "DNA")
    assert [d2g.key_bits(k) for k in range(1, 33)] == [2 * k for k in range(1, 33)]
    assert d2g.alphabet_size(1) == 0 and d2g.alphabet_name(9) == ""
    assert (d2g.ALPHABET_PROTEIN20, d2g.ALPHABET_PROTEIN_3BIT, d2g.ALPHABET_PROTEIN_14, d2g.ALPHABET_PROTEIN_6) == (2, 3, 4, 5)


def _inputs(k):
    """lower case, every invalid letter, records shorter than k, an empty record, a record without a letter"""
    a, b, c, d = (P.random_protein(s, n) for s, n in ((1, 500), (2, 333), (3, 64 + k), (4, 3000)))
    broken = bytearray(b)
    for i, ch in enumerate(P.INVALID_LETTERS + P.INVALID_LETTERS.lower() + "19 ."):
        broken[7 + i * 13] = ord(ch)
    mixed = bytes(ch | 0x20 if i % 3 == 0 else ch for i, ch in enumerate(a))
    wrapped = b">w some words\n" + b"\n".join(d[i:i + 60] for i in range(0, len(d), 60)) + b"\n"
    return [P.fa(mixed, "mixed") + P.fa(bytes(broken), "broken"),
            P.fa(c[:k - 1], "short") + P.fa(c, "c") + b">empty\n\n" + P.fa(b"XXXX**--", "noletter") + P.fa(c[:k], "one"),
            wrapped,
            P.fa(b"", "nothing")]


def _same(sp, model):
    codes, rs, rl, go, nk = model
    packed, prs, prl, pgo = sp.arrays()
    assert packed.size == codes.size + 64 and sp.nbases == codes.size
    assert np.array_equal(packed[:codes.size], codes) and not packed[codes.size:].any()
    assert np.array_equal(prs, rs) and np.array_equal(prl, rl) and np.array_equal(pgo, go)
    assert [sp.nkmers(g) for g in range(len(nk))] == nk


@pytest.mark.parametrize("alphabet,k", CASES, ids=[f"A{P.size(a)}k{k}" for a, k in CASES])
def test_packer_agrees_with_the_model(d2g, alphabet, k, tmp_path):
    fastas = _inputs(k)
    model = P.stream(fastas, k, alphabet)
    assert model[4][3] == 0 and model[4][0] > 0 and len(model[1]) >= (25 if k <= 5 else 5)      # the broken record: runs of 12 residues, kept while k <= 12
    sp = d2g.SeqPack(k, alphabet)
    assert sp.alphabet == alphabet
    for f in fastas:
        sp.add_fastx(f)
    _same(sp, model)
    # per-genome totals are the model's k-mers
    assert [sp.nkmers(g) for g in range(4)] == [P.fasta_keys(f, k, alphabet).size for f in fastas]
    # by record: one genome per record, named by its header's first word
    by = d2g.SeqPack(k, alphabet)
    for f in fastas:
        by.add_fastx_by_record(f)
    _same(by, P.stream(fastas, k, alphabet, by_record=True))
    assert [by.name(g) for g in range(by.ngenomes)] == ["mixed", "broken", "short", "c", "empty", "noletter", "one", "w", "nothing"]
    # files, plain and .gz, and after clear() (the buffer keeps stale bytes behind the stream)
    paths = []
    for i, f in enumerate(fastas):
        p = tmp_path / (f"in{i}.fa.gz" if i % 2 else f"in{i}.fa")
        p.write_bytes(gzip.compress(f) if i % 2 else f)
        paths.append(str(p))
    sp.clear()
    for p in paths:
        sp.add_path(p)
    _same(sp, model)
    by.clear()
    for p in reversed(paths):
        by.add_path_by_record(p)
    _same(by, P.stream(fastas[::-1], k, alphabet, by_record=True))
    # a raw sequence
    sp.clear()
    raw = fastas[0].split(b"\n")[3]
    sp.add_sequence(raw)
    _same(sp, P.stream([P.fa(raw)], k, alphabet))


def test_packer_refuses_k_beyond_the_alphabet(d2g):
    for a in P.ALPHABETS:
        d2g.SeqPack(P.max_k(a), a).close()
        with pytest.raises(d2g.D2GError):
            d2g.SeqPack(P.max_k(a) + 1, a)
    with pytest.raises(d2g.D2GError):
        d2g.SeqPack(5, 1)
    d2g.SeqPack(32).close()                                                # the DNA form is what it was
    sp = d2g.SeqPack(5)
    sp.add_sequence(b"ACGTACGTNACGTAC")
    packed, rs, rl, go = sp.arrays()
    assert rl.tolist() == [8, 6] and packed.size == 4 + 64 and sp.alphabet == 0


def test_packer_plan_and_key_bits_under_the_sanitizers():
    csrc = os.path.join(ROOT, "dashing2_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "../bin/alphabet_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "dashing2_amd", "bin", "alphabet_selftest_asan")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "alphabet selftest OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


# ---------------------------------------------------------------- the command line, before a GPU is asked for
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "hot-path scope"
LINES = {"--protein": "Parsing 20-character amino acid sequences", "--protein20": "Parsing 20-character amino acid sequences",
         "--enable-protein": "Parsing 20-character amino acid sequences",
         "--protein14": "Parsing amino acid sequences with 14-letter compressed alphabet.",
         "--protein8": "Using 3-bit protein encoding", "--protein6": "Parsing amino acid sequences with 6-letter compressed alphabet."}


def _cli(cmd, *args, env=None):
    e = dict(os.environ)
    for v in ("D2G_DEVICES", "D2G_DEVICE_PARSE", "D2G_HOST_PARSE"):
        e.pop(v, None)
    e.update(env or {})
    return subprocess.run([EXE, cmd, *args], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def proteome(tmp_path_factory):
    p = tmp_path_factory.mktemp("prot_host") / "p.fa"
    p.write_bytes(P.fa(P.random_protein(8, 400)))
    return str(p)


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
@pytest.mark.parametrize("flag", sorted(P.FLAGS))
def test_cli_no_longer_refuses_the_protein_flags(tmp_path, proteome, cmd, flag):
    """past the option parser the job asks for a GPU: without one it ends there, with one it runs -- neither way is the flag out of
    scope; the reference's one stderr line is printed; k is the alphabet's largest when -k is absent"""
    r = _cli(cmd, flag, "-S", "64", "-o", str(tmp_path / "o.bin"), proteome)
    assert SCOPE not in r.stderr and LINES[flag] in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


def test_usage_mentions_the_protein_flags():
    r = _cli("sketch", "-h")
    for flag in P.FLAGS:
        assert flag in r.stderr, flag
    assert "PROTEIN_3BIT" in r.stderr and "k <= 14" in r.stderr and "k <= 24" in r.stderr


@pytest.mark.parametrize("args,env,words", [
    (["--protein", "-k", "15"], {}, ["k = 15 > 14", "PROTEIN20", "rolling-hash"]),
    (["--protein14", "-k", "17"], {}, ["k = 17 > 16", "PROTEIN_14"]),
    (["--protein8", "-k", "22"], {}, ["k = 22 > 21", "PROTEIN_3BIT"]),
    (["--protein6", "-k", "25"], {}, ["k = 25 > 24", "PROTEIN_6"]),
    (["--protein", "-k", "5", "-w", "9"], {}, ["-w 9 > -k 5", "DNA only"]),
    (["--protein6", "-w", "30"], {}, ["-w 30 > -k 24"]),
    (["--protein", "-k", "5"], {"D2G_DEVICES": "0,1"}, ["D2G_DEVICES naming several GPUs", "PROTEIN20"]),
    (["--protein", "-k", "5"], {"D2G_DEVICES": "all"}, ["D2G_DEVICES naming several GPUs"]),
], ids=["k15", "k17", "k22", "k25", "w9", "w30", "devices01", "devicesall"])
def test_cli_refuses_before_a_gpu_is_asked_for(tmp_path, proteome, args, env, words):
    r = _cli("sketch", *args, "-S", "64", "-o", str(tmp_path / "o.bin"), proteome, env=env)
    assert r.returncode == 1 and SCOPE in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr and not os.path.exists(tmp_path / "o.bin")


def test_cli_largest_k_and_a_window_at_k_pass_the_parser(tmp_path, proteome):
    for args in (["--protein", "-k", "14"], ["--protein8", "-k", "21"], ["--protein", "-k", "5", "-w", "5"], ["--protein6"]):
        r = _cli("sketch", *args, "-S", "64", "-o", str(tmp_path / "o.bin"), proteome)
        assert SCOPE not in r.stderr and (r.returncode == 0 or "gfx950" in r.stderr), r.stderr


def test_cli_device_parse_is_ignored_with_a_note(tmp_path, proteome):
    r = _cli("sketch", "--protein", "-k", "5", "-S", "64", "-o", str(tmp_path / "o.bin"), proteome, env={"D2G_DEVICE_PARSE": "1"})
    assert r.stderr.count("D2G_DEVICE_PARSE ignored with PROTEIN20") == 1 and SCOPE not in r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


def test_contain_still_refuses_a_protein_database(tmp_path, proteome):
    hdr = P.kmer64_header(P.PROTEIN20, 4, 5)
    db = tmp_path / "db.kmer64"
    db.write_bytes(hdr + np.arange(1, 9, dtype=np.uint64).tobytes())
    (tmp_path / "db.kmer64.names.txt").write_text("a\nb\n")
    r = _cli("contain", str(db), proteome)
    assert r.returncode != 0 and "gfx950" not in r.stderr


def test_file_names_of_the_model():
    """the names the GPU tests look for on disk (tests/test_gpu_cli_protein.py): the alphabet's name where DNA stands, no .rc_canon"""
    assert P.cache_name("d/p.fa", 64, 5, P.PROTEIN20) == "d/p.fa.sketchsize64.k5.SetSpace.PROTEIN20.opss"
    assert P.cache_name("d/p.fa x.fa", 64, 16, P.PROTEIN_14, seedseed=3, outprefix="o") == "o/p.fa.seed3.sketchsize64.k16.SetSpace.PROTEIN_14.opss"
    assert P.kmercounts_column("p.fa", 64, 21, P.PROTEIN_3BIT) == "p.fa.sketchsize64.k21.SetSpace.PROTEIN_3BIT.kmercounts.f64"
    assert P.set_name("p.fa", 24, P.PROTEIN_6) == "p.fa.k24.FullMmerSet.PROTEIN_6.kmerset64"
    assert P.set_name("p.fa", 5, P.PROTEIN20, 2) == "p.fa.k5.ct_threshold2.FullMmerSet.PROTEIN20.kmerset64"
    assert P.kmer64_header(P.PROTEIN_14, 64, 16)[:4] == b"\x04\x00\x00\x00"
