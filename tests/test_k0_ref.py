"""The model of K0 (k0_ref.py) against the host packer and the oracle, on every case of the seam catalogue (k0_seam_cases.py): the
rule the device parser is held to in test_gpu_k0_stream.py is the rule the host parser follows, base for base.  No GPU."""
import numpy as np
import pytest

import k0_ref
import k0_seam_cases as kc
from test_host import _decode_runs

KS = (1, 5, 31)
_parsed = {}


def parsed(case):
    if case.name not in _parsed:
        _parsed[case.name] = k0_ref.Parsed(case.files, case.genome_nfiles)
    return _parsed[case.name]


@pytest.mark.parametrize("group", kc.GROUPS + ("reuse",))
def test_model_equals_host_packer_and_oracle(d2g, oracle, group):
    cases = [c for c in kc.CASES + list(kc.REUSE) if c.group == group]
    assert cases
    for case in cases:
        m = parsed(case)
        assert m.refused == case.refused, case.name
        if case.refused:
            continue                                                   # FASTQ: the host parser skips quality lines by length
        for k in KS:
            sp = d2g.SeqPack(k)
            for f in case.files:
                sp.add_fastx(f)                                        # one host "genome" per file
            packed, rs, rl, go = sp.arrays()
            host = _decode_runs(packed, rs, rl)
            for fi, f in enumerate(case.files):
                what = f"{case.name} k={k} file {fi}"
                assert m.run_strings(fi, k) == host[int(go[fi]):int(go[fi + 1])], what
                nk = m.file_runs(fi, k)[1]
                assert nk == sp.nkmers(fi) == oracle.sketch_buffer(f, k=k, canon=True, S=8)[3], what
            # the model's own genome table: the files' runs in order, the files' k-mer counts added up
            mrs, mrl, mgo, mnk = m.run_table(k)
            np.testing.assert_array_equal(mrl, rl, err_msg=case.name)
            bounds = np.concatenate([[0], np.cumsum(m.genome_nfiles)])
            np.testing.assert_array_equal(mgo, go[bounds], err_msg=case.name)
            np.testing.assert_array_equal(mnk, [sum(sp.nkmers(fi) for fi in range(a, b)) for a, b in zip(bounds[:-1], bounds[1:])])
            assert ((mrs[1:] >= mrs[:-1] + mrl[:-1]).all() and (mrl >= k).all()) if mrs.size else True, case.name
            sp.close()


def test_catalogue_places_its_events_on_the_seams():
    """the decisive byte of every seam event is where the case's name says (seam_file asserts it while the catalogue is built); here:
    the catalogue is complete and small"""
    names = {c.name for c in kc.CASES}
    for ev in kc.EVENTS:
        for P in kc.SEAMS:
            assert {f"{ev}@{P}{d:+d}" for d in (-1, 0, 1)} <= names
        assert f"{ev}@{kc.ROUND}+0" in names
    size = {c.name: sum(len(f) for f in c.files) for c in kc.CASES}
    long = [n for n, b in size.items() if b > 3 * kc.TILE + 128]       # (an event AT 3 tiles ends a few bytes past them)
    assert all(size[n] >= kc.ROUND for n in long) and len(long) <= len(kc.EVENTS) + 16, long
    assert any(c.refused for c in kc.CASES) and sum(c.refused for c in kc.CASES) == len(kc.SEAMS) * 3 + 1


def test_split_of_long_runs_follows_the_host_packer(d2g, monkeypatch):
    monkeypatch.setenv("D2G_MAX_RUN", "64")
    f = kc.HEAD + kc.fill(5, 1000) + b"N" + kc.fill(6, 64) + b"N" + kc.fill(7, 65) + b"\n"
    m = k0_ref.Parsed([f])
    for k in (1, 5, 31, 32):
        sp = d2g.SeqPack(k)
        sp.add_fastx(f)
        _, rs, rl, go = sp.arrays()
        mrs, mrl, _, mnk = m.run_table(k, max_run=64)
        np.testing.assert_array_equal(mrl, rl)
        np.testing.assert_array_equal(np.diff(mrs.astype(np.int64)), np.diff(rs.astype(np.int64)))
        assert int(mnk[0]) == sp.nkmers(0)
        sp.close()


def test_wang64_restatement_equals_the_library(d2g):
    x = np.random.default_rng(3).integers(0, 1 << 64, 1000, dtype=np.uint64)
    x[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    np.testing.assert_array_equal(k0_ref.wang64(x), [d2g.wang_hash(int(v)) for v in x])


def test_window_tables_cover_every_base():
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 1000):
        s, W = k0_ref.window_starts(n)
        covered = np.zeros(n, bool)
        for a in s:
            covered[a:a + W] = True
        assert covered.all() and (n == 0 or (s + W <= n).all())
    codes = np.arange(70, dtype=np.uint8) & 3
    v = k0_ref.window_values(codes, [0, 3], 32)
    assert int(v[0]) == int("".join(str(int(c)) for c in codes[:32]), 4) and int(v[1]) == int("".join(str(int(c)) for c in codes[3:35]), 4)
    p = k0_ref.pack_codes(codes)
    assert p.size == 18 + 64 and p[0] == 0b11100100 and not p[18:].any()
