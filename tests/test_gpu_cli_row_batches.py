"""The row batches of the exact (`cmp --set` / `--countdict`) and the edit-distance jobs are invisible: test_cli_cmp_batches_are_invisible
(test_gpu_cli.py) for the two jobs that now go through the slot queue as the register path does (host/row_batches.h).  Nine tiny inputs,
so a triangle has 36 values; every shape the job accepts, as text and as a binary matrix, with D2G_CMP_SLOT_VALUES unset, 1, 7 (not a
multiple of any row width here) and 36 (the whole triangle).  Every run of a shape gives the bytes of the unset run, and those are the
bytes the references of test_gpu_cli_exact.py / test_gpu_cli_edit.py give (exact_ref, edit_ref, oracle.textfmt).

A slot never holds less than the widest row, so D2G_CMP_SLOT_VALUES=1 means one slot per row of a rectangle (9 or 5 batches) and 8, 7,
6, 5, 4 + 3, 2 + 1 + 0 values for the triangle (6 batches): more batches than the three slots either way, so slots are reused."""
import json

import numpy as np
import pytest

import edit_ref as E
import exact_ref as X
import k3_seam_cases as C
from oracle import textfmt
from test_gpu_cli_edit import EDIT, OPTIONS
from test_gpu_cli_exact import K, _run, expected, fastq, opts_string

pytestmark = pytest.mark.gpu

SLOT_VALUES = (None, "1", "7", "36")
NSLOTS = 3
NREF = 5                                                                        # the panel: 5 references x 4 queries


def outputs_of(args, tmp_path, batches_of):
    """the --cmpout bytes of `args` under every slot size; all equal -> the bytes of the unset run"""
    outs = []
    for sv in SLOT_VALUES:
        out, st = tmp_path / "cmp.out", tmp_path / "stats.json"
        _run(args + ["--cmpout", str(out), "--gpu-stats", str(st)], env={} if sv is None else {"D2G_CMP_SLOT_VALUES": sv})
        outs.append(out.read_bytes())
        if sv == "1":
            assert batches_of(json.loads(st.read_text())["cmp"]) > NSLOTS, args
    for sv, o in zip(SLOT_VALUES, outs):
        assert o == outs[0], (args, sv)
    return outs[0]


# ---------------------------------------------------------------- --set / --countdict
@pytest.fixture(scope="module")
def nine_inputs(tmp_path_factory):
    """-> (paths, batch): nine inputs of 200 .. 700 bases that share stretches of two pools; one FASTQ, one with every record twice"""
    rng = np.random.default_rng(5300)
    base, other = C.random_bases(rng, 900), C.random_bases(rng, 600)
    genomes = [[base[:500]], [base[200:700], base[200:700]], [base[400:], other[:200]], [other], [other[100:500], base[:250]],
               [base[300:600]], [other[300:], base[600:800]], [base], [other[:300], other[:300], base[100:300]]]
    d = tmp_path_factory.mktemp("row_batches_fa")
    paths = [str(d / ("g%d.%s" % (i, "fq" if i == 4 else "fa"))) for i in range(9)]
    for i, (p, g) in enumerate(zip(paths, genomes)):
        open(p, "wb").write(fastq(g, "g%d" % i) if i == 4 else C.fasta(g, "g%d" % i))
    return paths, C.Batch("cli_row_batches", K, 16, True, 0, genomes)


@pytest.fixture(scope="module")
def exact_want(nine_inputs):
    """per weighted: (the condensed triangle, the full 9 x 9 matrix) of the containment, float32, from exact_ref"""
    _, batch = nine_inputs
    sets = X.exact_sets(batch)
    want = {}
    for weighted in (False, True):
        iszm, cards, vals = expected(sets, weighted, X.CONTAINMENT, None)
        full = np.array([[X.measure_value(int(iszm[i, j]), cards[i], cards[j], X.CONTAINMENT, K) for j in range(9)] for i in range(9)], np.float32)
        assert len(vals) == 36 and len({float(v) for v in vals}) > 12 and not np.array_equal(full, full.T)
        want[weighted] = (vals, full)
    assert not np.array_equal(want[False][1], want[True][1])
    return want


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
@pytest.mark.parametrize("shape", ["triangle", "phylip", "square", "panel"])
def test_exact_row_batches_are_invisible(nine_inputs, exact_want, tmp_path, shape, weighted):
    paths, _ = nine_inputs
    vals, full = exact_want[weighted]
    pre = tmp_path / "pre"
    pre.mkdir()
    opts = opts_string(weighted, outprefix=str(pre))
    q = tmp_path / "q.txt"
    q.write_text("\n".join(paths[NREF:]) + "\n")
    flags, inputs, text, binary = {
        "triangle": ([], paths, textfmt.render_symmetric(paths, vals, False, opts), vals.tobytes()),
        "phylip": (["--phylip"], paths, textfmt.render_symmetric(paths, vals, True), vals.tobytes()),
        "square": (["--square"], paths, textfmt.render_rect(paths, paths, full, "Asymmetric pairwise", opts), full.tobytes()),
        "panel": (["-Q", str(q)], paths[:NREF], textfmt.render_rect(paths, paths[:NREF], full[:NREF, NREF:], "Panel (Query/Refernce)", opts),
                  np.ascontiguousarray(full[:NREF, NREF:]).tobytes()),
    }[shape]
    common = ["cmp", "--countdict" if weighted else "--set", "-k", str(K), "--outprefix", str(pre), "--containment"] + flags
    assert outputs_of(common + inputs, tmp_path, lambda j: j["batches"]).decode() == text
    assert outputs_of(common + ["--binary-output"] + inputs, tmp_path, lambda j: j["batches"]) == binary


# ---------------------------------------------------------------- --edit-distance
@pytest.fixture(scope="module")
def nine_reads(tmp_path_factory):
    """a FASTA of nine records of 1 .. 70 symbols, mixed case and N -> (path, names, distance matrix by edit_ref)"""
    rng = np.random.default_rng(7500)
    alphabet = np.frombuffer(b"ACGTacgtN", np.uint8)
    base = bytes(rng.choice(alphabet[:4], 70).tolist())
    recs = []
    for n in (1, 9, 17, 26, 35, 44, 52, 61, 70):
        x = bytearray(base[:n])
        for _ in range(n // 8):
            x[int(rng.integers(n))] = int(rng.choice(alphabet))
        recs.append(bytes(x))
    order = rng.permutation(9)
    recs = [recs[i] for i in order]
    names = ["read%d" % i for i in range(9)]
    p = tmp_path_factory.mktemp("row_batches_edit") / "reads.fa"
    p.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), r) for n, r in zip(names, recs)))
    want = E.edit_matrix(recs)
    assert sorted(len(r) for r in recs) == [1, 9, 17, 26, 35, 44, 52, 61, 70] and len(set(E.triangle(want).tolist())) > 10
    return str(p), names, want


@pytest.mark.parametrize("shape", ["triangle", "phylip", "square"])                # a query panel is refused for this job (d2_options.cpp)
def test_edit_row_batches_are_invisible(nine_reads, tmp_path, shape):
    path, names, want = nine_reads
    tri, full = E.triangle(want).astype(np.float32), want.astype(np.float32)
    flags, text, binary = {
        "triangle": ([], textfmt.render_symmetric(names, tri, False, OPTIONS), tri.tobytes()),
        "phylip": (["--phylip"], textfmt.render_symmetric(names, tri, True), tri.tobytes()),
        "square": (["--square"], textfmt.render_rect(names, names, full, "Asymmetric pairwise", OPTIONS), full.tobytes()),
    }[shape]
    common = ["cmp"] + EDIT + flags
    assert outputs_of(common + [path], tmp_path, lambda j: j["edit"]["batches"]).decode() == text
    assert outputs_of(common + ["--binary-output", path], tmp_path, lambda j: j["edit"]["batches"]) == binary
