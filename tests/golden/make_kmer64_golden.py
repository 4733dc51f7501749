#!/usr/bin/env python3
"""Generates tests/golden/kmer64_small.bin and kmer64_small.json.  RUNS ONLY IN THE BUILD CONTAINER (it imports the reference's
python/parse.py from /root/reference, which cannot travel).

kmer64_small.bin is a <out>.kmer64 file of three small genomes (k = 11, S = 5: m = 6, the last register of every sketch dropped),
laid out as src/fastxsketch.cpp:245-259,619-620 writes it: tests/oph_kmers_ref.py's writer fed with its closed form.
kmer64_small.json holds what the reference's own reader, python/parse.py:102-115 parse_binary_kmers, reads back from that file:
k, w, canon, alphabet, sketch size, seed, the shape of the k-mer matrix and its first row.  tests/test_oph_kmers_host.py checks
the writer against that JSON without importing the reference.

parse_binary_kmers subscripts the FUNCTION alphabetcvt (python/parse.py:112), which raises as written; the reader is run with that
one name bound to an object that can be subscripted and gives alphabetcvt's own answer."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/python/parse.py"

K, S, W, CANON, SEED = 11, 5, 11, True, 0
GENOME_SEED, GENOME_LENS = 20261018, (40, 300, 11)


def genomes():
    import k3_seam_cases as C
    rng = np.random.default_rng(GENOME_SEED)
    return [[C.random_bases(rng, n)] for n in GENOME_LENS]


def load_ref():
    spec = importlib.util.spec_from_file_location("d2_parse_ref", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fn = mod.alphabetcvt

    class Subscriptable:
        def __getitem__(self, x):
            return fn(int(x))
        __call__ = __getitem__
    mod.alphabetcvt = Subscriptable()
    return mod


def main():
    import oph_kmers_ref as R
    ref = load_ref()
    exp = R.expected_files(["g%d.fa" % i for i in range(len(GENOME_LENS))], genomes(), S, K, W, CANON, SEED)
    path = os.path.join(HERE, "kmer64_small.bin")
    with open(path, "wb") as f:
        f.write(exp["kmer64"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)               # int() of a one-element array (python/parse.py:113)
        p = ref.parse_binary_kmers(path)
    out = {"k": int(p.k), "w": int(p.w), "canon": bool(p.canon), "alphabet": str(p.alphabet), "sketchsize": int(p.sketchsize),
           "seed": int(p.seed), "shape": [int(x) for x in p.kmers.shape], "first_row": [int(x) for x in p.kmers[0]]}
    with open(os.path.join(HERE, "kmer64_small.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
