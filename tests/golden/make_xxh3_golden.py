"""Writes tests/golden/xxh3_names.json: XXH3_64bits (seed 0) digests recorded from the `xxhash` Python module (3.8.1), one entry per
line so that the C++ self-test reads the file without a JSON library.  Names: one of every length 0 .. 240 (printable bytes, no tab),
and 1 .. 22, X, Y, MT with and without chr / Chr."""
import json
import os
import random

import xxhash

rng = random.Random(20)
alphabet = bytes(range(0x21, 0x7f))
names = [bytes(rng.choice(alphabet) for _ in range(n)) for n in range(241)]
for c in [str(i) for i in range(1, 23)] + ["X", "Y", "MT"]:
    names += [c.encode(), b"chr" + c.encode(), b"Chr" + c.encode()]
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xxh3_names.json")
with open(out, "w") as f:
    f.write('{"source": "xxhash %s, xxh3_64_intdigest, seed 0", "entries": [\n' % xxhash.VERSION)
    for i, n in enumerate(names):
        f.write('  {"hex": "%s", "xxh3_64": "%d"}%s\n' % (n.hex(), xxhash.xxh3_64_intdigest(n), "," if i + 1 < len(names) else ""))
    f.write("]}\n")
json.load(open(out))
