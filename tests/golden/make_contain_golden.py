#!/usr/bin/env python3
"""Generates tests/golden/contain_fmt.txt with fmt itself (header-only, the copy bundled with torch: 12.1.0).  RUNS ONLY IN THE
BUILD CONTAINER: it compiles a small C++ program against torch's include directory.

`dashing2 contain` prints every table entry as fmt's "\\t{:0.6g}%:{}" of 100.f * coverage and depth (reference
src/contain_main.cpp:291-293).  The file pins both conversions over everything the table can hold for three sketch sizes:

    g <S> <m> <text>    text = fmt::format("{:0.6g}", 100.f * (float)((1.0 / S) * m))   for every m of 0 .. S, S in {10, 1000, 1024}
    i 0 <v> <text>      text = fmt::format("{}", (float)v)                               small integers as float: a depth

tests/test_contain_host.py holds the product's writer (through selftest/contain_selftest.cpp) and contain_ref.py's to this file."""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (10, 1000, 1024)
INTS = list(range(0, 513)) + [999, 1000, 1023, 1024, 4095, 4096, 65535, 65536, 100000, 999999, 1000000, 9999999]

SRC = r"""
#include <fmt/format.h>
#include <cstdio>
int main() {
    const unsigned sizes[] = {%s};
    const unsigned ints[] = {%s};
    for (unsigned S : sizes) {
        const double ssiv = 1. / S;
        for (unsigned m = 0; m <= S; ++m) {
            const float cov = ssiv * m;
            std::printf("g %%u %%u %%s\n", S, m, fmt::format("{:0.6g}", 100.f * cov).c_str());
        }
    }
    for (unsigned v : ints) std::printf("i 0 %%u %%s\n", v, fmt::format("{}", float(v)).c_str());
    return 0;
}
"""


def main():
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "g.cpp"), os.path.join(d, "g")
        with open(src, "w") as f:
            f.write(SRC % (", ".join(map(str, SIZES)), ", ".join(map(str, INTS))))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DFMT_HEADER_ONLY", "-I" + inc, src, "-o", exe])
        out = subprocess.check_output([exe])
    with open(os.path.join(HERE, "contain_fmt.txt"), "wb") as f:
        f.write(out)
    print(len(out.splitlines()), "lines")


if __name__ == "__main__":
    sys.exit(main())
