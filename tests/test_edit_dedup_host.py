"""The surface of greedy clustering by edit distance (K2j) without a GPU: the C ABI exports the new entry points, capi binds them and
carries the timer's constant, and null arguments are refused before any device is touched."""
import os
import re
import subprocess

from conftest import ROOT

NEW = ["d2g_edit_dedup_dev", "d2g_edit_dedup"]


def test_the_new_symbols_are_declared_exported_and_bound(d2g):
    header = open(os.path.join(ROOT, "include", "d2g.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", d2g.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    from dashing2_amd import capi
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in exported and s in capi.SIGNATURES and hasattr(d2g.lib(), s), s
    for m in ("dedup_dev", "dedup"):
        assert callable(getattr(d2g.SeqSet, m))


def test_the_timer_constant(d2g):
    header = open(os.path.join(ROOT, "include", "d2g.h")).read()
    assert int(re.search(r"#define\s+D2G_TIME_EDIT_DEDUP\s+(\d+)", header).group(1)) == d2g.TIME_EDIT_DEDUP == 2 * d2g.TIME_EDIT_NEAR == 8192


def test_null_arguments_are_refused_without_a_device(d2g):
    assert d2g.lib().d2g_edit_dedup_dev(None, None, 3, None, 0, None) == -1
    assert d2g.lib().d2g_edit_dedup(None, None, 3, 0, None) == -1
