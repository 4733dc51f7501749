"""The surface of the bounded edit-distance routes (K2i) without a GPU: the C ABI exports the new entry points, capi binds them and
carries the constants, and the library reports the band bound the header states."""
import os
import re
import subprocess

from conftest import ROOT

NEW = ["d2g_edit_band_max", "d2g_edit_near_dev", "d2g_edit_within_dev", "d2g_edit_knn"]


def test_the_new_symbols_are_declared_exported_and_bound(d2g):
    header = open(os.path.join(ROOT, "include", "d2g.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", d2g.LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    from dashing2_amd import capi
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in exported and s in capi.SIGNATURES and hasattr(d2g.lib(), s), s
    for m in ("near_dev", "within_dev", "knn"):
        assert callable(getattr(d2g.SeqSet, m))


def test_constants_and_the_band_bound(d2g):
    header = open(os.path.join(ROOT, "include", "d2g.h")).read()
    assert int(re.search(r"#define\s+D2G_EDIT_BAND_MAX\s+(\d+)", header).group(1)) == d2g.EDIT_BAND_MAX == 31
    assert int(re.search(r"#define\s+D2G_TIME_EDIT_NEAR\s+(\d+)", header).group(1)) == d2g.TIME_EDIT_NEAR == 2 * d2g.TIME_EDIT
    assert d2g.lib().d2g_edit_band_max() == d2g.EDIT_BAND_MAX


def test_null_arguments_are_refused_without_a_device(d2g):
    assert d2g.lib().d2g_edit_near_dev(None, None, 0, 0, 3, None, None) == -1
    assert d2g.lib().d2g_edit_within_dev(None, None, 0, 0, 0, 3, 0, None, None, None, 0, None) == -1
    assert d2g.lib().d2g_edit_knn(None, None, 0, 0, 0, 3, 0, 0, None, None, None, 0, None) == -1
