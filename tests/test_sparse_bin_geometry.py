"""The output bins of the sparse path's pair list (d2g_sparse_bin_geometry: the arithmetic a set's allocation runs).  Host code only, no GPU.

A band of 32 output rows x a chunk of 2^cshift columns is one bin; a set may have SP_BIN_MAX = 39 936 of them (their cursors live in the LDS
of one workgroup).  cshift starts at 10 and grows while there would be more bins; beyond 1 277 952 sketches the bands alone are too many
and the list is applied entry by entry.  The call runs in a child process: a geometry loop that never ends fails the test instead of
stalling the suite."""
import json
import os
import subprocess
import sys

from conftest import ROOT

SP_BIN_MAX = 39 * 1024
BANDS_MAX_N = 32 * SP_BIN_MAX                 # 1 277 952


def _div_up(a, b):
    return -(-a // b)


def _fits(N, c):
    return _div_up(N, 32) * _div_up(N, 1 << c) <= SP_BIN_MAX


def _last_n_of(c):
    """the largest N whose bins at width 2^c still fit"""
    lo, hi = 1, BANDS_MAX_N
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if _fits(mid, c) else (lo, mid - 1)
    return lo


def _geometry(ns):
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import dashing2_amd as D; "
            "print(json.dumps([D.sparse_bin_geometry(int(n)) for n in sys.argv[2:]]))")
    r = subprocess.run([sys.executable, "-c", code, ROOT] + [str(n) for n in ns], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_sparse_bin_geometry_every_threshold():
    thresholds = [_last_n_of(c) for c in range(10, 21)]
    assert thresholds[:4] == [35_840, 51_104, 70_976, 98_304]          # (the widths the issue tracker names: cshift 11, 12, 13, 14 start one later)
    ns = {2, 31, 32, 33, 8191, 8192, 8193, BANDS_MAX_N, BANDS_MAX_N + 1, 1_300_000, 2 ** 30 - 1}
    for t in thresholds:
        ns.update((t, t + 1))
    ns = sorted(ns)
    got = _geometry(ns)
    assert len(got) == len(ns)
    for N, g in zip(ns, got):
        cs, nch, nbins, ok = g["cshift"], g["nch"], g["nbins"], g["binned_ok"]
        bands = _div_up(N, 32)
        assert ok == (bands <= SP_BIN_MAX), (N, g)                     # the 32-row bands alone exceed the bins from 1 277 953 on
        assert cs >= 10 and nch << cs >= N and nch == _div_up(N, 1 << cs), (N, g)
        if ok:
            assert nbins == bands * nch and nbins <= SP_BIN_MAX, (N, g)
            assert cs == 10 or not _fits(N, cs - 1), (N, g)            # the narrowest width that fits
            ppb = (1 << cs) // 1024
            assert bands * nch * ppb * 4 < 2 ** 31, (N, g)             # the compose grid of a whole-triangle launch (launch_sparse)
        else:
            assert nbins == 0 and nch == 1, (N, g)                     # nothing binned: one chunk covers the row
    by_n = dict(zip(ns, got))
    assert [by_n[t]["cshift"] for t in thresholds] == list(range(10, 21))
    assert [by_n[t + 1]["cshift"] for t in thresholds] == list(range(11, 22))
    assert by_n[BANDS_MAX_N] == {"cshift": 21, "nch": 1, "nbins": SP_BIN_MAX, "binned_ok": True}
