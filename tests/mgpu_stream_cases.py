"""Streams of DIFFERENT matrices for the multi-GPU engine's loopback tests (test_gpu_mgpu_streams.py), and the conditions that make a
stale buffer visible.  No GPU and no library kernel: NumPy only; the row ranges come from the caller (d2g.ut_partition is host arithmetic).

sequence(N, S, T, seed, kinds) -> T float64 matrices [N][S], every entry finite and >= 0, one structure per step, `kinds` cycled:
    ("planted", nvals)   every register of a column drawn from `nvals` values drawn afresh for the step (test_gpu_mgpu._planted).  On even
                         steps 5 % of the registers are 0.0 (the pattern of all-zero bits); odd steps hold none, so that P1 holds
    "families"           families of ~40 sketches that share 70 % of their family's registers, strangers otherwise; fresh values and
                         fresh membership every step
    "one_family"         every sketch shares half of ONE base sketch's registers: the ordering gives up, the dense walk runs

What a step must not inherit from the step before it, as conditions on the INPUTS (held to them by test_mgpu_stream_cases.py for every
shape and world size the GPU tests use; the pair ranges are those of d2g.ut_partition, the rows a rank holds the even split):
    P1  no 64-bit pattern of step t occurs anywhere in step t-1: a stale input row counts 0 against fresh rows instead of looking right
    P2  for every step t >= 1, every 32-register group g (the last, shorter one included) and every rank with a non-empty slab, the
        counts over group g's columns alone differ between M_t and M_t-1 for at least 100 pairs of the rank's slab (planted sequences;
        1 pair in family sequences): a block of groups left from the previous gather -- stale planes, stale meta, a transfer that did
        not happen or landed in another block -- changes every rank's result
    P3  the rows a rank holds differ between consecutive steps in at least 90 % of their entries (planted; 1 % family sequences)

Measured minima (the figures test_mgpu_stream_cases.py prints), planted sequence PLANTED_KINDS, T = 6:
    W  N    S     P2 min pairs over steps, groups, ranks   P3 min fraction
    2  263  1000  13078                        1.0
    3  517  96    39640                        1.0
    4  300  1024  9779                         1.0
    8  77   1024  291                          1.0
    5  129  100   1001                         1.0
family sequence FAMILY_KINDS, T = 18 (P2 counted over the first FAMILY_WITNESS_ROWS rows of every rank's slab only -- a lower bound):
    2  2600 512   >= 14647                     1.0
    3  1100 128   >= 5030                      1.0
the refused matrix and the clean one behind it (overflow_then_clean, OVERFLOW_SHAPE; same lower bound):
    2  3000 128   >= 16913                     1.0
P1 makes P3 1.0 by itself: a matrix that shares no pattern with its predecessor differs from it everywhere."""
import numpy as np

PLANTED_KINDS = tuple(("planted", n) for n in (2, 5, 3, 8, 4, 6))
FAMILY_KINDS = ("families", "one_family", "families", ("planted", 3))
STREAM_SHAPES = [(2, 263, 1000), (3, 517, 96), (4, 300, 1024), (8, 77, 1024), (5, 129, 100)]      # (W, N, S): planted, T = STREAM_T
STREAM_T = 6
FAMILY_SHAPES = [(2, 2600, 512), (3, 1100, 128)]                                                    # (W, N, S): FAMILY_KINDS, T = FAMILY_T
FAMILY_T = 18
FAMILY_WITNESS_ROWS = 8
OVERFLOW_SHAPE = (2, 3000, 128)                                                                     # the D2G_BS_TAGBITS=0 arrangement, then a clean matrix
ZERO_FRAC = 0.05


def seed_of(W, N, S):
    """the seed of the sequence every test of one shape uses: the CPU test holds exactly the matrices the GPU tests feed to P1-P3"""
    return 20261018 + 1000003 * W + 1009 * N + S


def overflow_then_clean(N, S, seed):
    """[a matrix whose first 64 columns hold N distinct values each (they overflow the rank kernel's fix list under D2G_BS_TAGBITS=0) and
    whose other columns are constant, a planted matrix of fresh values]"""
    rng = np.random.default_rng(seed)
    bad = np.empty((N, S))
    bad[:, :64] = rng.random((N, 64))
    bad[:, 64:] = rng.random(S - 64)[None, :]
    return [bad, _one(rng, N, S, ("planted", 5), 1)]


def _one(rng, N, S, kind, t):
    if kind == "families":
        fam = rng.integers(0, max(2, N // 40), N)
        base = rng.random((int(fam.max()) + 1, S))
        return np.where(rng.random((N, S)) < 0.7, base[fam], rng.random((N, S)))
    if kind == "one_family":
        base = rng.random(S)
        return np.where(rng.random((N, S)) < 0.5, base[None, :], rng.random((N, S)))
    name, nvals = kind
    assert name == "planted"
    vals = rng.random((nvals, S))
    m = vals[rng.integers(0, nvals, (N, S)), np.arange(S)[None, :]]
    if t % 2 == 0:
        m[rng.random((N, S)) < ZERO_FRAC] = 0.0
    return m


def sequence(N, S, T, seed, kinds):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(_one(rng, N, S, kinds[t % len(kinds)], t)) for t in range(T)]


def even_split(total, parts):
    """[parts + 1] bounds, sizes differ by at most one: the rows (and register groups) rank q holds"""
    return [total * p // parts for p in range(parts + 1)]


def ut_offsets(N):
    """offset of row i in the condensed upper triangle, [N + 1]"""
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def shared_patterns(a, b):
    """how many distinct 64-bit patterns of `a` occur in `b` (P1 wants 0)"""
    return int(np.intersect1d(a.view(np.uint64).ravel(), b.view(np.uint64).ravel()).size)


def group_counts(m, r0, r1):
    """equality counts of rows [r0, r1) against ALL rows, per 32-register group: uint16 [r1 - r0][N][ceil(S / 32)] (blocked comparisons)"""
    N, S = m.shape
    starts = np.arange(0, S, 32)
    out = np.empty((r1 - r0, N, starts.size), np.uint16)
    step = max(1, (1 << 24) // (N * S))
    for a in range(r0, r1, step):
        z = min(a + step, r1)
        eq = m[a:z, None, :] == m[None, :, :]
        out[a - r0:z - r0] = np.add.reduceat(eq, starts, axis=2, dtype=np.uint16)
    return out


def pairs_that_differ(ga, gb, r0):
    """P2 of rows [r0, r0 + len(ga)): per group, the pairs (i, j), i < j, whose count over the group's columns differs between two steps"""
    n, N, _ = ga.shape
    upper = np.arange(N)[None, :] > (r0 + np.arange(n))[:, None]
    return ((ga != gb) & upper[:, :, None]).sum(axis=(0, 1))


def slab_fraction_that_differs(a, b, lo, hi):
    """P3: the share of rank's held rows [lo, hi) whose 64-bit patterns differ between two steps (1.0 for no rows)"""
    if hi <= lo:
        return 1.0
    return float((a[lo:hi].view(np.uint64) != b[lo:hi].view(np.uint64)).mean())
