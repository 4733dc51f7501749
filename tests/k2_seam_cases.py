"""Register matrices whose equality counts are known BY CONSTRUCTION (test infrastructure for the K2 seam tests; pinned itself by
test_k2_seam_cases.py).

A matrix [N][S] of uint64 is built column by column from a RECIPE: how many values of the column are shared (held by two sketches or
more) and how often each one repeats.  With the matrix come, computed from the recipe and never from the matrix,

    d2[t]        the number of shared values of column t (what the rank kernel calls D2),
    labels[t][i] the index (>= 0) of the shared value sketch i holds in column t, or -1 for a value nobody else holds,
    shared[t]    the shared values of column t themselves (shared[t][k] is the value of label k),

and the exact equality count of a pair (i, j) is  sum_t (labels[t][i] == labels[t][j]) & (labels[t][i] >= 0)  in NumPy int64
(`counts_rect`, `counts_ut`).  That label count is the reference: it never looks at a 64-bit value, a hash table or a bit plane.

Equality here is equality of 64-bit PATTERNS -- what both GPU kernels implement, and what the reference program does for integer
registers.  `oracle.eqcounts_ut` takes float64 and compares as doubles: there ~0 (a NaN) equals nothing, itself included, and
0x8000000000000000 (-0.0) equals 0.  NEVER pass a matrix of the `specials` pool to the oracle.  The other pools hold neither a NaN
pattern nor a zero of either sign, so that for them both notions of equality agree.

Column recipes (functions of N that return the repeat counts of the shared values; every other sketch is unique):
    distinct, pairs (every value twice, the last one three times when N is odd), constant, two_values, shared(d, reps).
Value pools: random, low_only (high word 0), high_only (low word 0), twins (half of a column's values share their HIGH word and
differ in the low one, the other half share their LOW word), specials (SPECIALS first -- dealt in turn to shared labels and to
unique sketches, starting with SPECIALS[t % 10] in column t -- then random patterns).
Which sketch holds which label is a seeded permutation: equal values are not neighbours.
Matrix recipes: uniform, striped, one_busy_column_per_group."""
import numpy as np

M64 = 0xFFFFFFFFFFFFFFFF
SPECIALS = (0, M64, 0xFFFFFFFF, 0xFFFFFFFF00000000, 0x80000000, 0x8000000000000000, 0x40000000, 0x4000000000000000, 1, 2 ** 63 - 1)
POOLS = ("random", "low_only", "high_only", "twins", "specials")
PLAIN_POOLS = POOLS[:4]                                               # no NaN pattern, no zero: the oracle may see them


# ---------------------------------------------------------------- column recipes: N -> repeat counts of the shared values
class Recipe:
    def __init__(self, name, reps_of):
        self.name, self._reps_of = name, reps_of

    def reps(self, N):
        r = np.asarray(self._reps_of(N), np.int64).reshape(-1)
        if r.size and (r.min() < 2 or int(r.sum()) > N):
            raise ValueError(f"recipe {self.name}: repeat counts {r[:8]}... do not fit {N} sketches")
        return r

    def __repr__(self):
        return self.name


def _pairs(N):
    r = np.full(N // 2, 2, np.int64)
    if N % 2 and r.size:
        r[-1] = 3
    return r


def _two(N):
    if N < 4:
        raise ValueError("two_values needs N >= 4")
    return [N - N // 2, N // 2]


distinct = Recipe("distinct", lambda N: [])
pairs = Recipe("pairs", _pairs)
constant = Recipe("constant", lambda N: [N] if N >= 2 else [])
two_values = Recipe("two_values", _two)


def shared(d, reps=2):
    """exactly d shared values; reps: one repeat count for all of them, or d of them; the other sketches are unique"""
    rr = np.full(d, reps, np.int64) if np.isscalar(reps) else np.asarray(reps, np.int64)
    assert rr.size == d
    return Recipe(f"shared({d})", lambda N: rr)


# ---------------------------------------------------------------- value pools: n DISTINCT 64-bit patterns
def _hi_words(rng, n):
    """n random 32-bit high words, none 0 and none with an all-ones double exponent (no NaN, no infinity, no zero)"""
    h = rng.integers(1, 1 << 32, n, dtype=np.uint64)
    bad = ((h >> np.uint64(20)) & np.uint64(0x7FF)) == np.uint64(0x7FF)
    h[bad] ^= np.uint64(1 << 30)                                      # clears one exponent bit: still non-zero
    return h


def _distinct(draw, n):
    """n distinct values from draw(k) (k values, repeats possible)"""
    v = np.unique(draw(n))
    while v.size < n:
        v = np.unique(np.concatenate([v, draw(n - v.size + 8)]))
    return v[:n]


def pool_values(pool, n, rng, exclude=()):
    """n distinct uint64 patterns of the pool, in random order"""
    if n == 0:
        return np.zeros(0, np.uint64)
    if pool in ("random", "specials"):
        if pool == "random":
            draw = lambda k: (_hi_words(rng, k) << np.uint64(32)) | rng.integers(0, 1 << 32, k, dtype=np.uint64)
        else:                                                          # any pattern at all (NaNs included), but none of `exclude`
            ex = np.array(exclude, np.uint64)
            def draw(k):
                v = rng.integers(0, M64, k, dtype=np.uint64, endpoint=True)
                return v[~np.isin(v, ex)]
        v = _distinct(draw, n)
    elif pool == "low_only":
        v = _distinct(lambda k: rng.integers(1, 1 << 32, k, dtype=np.uint64), n)
    elif pool == "high_only":
        v = _distinct(lambda k: _hi_words(rng, k), n) << np.uint64(32)
    elif pool == "twins":
        # n - n // 2 values (H, lo_i): one high word, distinct low words; n // 2 values (hi_i, L): one low word, distinct high words != H
        # (L is none of the lo_i, so the two families share no value)
        na, nb = n - n // 2, n // 2
        lo = _distinct(lambda k: rng.integers(1, 1 << 32, k, dtype=np.uint64), na + 1)
        hi = _distinct(lambda k: _hi_words(rng, k), nb + 1)
        rng.shuffle(lo)
        rng.shuffle(hi)
        v = np.concatenate([(hi[0] << np.uint64(32)) | lo[1:], (hi[1:] << np.uint64(32)) | lo[0]])
    else:
        raise ValueError(pool)
    assert v.size == n and np.unique(v).size == n
    return rng.permutation(v)


# ---------------------------------------------------------------- one column
def build_column(N, recipe, pool, rng, t=0):
    """-> (values uint64[N], labels int32[N], shared values uint64[d]); everything but `values` comes from the recipe alone"""
    reps = recipe.reps(N)
    d, nu = reps.size, N - int(reps.sum())
    lab = np.concatenate([np.repeat(np.arange(d, dtype=np.int32), reps), np.full(nu, -1, np.int32)])
    slot = np.concatenate([np.repeat(np.arange(d, dtype=np.int64), reps), d + np.arange(nu, dtype=np.int64)])   # value slot of every sketch
    if pool == "specials":
        # SPECIALS, from SPECIALS[t % 10] on, go in turn to a shared label (0, 1, ...) and to a unique sketch, as long as there is room
        sp = [SPECIALS[(t + k) % len(SPECIALS)] for k in range(len(SPECIALS))]
        vals = np.zeros(d + nu, np.uint64)
        taken = np.zeros(d + nu, bool)
        ns = nq = 0
        for k, s in enumerate(sp):
            to_shared = (k % 2 == 0 and ns < d) or nq >= nu
            if to_shared and ns >= d:
                break
            pos = ns if to_shared else d + nq
            ns, nq = ns + to_shared, nq + (not to_shared)
            vals[pos], taken[pos] = np.uint64(s), True
        vals[~taken] = pool_values(pool, int((~taken).sum()), rng, exclude=SPECIALS)
    else:
        vals = pool_values(pool, d + nu, rng)
    perm = rng.permutation(N)                                         # sketch perm[k] takes entry k
    values, labels = np.empty(N, np.uint64), np.empty(N, np.int32)
    values[perm], labels[perm] = vals[slot], lab
    return values, labels, vals[:d].copy()


# ---------------------------------------------------------------- matrices
class Case:
    """matrix uint64 [N][S]; d2 int64 [S]; labels int32 [S][N]; shared: list of uint64 arrays; recipes, pools: per column"""

    def __init__(self, matrix, d2, labels, shared_values, recipes, pools):
        self.matrix, self.d2, self.labels, self.shared, self.recipes, self.pools = matrix, d2, labels, shared_values, recipes, pools
        self.N, self.S = matrix.shape
        self._lab_rows = np.where(labels < 0, np.int32(-2), labels)   # the row side: a unique sketch (-2) equals no column-side label (-1)
        self._busy = [t for t in range(self.S) if d2[t] > 0]          # a column without a shared value adds nothing to any count

    # the reference: sum_t (label_t[i] == label_t[j]) & (label_t[i] >= 0), int64
    def counts_rect(self, a0, a1, b0, b1):
        acc = np.zeros((a1 - a0, b1 - b0), np.int64)
        for t in self._busy:
            la = self._lab_rows[t, a0:a1]
            if la.size and la.max() >= 0:
                acc += la[:, None] == self.labels[t, None, b0:b1]
        for i in range(max(a0, b0), min(a1, b1)):                     # a sketch against ITSELF agrees in every register, unique values included
            acc[i - a0, i - b0] = self.S
        return acc

    def counts_ut(self, r0=0, r1=None):
        """rows [r0, r1) of the condensed upper triangle (pairs i < j, row by row)"""
        r1 = self.N if r1 is None else r1
        if r1 <= r0 or r0 + 1 >= self.N:
            return np.zeros(0, np.int64)
        blk = self.counts_rect(r0, r1, r0 + 1, self.N)
        return blk[np.arange(r0 + 1, self.N)[None, :] > np.arange(r0, r1)[:, None]]

    def group_max_d2(self, order=None):
        """max D2 of every 32-column group when the columns stand in `order` (default: as given -- the operand's order with D2G_BS_SORT=0)"""
        d = self.d2 if order is None else self.d2[order]
        return np.array([d[g:g + 32].max() for g in range(0, self.S, 32)], np.int64)

    def planes_expected(self, sorted_columns):
        """(max D2 + 1, most id planes of a group, mean id planes per group as float32) -- with the column plan's sort (stable, descending
        plane class bit_length(D2 + 1)) or without it"""
        order = None
        if sorted_columns:
            cls = np.array([int(x + 1).bit_length() for x in self.d2])
            order = np.argsort(-cls, kind="stable")
        gm = self.group_max_d2(order)
        nb = [int(x + 1).bit_length() for x in gm]
        return int(self.d2.max()) + 1, max(nb), np.float32(sum(nb) / len(nb))


def ut_offsets(N):
    """offsets of the rows in the condensed upper triangle (N + 1 entries)"""
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def from_columns(N, columns, seed):
    """columns: list of (recipe, pool) -- fresh values and a fresh permutation per column"""
    rng = np.random.default_rng(seed)
    S = len(columns)
    m = np.empty((N, S), np.uint64)
    labels = np.empty((S, N), np.int32)
    d2 = np.zeros(S, np.int64)
    sh = []
    for t, (rec, pool) in enumerate(columns):
        m[:, t], labels[t], s = build_column(N, rec, pool, rng, t)
        d2[t] = rec.reps(N).size
        sh.append(s)
    return Case(m, d2, labels, sh, [c[0] for c in columns], [c[1] for c in columns])


def uniform(N, S, recipe, pool="random", seed=0):
    """every column the same recipe, fresh values per column"""
    return from_columns(N, [(recipe, pool)] * S, seed)


def striped(N, S, recipes, pools=("random",), seed=0):
    """column t: recipes[t % len(recipes)] with pools[(t // len(recipes)) % len(pools)] -- a known pattern: with D2G_BS_SORT=0 the
    maximum D2 of every 32-column group follows from the recipes (Case.group_max_d2)"""
    R, P = len(recipes), len(pools)
    return from_columns(N, [(recipes[t % R], pools[(t // R) % P]) for t in range(S)], seed)


def one_busy_column_per_group(N, S, busy, quiet=distinct, pool="random", seed=0):
    """column 32 g + (7 g + 3) % (columns of group g) of every 32-column group g follows `busy`, every other column `quiet`"""
    busy_cols = {32 * g + (7 * g + 3) % min(32, S - 32 * g) for g in range(-(-S // 32))}
    return from_columns(N, [(busy if t in busy_cols else quiet, pool) for t in range(S)], seed)
