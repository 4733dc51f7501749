"""Independent NumPy restatement of the reference's truncated-register comparison, written from the reference source
(src/cmp_core.cpp, src/setsketch.cpp, src/setsketch.h) and from nothing under dashing2_amd/csrc:

    make_compressed()                      src/cmp_core.cpp:209-322   (reg2sig :19-30)
    CSetSketch::optimal_parameters         src/setsketch.h:563-566 -> src/setsketch.cpp:7-10
    g_b()                                  src/cmp_core.cpp:323-325
    compare(), compressed branch           src/cmp_core.cpp:355-361 (prologue), 362-449, 573-575

np.longdouble is the x87 80-bit type on x86-64 Linux (asserted below); its exp/log/log1p/power are the machine's libm expl/logl/
log1pl/powl -- the same functions the C++ calls -- so expected values are computed LIVE by the tests that compare floats.
fmal() is ONE rounding: it is restated with exact rational arithmetic and one round-to-nearest-even to 64 bits.
The epilogues take arrays (one entry per pair) so that a test can afford every pair of a few hundred sketches.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant == 63, "needs the x87 80-bit long double"
F32, F64 = np.float32, np.float64
SIMILARITY, CONTAINMENT, SYMMETRIC_CONTAINMENT, POISSON_LLR, INTERSECTION, UNION_SIZE = range(6)
DBL_MAX = np.finfo(F64).max
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- exact helpers
def ld_to_fraction(x):
    """exact value of a finite long double"""
    x = LD(x)
    if x == 0:
        return Fraction(0)
    m, e = np.frexp(x)                          # x = m * 2^e, 0.5 <= |m| < 1
    n = np.ldexp(abs(m), 64)                    # an integer below 2^64, exact
    hi = np.floor(np.ldexp(n, -32))
    lo = n - np.ldexp(hi, 32)
    mant = (int(float(hi)) << 32) | int(float(lo))
    fr = Fraction(mant) * (Fraction(2) ** (int(e) - 64))
    return -fr if m < 0 else fr


def fraction_to_ld(fr):
    """round-to-nearest-even of an exact rational to the 64-bit significand (normal range)"""
    if fr == 0:
        return LD(0)
    neg, fr = fr < 0, abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length() - 64
    while fr / Fraction(2) ** e >= (1 << 64):
        e += 1
    while fr / Fraction(2) ** e < (1 << 63):
        e -= 1
    scaled = fr / Fraction(2) ** e
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    if n == (1 << 64):
        n >>= 1
        e += 1
    v = np.ldexp(LD(n >> 32) * LD(4294967296.0) + LD(n & 0xFFFFFFFF), e)
    return -v if neg else v


def fmal(x, y, z):
    """fmal(x, y, z) = round(x * y + z), one rounding"""
    return fraction_to_ld(ld_to_fraction(x) * ld_to_fraction(y) + ld_to_fraction(z))


def wang_hash(k):
    """sketch::hash::WangHash::hash (Thomas Wang's published 64-bit mix) on uint64 arrays"""
    k = np.asarray(k, np.uint64).copy()
    u = np.uint64
    with np.errstate(over="ignore"):
        k = ~k + (k << u(21))
        k ^= k >> u(24)
        k = k + (k << u(3)) + (k << u(8))
        k ^= k >> u(14)
        k = k + (k << u(2)) + (k << u(4))
        k ^= k >> u(28)
        k += k << u(31)
    return k


# ---------------------------------------------------------------- make_compressed
CODE_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
Q_DOUBLE = {1: F64(254.3), 2: F64(65534), 4: F64(4294967294)}        # :248 -- double constants, widened
BBIT_SHIFT = {1: 58, 2: 48, 4: 32}                                    # :306


def truncate(sigs, regbytes, bbit):
    """-> (codes, a, b, minreg, maxreg); a = b = 0 (and no min/max) for the b-bit method"""
    sigs = np.ascontiguousarray(sigs, F64)
    if bbit:                                                          # :294-320 with reg2sig(double) :25-29
        h = wang_hash(sigs.view(np.uint64) ^ np.uint64(0xa3407fb23cd20ef))
        return (h >> np.uint64(BBIT_SHIFT[regbytes])).astype(CODE_DTYPE[regbytes]), LD(0), LD(0), None, None
    q = LD(Q_DOUBLE[regbytes])
    keep = ~((sigs <= 0) | (sigs == DBL_MAX))                         # :254
    minreg, maxreg = F64(sigs[keep].min()), F64(sigs[keep].max())     # :250-257
    mx, mn = (minreg, maxreg)                                         # :259 passes (minreg, maxreg) as (maxreg, minreg) ...
    if mx < mn:                                                       # ... setsketch.h:564 swaps
        mx, mn = mn, mx
    b = np.exp(np.log(LD(mx) / LD(mn)) / q)                           # setsketch.cpp:8
    a = LD(mx) / b                                                    # setsketch.cpp:9
    logbinv = LD(1) / np.log1p(b - LD(1))                             # :269
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sub = LD(1) - np.log(sigs.astype(LD) / a) * logbinv           # :282
    top = int(q + LD(1))                                              # int64_t(q + 1)
    fits = np.isfinite(sub) & (sub > -np.ldexp(LD(1), 63)) & (sub < np.ldexp(LD(1), 63))
    isub = np.full(sub.shape, -(1 << 63), np.int64)                   # out of range / inf / NaN: x86 "integer indefinite"
    isub[fits] = np.trunc(sub[fits]).astype(np.int64)                 # static_cast<int64_t>: toward zero
    isub = np.maximum(np.int64(0), np.minimum(np.int64(top), isub))   # :286
    return isub.astype(CODE_DTYPE[regbytes]), a, b, minreg, maxreg


# ---------------------------------------------------------------- compare(), compressed branch
def _max0(x):
    """std::max(x, 0.L) = (x < 0.L) ? 0.L : x  (NaN stays)"""
    return np.where(x < 0, LD(0), x)


def _sim2dist(x, k):
    """:361 with a long double argument: long double arithmetic and logl, returned as double"""
    pm = LD(F64(-1.0) / F64(max(1, k)))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (np.log(LD(2.0) * x / (LD(1.0) + x)) * pm).astype(F64)
    return np.where(x != 0, d, F64(np.inf)).astype(LD)


def _finish(ret):
    """:573-575, then long double -> LSHDistType = float"""
    ret = np.where(np.isnan(ret) | np.isinf(ret), np.finfo(LD).max, ret)
    with np.errstate(over="ignore"):
        return ret.astype(F32)


def epilogue_bbit(neq, S, regbytes, lhc, rhc, measure, k):
    """:406-423 from the number of equal codes (arrays, one entry per pair)"""
    neq = np.atleast_1d(np.asarray(neq, np.int64))
    lhcard, rhcard = np.atleast_1d(np.asarray(lhc, F64)).astype(LD), np.atleast_1d(np.asarray(rhc, F64)).astype(LD)
    invdenom = LD(1) / LD(S)                                          # :360
    b2pow = -np.ldexp(LD(1), -8 * regbytes)                           # :409
    table = {int(n): fmal(LD(int(n)), invdenom, b2pow) for n in np.unique(neq)}
    f = np.array([table[int(n)] for n in neq], LD)
    q = f / (LD(1) + b2pow)
    ret = np.where(LD(0) < q, q, LD(0))                               # std::max(0.L, q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = _max0((lhcard + rhcard) / (LD(2) - (LD(1) - ret)))
        if measure == INTERSECTION:
            ret = u
        elif measure == UNION_SIZE:
            ret = lhcard + rhcard - u
        elif measure == CONTAINMENT:
            ret = u * ret / lhcard
        elif measure == POISSON_LLR:
            ret = _sim2dist(ret, k)
        elif measure == SYMMETRIC_CONTAINMENT:
            ret = u * ret / np.where(rhcard < lhcard, rhcard, lhcard)
    return _finish(ret)


def g_b(b, arg):
    """:323-325"""
    return (LD(1) - np.power(LD(b), -arg)) / (LD(1) - LD(1) / LD(b))


def epilogue_gtlt(gt, lt, S, b, lhc, rhc, measure, k):
    """:425-448 from (#a>b, #a<b) and the base b (arrays, one entry per pair)"""
    gt, lt = np.atleast_1d(np.asarray(gt, np.int64)), np.atleast_1d(np.asarray(lt, np.int64))
    lhcard, rhcard = np.atleast_1d(np.asarray(lhc, F64)).astype(LD), np.atleast_1d(np.asarray(rhc, F64)).astype(LD)
    invdenom = LD(1) / LD(S)
    counts = np.arange(S + 1)
    gb = g_b(b, counts.astype(LD) * invdenom)                         # :425-426, :430-431: g_b(b, count * invdenom)
    alpha, beta = gb[gt], gb[lt]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = np.where(alpha + beta >= 1, lhcard + rhcard, _max0((lhcard + rhcard) / (LD(2) - alpha - beta)))
        ret = _max0(LD(1) - (alpha + beta))                           # :439
        if measure == INTERSECTION:
            ret = ret * mu
        elif measure == UNION_SIZE:
            ret = lhcard + rhcard - (ret * mu)
        elif measure == CONTAINMENT:
            ret = ret * mu / lhcard
        elif measure == SYMMETRIC_CONTAINMENT:
            ret = (ret * mu) / np.where(rhcard < lhcard, rhcard, lhcard)
        elif measure == POISSON_LLR:
            ret = _sim2dist(ret, k)
    return _finish(ret)


# ---------------------------------------------------------------- counts of codes (sketch::eq::count_gtlt / count_eq on the codes)
def gtlt_rect(codes, a0, a1, b0, b1, block=64):
    """(#row > col, #row < col) for rows [a0,a1) x columns [b0,b1), blocked broadcast comparisons"""
    codes = np.ascontiguousarray(codes)
    g = np.zeros((a1 - a0, b1 - b0), np.uint32)
    l = np.zeros_like(g)
    cols = codes[b0:b1]
    for r in range(a0, a1, block):
        rows = codes[r:min(r + block, a1)]
        for c in range(0, b1 - b0, 512):
            cc = cols[c:c + 512]
            g[r - a0:r - a0 + len(rows), c:c + len(cc)] = (rows[:, None, :] > cc[None, :, :]).sum(-1, dtype=np.uint32)
            l[r - a0:r - a0 + len(rows), c:c + len(cc)] = (rows[:, None, :] < cc[None, :, :]).sum(-1, dtype=np.uint32)
    return g, l


def ut_index(N, r0=0, r1=None):
    """(i, j) of every entry of rows [r0,r1) of the condensed upper triangle, in its order"""
    r1 = N if r1 is None else r1
    i = np.concatenate([np.full(N - 1 - r, r, np.int64) for r in range(r0, r1)] or [np.zeros(0, np.int64)])
    j = np.concatenate([np.arange(r + 1, N, dtype=np.int64) for r in range(r0, r1)] or [np.zeros(0, np.int64)])
    return i, j


def gtlt_ut(codes, r0=0, r1=None):
    N = codes.shape[0]
    r1 = N if r1 is None else r1
    g, l = gtlt_rect(codes, r0, r1, 0, N)
    i, j = ut_index(N, r0, r1)
    return g[i - r0, j], l[i - r0, j]


def dist_ut(sigs, cards, regbytes, bbit, measure, k, r0=0, r1=None):
    """what `cmp --fastcmp regbytes [--bbit-sigs]` computes for rows [r0,r1) of the triangle -> (float32 values, a, b)"""
    codes, a, b, _, _ = truncate(sigs, regbytes, bbit)
    N, S = codes.shape
    g, l = gtlt_ut(codes, r0, r1)
    i, j = ut_index(N, r0, r1)
    cards = np.asarray(cards, F64)
    if bbit:
        return epilogue_bbit(S - g.astype(np.int64) - l, S, regbytes, cards[i], cards[j], measure, k), a, b
    return epilogue_gtlt(g, l, S, b, cards[i], cards[j], measure, k), a, b


def dist_rect(sigs, cards, regbytes, bbit, measure, k, a0, a1, b0, b1):
    """the same for the row-major block rows [a0,a1) x columns [b0,b1): compare(row, column)"""
    codes, a, b, _, _ = truncate(sigs, regbytes, bbit)
    S = codes.shape[1]
    g, l = gtlt_rect(codes, a0, a1, b0, b1)
    cards = np.asarray(cards, F64)
    lh = np.repeat(cards[a0:a1], b1 - b0)
    rh = np.tile(cards[b0:b1], a1 - a0)
    if bbit:
        out = epilogue_bbit(S - g.astype(np.int64).ravel() - l.ravel(), S, regbytes, lh, rh, measure, k)
    else:
        out = epilogue_gtlt(g.ravel(), l.ravel(), S, b, lh, rh, measure, k)
    return out.reshape(a1 - a0, b1 - b0), a, b
