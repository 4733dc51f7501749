"""d2g_bmh_check_weights, the host-side checks of d2g_bmh_from_weighted / _ids (no GPU): a set's first guess of its pruning bound,
scale * 1.25 (S / W) (ln S + 8.58) with W its total weight, has to be below 2^864 = 2^1024 / 16^40 -- the redo loop raises a guess
16-fold and gives up after 40 passes -- or the bound can reach +inf, where nothing prunes and the walk of the set never ends.  Such
a set is refused with D2G_ERR_INVALID before anything is allocated or launched; so are NaN, weights above 2^53 and a set_off that
is not monotone, as before."""
import math

import numpy as np
import pytest

LIMIT = 2.0 ** 864
S_MAX = 2 ** 24 - 1
TINY = (1e-306, 1e-310, 5e-324)


def guess(W, S, scale=1.0):
    """bmh_guess of d2g_k3_bmh.hip, the same operations in the same order"""
    m = float(S)
    return scale * (1.25 * (m / W) * (math.log(m) + 0.58 + 8.0))


def refused(d2g, weights, set_off, S, scale=1.0):
    try:
        d2g.bmh_check_weights(None if weights is None else np.asarray(weights, np.float64), np.asarray(set_off, np.uint64), S, scale)
    except d2g.D2GError as e:
        assert e.status == -1                                           # D2G_ERR_INVALID
        return str(e)
    return None


@pytest.mark.parametrize("S", [1, 2, 64, 1000, S_MAX])
@pytest.mark.parametrize("w", TINY)
def test_a_total_weight_that_small_is_refused(d2g, w, S):
    msg = refused(d2g, [w], [0, 1], S)
    assert msg and "set 0" in msg and "total weight too small for the sketch size" in msg
    # a whole set of such weights: its total is still far too small (for a subnormal weight it may not even be normal)
    msg = refused(d2g, [1.0, 2.0] + [w] * 1000, [0, 2, 1002], S)
    assert msg and "set 1" in msg and "total weight too small for the sketch size" in msg
    # behind an empty set and a set of non-positive weights, which have no bound to guess
    msg = refused(d2g, [0.0, -1.0, w], [0, 0, 2, 3], S)
    assert msg and "set 2" in msg


@pytest.mark.parametrize("S", [1, 64, S_MAX])
@pytest.mark.parametrize("w", TINY)
def test_one_such_weight_among_normal_ones_is_accepted(d2g, w, S):
    assert refused(d2g, [3.0, w, 0.25, w, 2.0 ** 53], [0, 5], S) is None
    assert refused(d2g, [w, 1e-200], [0, 2], S) is None


@pytest.mark.parametrize("S", [1, 3, 64, S_MAX])
def test_the_limit_is_two_to_the_864(d2g, S):
    """W0 = the total weight whose guess is 2^864; a part in 10^12 to either side of it is far more than the rounding of the three
    operations and far less than anything a caller could aim at"""
    W0 = 1.25 * float(S) * (math.log(float(S)) + 8.58) / LIMIT
    above, below = W0 * (1 - 1e-12), W0 * (1 + 1e-12)                    # of the limit: a smaller weight gives the larger guess
    assert guess(below, S) < LIMIT < guess(above, S) and math.isfinite(guess(above, S))
    assert refused(d2g, [below], [0, 1], S) is None
    assert refused(d2g, [above], [0, 1], S)
    # the same totals as the sum of a set (four equal parts add exactly)
    assert refused(d2g, [below / 4] * 4, [0, 4], S) is None
    assert refused(d2g, [above / 4] * 4, [0, 4], S)
    # the scale of the first guess counts: the test hook D2G_K3_GUESS_SCALE = 0.001 lets a 1000 times smaller total through
    assert refused(d2g, [above], [0, 1], S, scale=0.001) is None
    assert refused(d2g, [below], [0, 1], S, scale=16.0)


def test_what_passes_stays_finite_through_every_redo_pass():
    """the reasoning behind 2^864, restated on the numbers: 40 raises by 16 of the largest guess that passes stay finite"""
    g = np.nextafter(LIMIT, 0.0)
    for _ in range(40):
        g *= 16.0
    assert math.isfinite(g) and not math.isfinite(LIMIT * 16.0 ** 40)


def test_the_earlier_checks(d2g):
    assert "NaN" in refused(d2g, [1.0, float("nan")], [0, 2], 64)
    assert "2^53" in refused(d2g, [1.0, 2.0 ** 53 * (1 + 2.0 ** -52)], [0, 2], 64)
    assert "2^53" in refused(d2g, [float("inf")], [0, 1], 64)
    assert refused(d2g, [2.0 ** 53], [0, 1], 64) is None
    assert "monotone" in refused(d2g, [1.0, 1.0], [0, 2, 1], 64)
    assert "sketchsize" in refused(d2g, [1.0], [0, 1], 0)
    assert "sketchsize" in refused(d2g, [1.0], [0, 1], 1 << 24)
    # unit weights, empty sets, no sets at all, and weights the walk ignores
    assert refused(d2g, None, [0, 5, 5, 9], 64) is None
    assert refused(d2g, [], [0, 0, 0], 64) is None
    assert refused(d2g, [], [0], 64) is None
    assert refused(d2g, [0.0, -3.0, -float("inf")], [0, 3], 64) is None
