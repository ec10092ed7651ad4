"""The definition of the bilateral pre-filter of the normal map, checked on its float64 NumPy model alone (no GPU): the properties
that make it worth having in front of a Sobel -- it leaves flat regions alone, it does not mix the two sides of a silhouette, it
smooths the one-level terraces of a quantised ramp -- and the pure-Python argument checks of the public layers.
tests/test_gpu_normalmap_bilateral.py holds the kernel to this model bit for bit."""
import numpy as np
import pytest

import normalmap_bilateral_cases as bc


def rounding_slack(params, vmax):
    """How far the definition's float64 accumulation can carry a weighted mean of values <= vmax away from the exact one: T taps,
    relative error of num below T u, of den below (T - 1) u, one more u for the division, u = 2^-53 (first order; the factor 2 T + 2
    covers the higher-order terms for T <= 709).  At vmax = 65535 and d = 31 this is 1e-8 levels: the properties below are stated
    for the exact weighted mean and hold for the computed one up to this slack, not beyond it."""
    taps = int(np.count_nonzero(bc.tables(*params)[0]))
    return (2 * taps + 2) * 2.0 ** -53 * vmax


@pytest.mark.parametrize("wrap", [False, True], ids=["reflect", "wrap"])
def test_a_constant_map_is_returned_exactly(wrap):
    """On a constant map v every range weight is wr[0] = 1: num = sum fl(ws[t] v), den = sum ws[t].  For v = 0 and v a power of two
    every product is exact, so num = v den exactly and the quotient IS v.  For any other v each product and each of the two sums
    rounds (T taps: relative error of num below T u, of den below (T - 1) u, one more u for the division, u = 2^-53), so the
    definition returns v only to within (2 T + 2) u v -- an exact return for every v, which the feature request states, is not a
    property of the accumulation it fixes: v = 12345 with (9, 300.0, 2.5) comes out one unit in the last place off."""
    for params in ((3, 3.0, 1.0), (9, 300.0, 2.5), (15, 20000.0, 5.0)):
        taps = int(np.count_nonzero(bc.tables(*params)[0]))
        for value in (0, 1, 2, 256, 4096, 32768):
            d = np.full((9, 11), value, np.uint16)
            out = bc.model(d, params, wrap)
            assert out.dtype == np.float64 and np.array_equal(out, d.astype(np.float64)), (value, params)
        for value in (3, 255, 12345, 40000, 65535):
            d = np.full((9, 11), value, np.uint16)
            err = np.abs(bc.model(d, params, wrap) - value).max()
            assert err <= (2 * taps + 2) * 2.0 ** -53 * value, (value, params, err)


def test_the_far_side_of_a_cliff_has_weight_zero():
    """sigma_color = 64: wr[k] = exp(-k^2 / 8192) is exactly 0.0 from k = 4096 on (exp(-2048.0) == 0), so each side of the cliff
    stays within its own [min, max] although the window reaches across -- up to the rounding of the accumulation (rounding_slack:
    the computed mean of equal values v can be an ulp or two off v; measured here: 2 ulp = 7.3e-12 below the minimum)."""
    assert np.exp(-2048.0) == 0.0
    ws, wr = bc.tables(9, 64.0, 3.0)
    assert wr[0] == 1.0 and np.all(wr[bc.CLIFF - 60:] == 0.0)
    h, w, cut = 12, 60, 30
    d = bc.staircase(h, w, cliff_at=cut)
    assert int(d[0, cut]) - int(d[0, cut - 1]) >= bc.CLIFF
    for wrap in (False, True):
        out = bc.model(d, (9, 64.0, 3.0), wrap)
        for side, sl in (("low", slice(0, cut)), ("high", slice(cut, w))):
            eps = rounding_slack((9, 64.0, 3.0), float(d[:, sl].max()))
            assert eps < 1e-9
            assert out[:, sl].min() >= d[:, sl].min() - eps and out[:, sl].max() <= d[:, sl].max() + eps, (wrap, side)
    # a Gaussian of the same window does mix them
    blur = bc.model(d, (9, 1e9, 3.0))
    assert blur[:, cut - 1].max() > d[:, :cut].max() + 100


def test_the_staircase_comes_out_monotone_and_smoother():
    """(5, 300.0, 2.0) on one-level steps 6 pixels wide: the output rises monotonically (up to the rounding of two neighbouring
    means on a tread, where the exact means are equal: measured 2 ulp = 7.3e-12) and its largest second difference, 0.18 of a level,
    is smaller than the input's, 1 level."""
    h, w, cut = 8, 96, 48
    params = (5, 300.0, 2.0)
    d = bc.staircase(h, w, cliff_at=cut)
    out = bc.model(d, params)
    for sl in (slice(0, cut), slice(cut, w)):                 # away from the cliff: each side on its own
        a, f = d[3, sl].astype(np.float64), out[3, sl]
        assert np.all(np.diff(f) >= -2.0 * rounding_slack(params, a.max()))
        assert f[-1] - f[0] > 6.0                             # it does rise: 8 treads per side
        assert np.abs(np.diff(f, 2)).max() < 0.25 < np.abs(np.diff(a, 2)).max() == 1.0


@pytest.mark.parametrize("params", [(3, 3.0, 1.0), (9, 300.0, 2.5), (31, 50.0, 9.0)], ids=["d3", "d9", "d31"])
def test_wrap_equals_the_reflect_model_on_the_wrap_padded_input(params):
    r = params[0] // 2
    for h, w in ((17, 16), (33, 40)):
        for name, d in bc.cases(h, w, seed=h + w):
            want = bc.model(np.pad(d, r, mode='wrap'), params)[r:r + h, r:r + w]
            assert np.array_equal(bc.model(d, params, wrap=True), want), (name, h, w)
    small = bc.random_depth(4, 6, seed=3)                     # window wider than the image: wrap only, the pad goes round
    want = bc.model(np.pad(small, r, mode='wrap'), params)[r:r + 4, r:r + 6]
    assert np.array_equal(bc.model(small, params, wrap=True), want)


def test_model_tables_are_the_products_tables():
    from src import _native
    for params in ((3, 3.0, 1.0), (15, 20000.0, 5.0), (31, 50.0, 9.0)):
        ws, wr = _native.bilateral_tables(*params)
        mws, mwr = bc.tables(*params)
        assert ws.dtype == np.float64 and wr.dtype == np.float64 and ws.shape == (params[0] ** 2,) and wr.shape == (65536,)
        assert np.array_equal(ws, mws.ravel()) and np.array_equal(wr, mwr)
        r = params[0] // 2
        assert ws[0] == 0.0 and ws[r] != 0.0 and ws[(params[0] ** 2) // 2] == 1.0       # corner outside the circle, (-R, 0) on it


BAD_TUPLES = [(4, 1, 1), (1, 1.0, 1.0), (33, 1.0, 1.0), (5, 0.0, 1.0), (5, 1.0, -2.0), (5, float("nan"), 1.0), (5, 1.0, float("inf")),
              (5.5, 1.0, 1.0), (5, 1.0), 5, "5,1,1", (True, 1.0, 1.0), (5, "a", 1.0)]


def test_bad_tuples_and_other_dtypes_raise_in_the_pure_python_checks():
    from src import _native
    import src.normalmap_generation as nm
    assert _native.bilateral_params((5, 300, 2)) == (5, 300.0, 2.0)
    assert _native.bilateral_params([31, 0.5, 9.0]) == (31, 0.5, 9.0)
    for bad in BAD_TUPLES:
        with pytest.raises(ValueError):
            _native.bilateral_params(bad)
        with pytest.raises(_native.DepthStereoError, match="create_normalmap"):
            nm._check_bilateral(bad, True, np.dtype(np.uint16))
    assert nm._check_bilateral((5, 300.0, 2.0), True, np.dtype(np.uint16)) == (5, 300.0, 2.0)
    for dt in (np.float64, np.float32, np.float16, np.uint8, np.int32):
        with pytest.raises(_native.DepthStereoError, match="uint16 depth maps only"):
            nm._check_bilateral((5, 300.0, 2.0), False, np.dtype(dt))
