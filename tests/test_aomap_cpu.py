"""The ambient-occlusion map without a GPU: what the definition (include/depthstereo.h, ds_aomap_u16) promises, shown on its NumPy
model (tests/aomap_cases.py); the product's host half (the ray table builder, the validator) against the model's; and a census that
keeps tests/test_gpu_aomap.py honest: the case list it runs must contain the inputs on which a wrong tie rule, a missing clamp or a
mishandled empty ray would show."""
import numpy as np
import pytest

import aomap_cases as ac


def test_a_flat_map_sees_the_whole_sky():
    for wrap in (False, True):
        for invert in (False, True):
            u8, v = ac.model(ac.flat(9, 13), 8, 16, 2000.0, 1.5, invert=invert, wrap=wrap)
            assert (u8 == 255).all() and (v == 1.0).all()


def test_a_spike_shades_its_surroundings_and_not_itself():
    d = ac.spike(21, 30)
    u8, _ = ac.model(d, 8, 8, 64.0)
    y, x = 21 // 2, 30 // 3
    assert u8[y, x] == 255 and u8[y, x + 1] < 255 and u8[y + 8, x] < 255 and u8[y + 9, x] == 255 and u8[0, 29] == 255


@pytest.mark.parametrize("shape,params", [((40, 70), (32, 16, 2000.0, 1.5)), ((9, 33), (8, 8, 64.0, 1.0)), ((4, 6), (32, 16, 64.0, 1.0)),
                                          ((4, 6), (32, 8, 64.0, 1.0)), ((5, 7), (3, 4, 65535.0, 1.0))],
                         ids=lambda v: "x".join(str(i) for i in v[:2]))
def test_wrap_is_the_model_on_a_wrap_padded_map(shape, params):
    h, w = shape
    R = params[0]
    for name, d in ac.depth_cases(h, w, seed=h + w):
        for invert in (False, True):
            u8, v = ac.model(d, *params, invert=invert, wrap=True)
            pu8, pv = ac.model(np.pad(d, R, mode='wrap'), *params, invert=invert, wrap=False)
            assert np.array_equal(u8, pu8[R:R + h, R:R + w]) and np.array_equal(v, pv[R:R + h, R:R + w]), (name, invert)


def test_wrap_tiles_like_the_map():
    for (h, w), params in (((9, 14), (8, 8, 64.0, 1.0)), ((4, 6), (32, 16, 2000.0, 1.0)), ((6, 5), (1, 8, 300.0, 1.0))):
        for name, d in ac.depth_cases(h, w, seed=3 * h + w):
            u8, v = ac.model(d, *params, wrap=True)
            tu8, tv = ac.model(np.tile(d, (2, 2)), *params, wrap=True)
            assert np.array_equal(tu8, np.tile(u8, (2, 2))) and np.array_equal(tv, np.tile(v, (2, 2))), name


def test_offset_builder_equals_the_models_table():
    from src import _native
    for K in ac.DIRECTIONS:
        for R in ac.RADII:
            taps, start = _native.aomap_offsets(R, K)
            want_taps, want_start = ac.table(R, K)
            assert taps.dtype == np.int32 and start.dtype == np.int32 and taps.shape == want_taps.shape and start.shape == (K + 1,)
            assert np.array_equal(taps, want_taps) and np.array_equal(start, want_start), (R, K)
            assert start[-1] == len(taps) <= K * R
    # what the definition says about the table itself
    assert [len(r) for r in ac.rays(1, 8)] == [1, 0] * 4                          # at R = 1 the diagonals are empty
    assert len(ac.table(32, 16)[0]) <= 16 * 32
    for K in ac.DIRECTIONS:
        for R in (1, 2, 5, 32):
            for ray in ac.rays(R, K):
                assert len({t[:2] for t in ray}) == len(ray) and all(t[2] <= R * R for t in ray)
    frac = np.abs((np.arange(1, 33) * (np.sqrt(2.0) - 1.0)) % 1.0 - 0.5)
    assert frac.min() > 0.0147                                                    # no step comes near a tie of rint


def test_validator_accepts_and_rejects():
    from src import _native
    assert _native.aomap_params((16, 8, 32.0)) == (16, 8, 32.0, 1.0)
    assert _native.aomap_params([1, 4, 1, 2]) == (1, 4, 1.0, 2.0)
    assert _native.aomap_params((32, 16, 1e-9, 1e9)) == (32, 16, 1e-9, 1e9)
    assert _native.aomap_params((np.int64(8), np.int32(16), np.float32(2.0))) == (8, 16, 2.0, 1.0)
    assert _native.aomap_params((8.0, 16.0, 2)) == (8, 16, 2.0, 1.0)              # a float that IS the integer
    got = _native.aomap_params((3, 4, 5))
    assert [type(v) for v in got] == [int, int, float, float]
    for bad in ((0, 8, 32.0), (33, 8, 32.0), (-1, 8, 32.0), (8.5, 8, 32.0), (True, 8, 32.0), (8, True, 32.0), (np.bool_(True), 8, 32.0),
                (8, 5, 32.0), (8, 0, 32.0), (8, 32, 32.0), (8, 8, 0.0), (8, 8, -1.0), (8, 8, float('inf')), (8, 8, float('nan')),
                (8, 8, 32.0, 0.0), (8, 8, 32.0, -2.0), (8, 8, 32.0, float('inf')), (8, 8, 32.0, float('nan')), (8, 8), (8,),
                (8, 8, 32.0, 1.0, 1.0), "8", b"888", 8, None, (8, 8, "x"), ("r", 8, 32.0), (8, 8, None), {0: 8, 1: 8, 2: 32.0}):
        with pytest.raises(ValueError):
            _native.aomap_params(bad)


def test_census_of_the_gpu_cases():
    """From the model alone: the case list of tests/test_gpu_aomap.py contains a case where the opposite tie rule changes float64
    outputs, a case whose value goes below 0 (the clamp runs) and a case with an empty ray."""
    shape, params = ac.KERNEL_CASES[2]
    assert shape == (1, 40, 70) and params[:3] == (32, 16, 2000.0)
    d = ac.inputs(shape)["ramp12_12"]
    _, v = ac.model(d, *params, wrap=True)
    _, v_ge = ac.model(d, *params, wrap=True, tie_ge=True)
    changed = int((v != v_ge).sum())
    print("pixels whose float64 value the opposite tie rule changes:", changed, "of", v.size)
    assert changed > 0
    u8, v = ac.want(shape, params, "random", False, False)
    assert (v < 0.0).any() and (u8 == 0).any() and (v > 0.0).any()
    u8w, vw = ac.want(shape, params, "random", False, True)
    assert (vw < 0.0).any()
    assert any(p[0] == 1 and p[1] == 8 for _, p in ac.KERNEL_CASES) and any(len(r) == 0 for r in ac.rays(1, 8))
    # and every case list entry is a legal parameter tuple
    from src import _native
    for _, p in ac.KERNEL_CASES:
        assert _native.aomap_params(p) == p
