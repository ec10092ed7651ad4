"""The lens blur without a GPU: what the definition (include/depthstereo.h, ds_lensblur_u8) promises, shown on its NumPy model
(tests/lensblur_cases.py) and on a second, per-pixel model; the product's host half (the weight table, the validator) against the
model's; and a census that keeps tests/test_gpu_lensblur.py honest: every case it runs must contain the taps on which a wrong
occlusion rule, a missing clamp, an ignored band or a mishandled border would show."""
import numpy as np
import pytest

import lensblur_cases as lc


@pytest.mark.parametrize("h,w,R,aperture,band", [(5, 7, 2, 6.0, 2734), (4, 6, 32, 16383.75, 4), (6, 9, 5, 20.0, 0), (7, 5, 9, 300.0, 40)])
def test_the_two_models_agree_on_tiny_shapes(h, w, R, aperture, band):
    A = lc.quarter_pixels(aperture)
    image, depths = lc.inputs((1, h, w), R, A)
    for name, depth in depths.items():
        for focus in ('near', 'far', ('point', 0.5, 0.5), 12345):
            for invert in (False, True):
                a = lc.model(image[0], depth[0], focus, R, A, band, invert)
                b = lc.model_loops(image[0], depth[0], focus, R, A, band, invert)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, focus, invert)


def test_all_in_focus_is_the_image():
    """If every rho < 4 the output equals the image."""
    for shape, (R, aperture, _, _) in lc.KERNEL_CASES[:4]:
        A = lc.quarter_pixels(aperture)
        image, depths = lc.inputs(shape, R, A)
        out, rho = lc.model(image, depths["flat"], [777] * shape[0], R, A, 0)
        assert (rho == 0).all() and np.array_equal(out, image)
        # rho up to 3 everywhere: differences just below the one at which rho reaches 4
        e3 = ((4 << 16) - 32768 - 1) // A
        d = (20000 + np.random.default_rng(1).integers(0, e3 + 1, shape)).astype(np.uint16)
        out, rho = lc.model(image, d, [20000] * shape[0], R, A, 0)
        assert rho.max() <= 3 and np.array_equal(out, image)


def test_a_constant_colour_comes_back_unchanged():
    for shape, (R, aperture, focus, band) in lc.KERNEL_CASES:
        A = lc.quarter_pixels(aperture)
        _, depths = lc.inputs(shape, R, A)
        image = np.empty(shape + (3,), np.uint8)
        image[...] = (3, 200, 255)
        for name, depth in depths.items():
            for invert in (False, True):
                out, _ = lc.model(image, depth, lc.focus_list(depth, focus), R, A, band, invert)
                assert np.array_equal(out, image), (shape, name, invert)


def test_accumulator_bound():
    den, num = lc.accumulator_bound(32)
    assert (den, num) == (8103748, 2066455740) and num < 2**31 and 2 * num + den < 2**32
    for R in (1, 2, 8, 16):
        assert lc.accumulator_bound(R)[1] <= num
    for case, (shape, (R, aperture, focus, band)) in enumerate(lc.KERNEL_CASES):
        A = lc.quarter_pixels(aperture)
        image, depths = lc.inputs(shape, R, A)
        census = {}
        for name, depth in depths.items():
            lc.model(image, depth, lc.focus_list(depth, focus), R, A, band, census=census)
        assert census['max_num'] <= 255 * census['max_den'] and census['max_den'] <= lc.accumulator_bound(R)[0] <= den, (case, census)


def test_the_cliff():
    """Focusing the near plane changes only far-plane pixels; focusing the far plane lets the near plane bleed across the edge; invert
    changes outputs."""
    h, w, R, A = 12, 40, 8, 96
    image = lc.random_image(h, w, 7)
    depth = lc.cliff(h, w, 8, 16384)
    near = depth >= 16000                                                  # right of the middle
    out, rho = lc.model(image, depth, 'near', R, A, 10)
    assert (rho[near] == 0).all() and (rho[~near] == 24).all()
    assert np.array_equal(out[near], image[near]) and (out[~near] != image[~near]).any()
    out, rho = lc.model(image, depth, 'far', R, A, 10)
    assert (rho[~near] == 0).all()
    edge = w // 2
    assert (out[:, edge - 6:edge] != image[:, edge - 6:edge]).any()        # in-focus far pixels next to the edge receive the near plane
    assert np.array_equal(out[:, :edge - 6], image[:, :edge - 6])          # and beyond its reach (rho 24 = 6 pixels) nothing does
    for focus in ('near', 'far'):
        assert not np.array_equal(lc.model(image, depth, focus, R, A, 10)[0], lc.model(image, depth, focus, R, A, 10, invert=True)[0])
        assert np.array_equal(lc.model(image, depth, focus, R, A, 10)[1], lc.model(image, depth, focus, R, A, 10, invert=True)[1])


@pytest.mark.parametrize("case", range(len(lc.KERNEL_CASES)), ids=lc.KERNEL_IDS)
def test_census_of_the_gpu_cases(case):
    """From the model alone: the inputs of every case of tests/test_gpu_lensblur.py contain taps that the occlusion rule rejects although
    rho(q) alone would accept them, taps taken with min(...) = rho(p) < rho(q), rho clamped at 4 R, rho = 0 produced by band, and
    border pixels with skipped taps."""
    shape, (R, aperture, focus, band) = lc.KERNEL_CASES[case]
    A = lc.quarter_pixels(aperture)
    image, depths = lc.inputs(shape, R, A)
    census = {}
    for name in lc.DEPTHS:
        lc.model(image, depths[name], lc.focus_list(depths[name], focus), R, A, band, census=census)
    print(lc.KERNEL_IDS[case], census)
    for what in ('occluded', 'took_own', 'clamped', 'banded', 'skipped'):
        assert census[what] > 0, (what, census)
    from src import _native
    assert _native.lensblur_params((R, aperture, 0, band)) == (R, aperture, 0, band) and _native.lensblur_quarter_pixels(aperture) == A


def test_table_builder_equals_the_counts():
    from src import _native
    (t,) = _native.lensblur_table(32)
    assert t.dtype == np.uint32 and t.shape == (129,)
    n = lc.disc_counts(32)
    assert n[:4] == (1, 1, 1, 1) and n[4] == 5 and n[128] == 3209 and 2**20 // n[128] == 326
    assert np.array_equal(t, lc.weights(32)) and int(t[128]) == 326 and int(t[0]) == 2**20
    for R in range(1, 33):
        (t,) = _native.lensblur_table(R)
        assert t.dtype == np.uint32 and np.array_equal(t, lc.weights(R)), R
        assert np.array_equal(t, lc.weights(32)[:4 * R + 1])               # n(rho) does not depend on R


def test_validator_accepts_and_rejects():
    from src import _native
    P = _native.lensblur_params
    assert P((12, 48.0, ('point', 0.5, 0.5))) == (12, 48.0, ('point', 0.5, 0.5), 0)
    assert P([1, 0.25, 0, 0]) == (1, 0.25, 0, 0) and P((32, 16383.75, 65535, 65535)) == (32, 16383.75, 65535, 65535)
    assert P((np.int64(8), np.float32(2.0), np.uint16(7), np.int32(3))) == (8, 2.0, 7, 3)
    assert P((8.0, 3, 7.0, 2.0)) == (8, 3.0, 7, 2)                         # floats that ARE the integers
    assert P((8, 3, ['point', 0, 1])) == (8, 3.0, ('point', 0.0, 1.0), 0)
    assert [type(v) for v in P((3, 4, 5, 6))] == [int, float, int, int]
    assert _native.lensblur_quarter_pixels(48.0) == 192 and _native.lensblur_quarter_pixels(16383.75) == 65535
    for bad in ((0, 48.0, 0), (33, 48.0, 0), (-1, 48.0, 0), (8.5, 48.0, 0), (True, 48.0, 0), (np.bool_(True), 48.0, 0),
                (8, 0.0, 0), (8, -1.0, 0), (8, 0.1, 0), (8, 16383.9, 0), (8, float('inf'), 0), (8, float('nan'), 0), (8, "x", 0), (8, None, 0),
                (8, 48.0, -1), (8, 48.0, 65536), (8, 48.0, 0.5), (8, 48.0, True), (8, 48.0, None), (8, 48.0, "near"),
                (8, 48.0, ('point', 0.5)), (8, 48.0, ('point', 1.5, 0.5)), (8, 48.0, ('point', 0.5, -0.1)), (8, 48.0, ('spot', 0.5, 0.5)),
                (8, 48.0, ('point', float('nan'), 0.5)), (8, 48.0, ('point', "a", 0.5)),
                (8, 48.0, 0, -1), (8, 48.0, 0, 65536), (8, 48.0, 0, 1.5), (8, 48.0, 0, True), (8, 48.0, 0, None),
                (8, 48.0), (8,), (8, 48.0, 0, 0, 0), "8", b"888", 8, None, {0: 8, 1: 48.0, 2: 0}):
        with pytest.raises(ValueError):
            P(bad)
