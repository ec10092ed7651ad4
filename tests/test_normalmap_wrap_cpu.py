"""The yardstick of the wrap-around normal map, pinned with the CPU oracle alone (no GPU, no product code).

These tests check the DEFINITION -- normalmap(np.pad(d, R, mode='wrap'))[R:R+h, R:R+w], tests/normalmap_wrap_cases.py -- and not the
kernels: they pass on a tree without the feature.  What they establish is that the definition is the periodic normal map (it
commutes with np.roll, it is the centre tile of a 3 x 3 tiling), that it differs from the reference's reflected borders where it
should (the outermost ring) and nowhere else.  tests/test_gpu_normalmap_wrap.py holds the kernels to this definition."""
import numpy as np
import pytest

import normalmap_wrap_cases as wc

SHAPES = [(37, 52), (5, 7), (64, 64)]
CASES = [(dt, o) for dt in (np.uint16, np.float64) for o in wc.OPTIONS] + [(np.float32, o) for o in wc.OPTIONS_F32]
IDS = ["%s-%d-%d-%d" % ((np.dtype(dt).name,) + o) for dt, o in CASES]


@pytest.mark.parametrize("dtype,opt", CASES, ids=IDS)
def test_definition_is_roll_equivariant(oracle, dtype, opt):
    nm = oracle.create_normalmap_array
    for h, w in SHAPES:
        d = wc.depth(h, w, dtype, seed=h * 100 + w)
        shift = (3, w - 2)
        a = wc.wrap_by_definition(nm, np.roll(d, shift, axis=(0, 1)), *opt)
        b = np.roll(wc.wrap_by_definition(nm, d, *opt), shift, axis=(0, 1))
        assert a.shape == (h, w, 3) and a.dtype == np.uint8
        assert np.array_equal(a, b), (h, w)


@pytest.mark.parametrize("dtype,opt", CASES, ids=IDS)
def test_definition_is_the_centre_tile_of_a_3x3_tiling(oracle, dtype, opt):
    nm = oracle.create_normalmap_array
    r = wc.radius(*opt)
    ran = 0
    for h, w in SHAPES:
        if h < r or w < r:
            continue                      # the tiling reaches one image far: a radius above the image size needs the modulo itself
        d = wc.depth(h, w, dtype, seed=h * 100 + w + 1)
        tiled = wc.plain(nm, np.tile(d, (3, 3)), *opt)
        assert np.array_equal(wc.wrap_by_definition(nm, d, *opt), tiled[h:2 * h, w:2 * w]), (h, w)
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize("dtype,opt", CASES, ids=IDS)
def test_definition_equals_the_reflected_result_away_from_the_border(oracle, dtype, opt):
    nm = oracle.create_normalmap_array
    r = wc.radius(*opt)
    ran = 0
    for h, w in SHAPES:
        if h <= 2 * r or w <= 2 * r:
            continue                      # no pixel is R away from every border
        d = wc.depth(h, w, dtype, seed=h * 100 + w + 2)
        a, b = wc.wrap_by_definition(nm, d, *opt), wc.plain(nm, d, *opt)
        assert np.array_equal(a[r:h - r, r:w - r], b[r:h - r, r:w - r]), (h, w)
        ran += 1
    assert ran >= 1


@pytest.mark.parametrize("opt", [(0, 3, 0), (5, 3, 5), (0, 0, 0)], ids=["sobel3", "blur5-sobel3-blur5", "gradient"])
def test_reflected_borders_break_the_outermost_ring_of_a_periodic_map(oracle, opt):
    nm = oracle.create_normalmap_array
    d = wc.smooth_periodic(48, 64)
    a, b = wc.wrap_by_definition(nm, d, *opt), wc.plain(nm, d, *opt)
    ring = wc.ring_mask(48, 64)
    assert ring.sum() == 220
    differ = (a != b).any(axis=2)[ring].sum()
    assert differ >= 0.95 * 220, differ
