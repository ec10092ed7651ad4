"""Eight paths and the speckle filter without a GPU: what the definitions (include/depthstereo.h, ds_stereo_match_ex_u8 and
ds_speckle_filter_i16) promise, shown on their NumPy model (tests/stereo_match_ex_cases.py); the guards that keep
tests/test_gpu_stereo_match_ex.py and tests/test_gpu_speckle_filter.py from passing vacuously -- every eight-path case has a disparity
plane that differs from its four-path one, every filtered case has a component removed and one kept, the sizes sit on a component's
count and on that count minus 1 --; and the validators, value by value."""
import numpy as np
import pytest

import stereo_match_cases as sc
import stereo_match_ex_cases as ex


def test_model_ex_with_four_paths_and_no_filter_is_the_model():
    for shape in sc.SMALL_SHAPES:
        for name in sc.INPUTS:
            l, r = sc.pair(name, shape)
            for a, b in zip(sc.model(l, r), ex.model_ex(l, r, paths=4, speckle_size=0, speckle_range=3)):
                assert a.dtype == b.dtype and np.array_equal(a, b), (shape, name)
    l, r = sc.pair("planes", (2, 9, 130), 1)
    params = (32, -7, 64, 255, 25, 0)
    assert all(np.array_equal(a, b) for a, b in zip(sc.model(l, r, *params), ex.model_ex(l, r, *params)))


def test_diagonal_paths_of_one_row_or_one_column_equal_the_cost():
    rng = np.random.default_rng(3)
    for shape in ((1, 67, 32), (5, 1, 32), (1, 1, 64)):
        C = rng.integers(0, 25, shape).astype(np.int64)
        for dy, dx in ex.DIAGONALS:
            assert np.array_equal(ex.diagonal_path(C, 4, 48, dy, dx), C), (shape, dy, dx)
        assert np.array_equal(ex.aggregate(C, 4, 48, 8), sc.aggregate(C, 4, 48) + 4 * C)


def test_diagonal_path_restarts_where_the_predecessor_is_outside_and_is_a_vertical_path_along_its_line():
    """A diagonal line read off into a one-column image must give that column's vertical path: the recurrence is the same, only the
    set of pixels on a line changes."""
    rng = np.random.default_rng(4)
    h, w, D = 7, 5, 32
    C = rng.integers(0, 25, (h, w, D)).astype(np.int64)
    for dy, dx in ex.DIAGONALS:
        L = ex.diagonal_path(C, 3, 20, dy, dx)
        for y0 in range(h):
            for x0 in range(w):
                if 0 <= y0 - dy < h and 0 <= x0 - dx < w:
                    continue                                                  # not the first pixel of its path
                assert np.array_equal(L[y0, x0], C[y0, x0])
                pts = []
                y, x = y0, x0
                while 0 <= y < h and 0 <= x < w:
                    pts.append((y, x))
                    y, x = y + dy, x + dx
                line = np.stack([C[p] for p in pts])[:, None, :]              # [len, 1, D]: a one-column image
                want = sc.path(line, 3, 20, 0, False)[:, 0]
                assert np.array_equal(np.stack([L[p] for p in pts]), want), (dy, dx, y0, x0)


def test_eight_path_cases_differ_from_their_four_path_planes():
    for name, shape, params in ex.EIGHT_PATH_CASES:
        four, eight = ex.want(name, shape, 3, params, (4, 0, 0)), ex.want(name, shape, 3, params, (8, 0, 0))
        assert int((four[0] != eight[0]).sum()) > 100, (name, shape)
        assert all(np.array_equal(a, b) for a, b in zip(four, sc.want(name, shape, 3, params)))
    # and so do the parametrised shapes that have diagonals longer than 1, at every D
    differing = set()
    for shape in ex.EX_SHAPES:
        for row, e in ex.EX_PARAMS:
            if e[0] == 8 and min(shape[1:]) > 1 and not np.array_equal(ex.want("planes", shape, row[6], row[:6], (8, 0, 0))[0],
                                                                        sc.want("planes", shape, row[6], row[:6])[0]):
                differing.add((shape, row[0]))
    for shape in ((1, 7, 20), (2, 9, 130), (1, 33, 257), (1, 67, 5)):
        assert any((shape, D) in differing for D in (32, 64, 128)), shape
    assert {D for _, D in differing} == {32, 64, 128}


def test_the_components_the_cases_were_chosen_for():
    name, shape, params = ex.PLANES_EX
    four = ex.component_sizes(ex.sizes_of(name, shape, params, 4, 1)[0])
    eight = ex.component_sizes(ex.sizes_of(name, shape, params, 8, 1)[0])
    assert four == [1] * 10 + [2, 764, 3808] and eight == [1] * 8 + [2, 2, 2, 4, 719, 3845]
    name, shape, params = ex.STRIPES_EX
    four = ex.component_sizes(ex.sizes_of(name, shape, params, 4, 1)[0])
    eight = ex.component_sizes(ex.sizes_of(name, shape, params, 8, 1)[0])
    assert len(four) == 1285 and len(eight) == 1680 and four[0] == eight[0] == 1 and four[-1] == 1314 and eight[-1] == 1385
    assert sum(1 for v in four if 9 <= v <= 50) >= 3 and sum(1 for v in eight if 9 <= v <= 50) >= 3
    noise = ex.component_sizes(ex.sizes_of("noise", shape, params, 8, 1)[0])
    assert max(noise) <= 70                                                   # `noise` keeps nothing from size 70 on: not a filter case


def test_every_filtered_case_removes_a_component_and_keeps_one():
    on_a_count = below_a_count = 0
    for name, shape, params, paths, rng, sizes in ex.SPECKLE_CASES:
        present = set()
        for z in ex.sizes_of(name, shape, params, paths, rng):
            present |= set(ex.component_sizes(z))
        for size in sizes:
            if size == 65535:
                assert max(present) <= size
                continue
            assert min(present) <= size < max(present), (name, paths, size)   # one goes, one stays
            on_a_count += size in present
            below_a_count += size + 1 in present
            off, on = ex.want(name, shape, 3, params, (paths, 0, 0)), ex.want(name, shape, 3, params, (paths, size, rng))
            assert not np.array_equal(off[1], on[1]) and on[1].any(), (name, paths, size)
            assert int((off[1] != on[1]).sum()) == sum(v for z in ex.sizes_of(name, shape, params, paths, rng)
                                                       for v in ex.component_sizes(z) if v <= size)
    assert on_a_count >= 6 and below_a_count >= 6


def test_the_filter_patterns_are_what_their_names_say():
    t = ex.PATTERN_T
    for shape in ex.SPECKLE_SHAPES:
        n, h, w = shape
        for name in ex.PATTERNS:
            disp, valid = ex.pattern(name, shape)
            assert disp.dtype == np.int16 and valid.dtype == np.uint8 and disp.shape == valid.shape == shape
        z = ex.pattern_sizes("constant", shape)
        assert (z == h * w).all()
        z = ex.pattern_sizes("checkerboard", shape)
        assert set(np.unique(z)) <= {0, 1} and int(z.sum()) == n * ((h * w + 1) // 2)
        z, (_, v) = ex.pattern_sizes("serpentine", shape), ex.pattern("serpentine", shape)
        assert (z[v != 0] == int(v[0].sum())).all() and (z[v == 0] == 0).all()         # one component: every valid pixel
        z, (_, v) = ex.pattern_sizes("spiral", shape), ex.pattern("spiral", shape)
        assert (z[v != 0] == int(v[0].sum())).all() and int(v[0].sum()) >= (h * w) // 2
        z, (_, v) = ex.pattern_sizes("comb", shape), ex.pattern("comb", shape)
        assert (z[v != 0] == int(v[0].sum())).all()
        assert (ex.pattern_sizes("ramp_t", shape) == h * w).all() and (ex.pattern_sizes("ramp_t1", shape) == 1).all()
        d, _ = ex.pattern("extremes", shape)
        z = ex.pattern_sizes("extremes", shape)
        assert z.max() <= 2 * min(h, 2) or h * w == 1                         # pairs and short columns, never one 16-bit-wrapped blob
        if w >= 4:
            assert d.min() == -32768 and d.max() == 32767 and z.max() < h * w
        z, (_, v) = ex.pattern_sizes("borders", shape), ex.pattern("borders", shape)
        assert (z[v != 0] == int(v[0].sum())).all()                           # per image: nothing of the neighbour image is counted
    # the mixed case: the random pattern has components on both sides of the sizes the GPU test uses
    z = ex.component_sizes(ex.pattern_sizes("random", (1, 33, 257))[0])
    assert z[0] == 1 and z[-1] > 40 and any(2 <= v <= 8 for v in z)
    # the serpentine's diameter: about half the pixels
    _, v = ex.pattern("serpentine", (1, 33, 257))
    assert int(v.sum()) > 33 * 257 // 2
    assert t == 5


def test_flood_fill_on_a_hand_made_map():
    disp = np.array([[0, 5, 10, 99], [50, 50, 16, 99], [0, 0, 0, 0]], np.int16)
    valid = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 0, 1, 1]], np.uint8)
    z = ex.speckle_sizes(disp, valid, 5)
    #  0-5-10 is a ramp in steps of t: one component of 3; 16 below 10 differs by 6: apart; 50, 50: a pair; 99 alone; the last row is cut
    #  by its invalid pixel into 1 and 2
    assert z.tolist() == [[3, 3, 3, 1], [2, 2, 1, 0], [1, 0, 2, 2]]
    out, sizes = ex.speckle_filter(disp[None], valid[None], 2, 5)
    assert out[0].tolist() == [[1, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and sizes.dtype == np.uint32 and np.array_equal(sizes[0], z)
    assert ex.speckle_filter(disp[None], valid[None], 1, 5)[0][0].tolist() == [[1, 1, 1, 0], [1, 1, 0, 0], [0, 0, 1, 1]]


def test_ex_validator_accepts_and_rejects():
    from src import _native
    V = _native.stereo_match_ex_params
    assert V((4, 0, 0)) == (4, 0, 0) == _native.STEREO_MATCH_EX_DEFAULTS and V([8, 64, 1]) == (8, 64, 1) == _native.STEREO_MATCH_EX_PRESET
    assert V((8, 65535, 16)) == (8, 65535, 16) and V((np.int64(8), np.uint16(9), 2.0)) == (8, 9, 2)
    assert [type(v) for v in V((4.0, 1.0, np.float32(0.0)))] == [int] * 3
    nan, inf = float('nan'), float('inf')
    for bad in ((0, 0, 0), (2, 0, 0), (5, 0, 0), (16, 0, 0), (-8, 0, 0), (True, 0, 0), ('8', 0, 0), (None, 0, 0), (nan, 0, 0), (inf, 0, 0),
                (8.5, 0, 0), (b'8', 0, 0),
                (8, -1, 0), (8, 65536, 0), (8, True, 0), (8, '64', 0), (8, nan, 0), (8, 0.5, 0), (8, None, 0), (8, inf, 0),
                (8, 64, -1), (8, 64, 17), (8, 64, False), (8, 64, '1'), (8, 64, nan), (8, 64, 1.5), (8, 64, None),
                (), (8,), (8, 64), (8, 64, 1, 0), "864", b"abc", 8, None, {8: 64}):
        with pytest.raises(ValueError):
            V(bad)


def test_public_validators_of_paths_and_speckle():
    import src.stereo_matching as sm
    P = sm._ex_params
    assert P(4, None, "t") == (4, 0, 0) and P(8, (64, 1), "t") == (8, 64, 1) and P(8, [1, 0], "t") == (8, 1, 0) and P(4, (0, 5), "t") == (4, 0, 5)
    for paths, speckle in ((6, None), (True, None), ("8", None), (None, None), (8, 64), (8, (64,)), (8, (64, 1, 0)), (8, "64"), (8, (64, 17)),
                           (8, (65536, 1)), (8, (True, 1)), (8, (64, float('nan'))), (8, (-1, 1)), (8, {}), (8, (None, 1))):
        with pytest.raises(ValueError):
            P(paths, speckle, "t")
