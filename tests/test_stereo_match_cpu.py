"""Depth from stereo pairs without a GPU: what the definition (include/depthstereo.h, ds_stereo_match_u8) promises, shown on its NumPy
model (tests/stereo_match_cases.py); a census that keeps tests/test_gpu_stereo_match.py honest: the cases it runs must contain pixels
that fail each check, filled pixels, pixels the median changes and sub-pixel parts; and the product's host half (the validators, the
splitter)."""
import numpy as np
import pytest

import stereo_match_cases as sc


def test_validator_accepts_and_rejects():
    from src import _native
    V = _native.stereo_match_params
    assert V((64,)) == (64, 0, 4, 48, 5, 1) == _native.STEREO_MATCH_DEFAULTS
    assert V([128, -128]) == (128, -128, 4, 48, 5, 1) and V((32, 127, 1, 1)) == (32, 127, 1, 1, 5, 1)
    assert V((64, 0, 64, 255, 50)) == (64, 0, 64, 255, 50, 1) and V((64, 0, 64, 64, 0, -1)) == (64, 0, 64, 64, 0, -1)
    assert V((np.int64(32), np.int8(-7), 4.0, np.float32(48.0), np.uint8(25), 3)) == (32, -7, 4, 48, 25, 3)
    assert [type(v) for v in V((64.0, 0.0, 4.0, 48.0, 5.0, 1.0))] == [int] * 6
    nan, inf = float('nan'), float('inf')
    for bad in ((16,), (65,), (256,), (0,), (True,), ('64',), (None,), (nan,), (inf,), (64.5,), (b'64',),
                (64, -129), (64, 128), (64, True), (64, '0'), (64, nan), (64, 0.5), (64, None),
                (64, 0, 0, 48), (64, 0, 65, 255), (64, 0, 4, 3), (64, 0, 4, 256), (64, 0, True, 48), (64, 0, 4, nan), (64, 0, '4', 48),
                (64, 0, 4, 48, -1), (64, 0, 4, 48, 51), (64, 0, 4, 48, True), (64, 0, 4, 48, 5.5), (64, 0, 4, 48, nan),
                (64, 0, 4, 48, 5, -2), (64, 0, 4, 48, 5, 4), (64, 0, 4, 48, 5, False), (64, 0, 4, 48, 5, '1'), (64, 0, 4, 48, 5, nan),
                (), (64, 0, 4), (64, 0, 4, 48, 5, 1, 0), "64", b"ab", 64, None, {0: 64}):
        with pytest.raises(ValueError):
            V(bad)


def test_stereo_input_option_validator():
    import src.stereo_matching as sm
    assert sm.stereo_input_params(('left-right',)) == ('left-right', 64, 0, 4, 48, 5, 1)
    assert sm.stereo_input_params(['bottom-top', 32, -4]) == ('bottom-top', 32, -4, 4, 48, 5, 1)
    assert sm.stereo_input_params(('right-left', 128, 5, 1, 1, 0, -1)) == ('right-left', 128, 5, 1, 1, 0, -1)
    for bad in ('left-right', (), ('sbs',), (None,), (64,), ('left-right', 65), ('left-right', 64, 0, 4), ('top-bottom', True), None, 5,
                ('left-right', 64, 0, 4, 48, 5, 1, 0), (b'left-right',)):
        with pytest.raises(ValueError):
            sm.stereo_input_params(bad)


def test_split_stereo_pair_on_all_four_layouts():
    from PIL import Image
    import src.stereo_matching as sm
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (6, 10, 3), dtype=np.uint8)
    first_lr, second_lr, first_tb, second_tb = a[:, :5], a[:, 5:], a[:3], a[3:]
    for layout, want in (('left-right', (first_lr, second_lr)), ('right-left', (second_lr, first_lr)),
                         ('top-bottom', (first_tb, second_tb)), ('bottom-top', (second_tb, first_tb))):
        for image in (a, Image.fromarray(a), a[:, :, 0]):
            left, right = sm.split_stereo_pair(image, layout)
            ch = slice(0, 1) if isinstance(image, np.ndarray) and image.ndim == 2 else slice(None)
            assert isinstance(left, Image.Image) == isinstance(image, Image.Image)
            assert np.array_equal(np.asarray(left).reshape(want[0][:, :, ch].shape), want[0][:, :, ch]), layout
            assert np.array_equal(np.asarray(right).reshape(want[1][:, :, ch].shape), want[1][:, :, ch]), layout
    for image, layout in ((a[:, :9], 'left-right'), (a[:, :9], 'right-left'), (a[:5], 'top-bottom'), (a[:5], 'bottom-top'),
                          (Image.fromarray(a[:, :9]), 'left-right'), (Image.fromarray(a[:5]), 'bottom-top'), (a[:, :1], 'left-right')):
        with pytest.raises(ValueError):
            sm.split_stereo_pair(image, layout)
    assert sm.split_stereo_pair(a[:, :9], 'top-bottom')[0].shape == (3, 9, 3)  # only the split dimension must be even
    for layout in ('sbs', 'Left-Right', None, 0, b'left-right'):
        with pytest.raises(ValueError):
            sm.split_stereo_pair(a, layout)
    with pytest.raises(ValueError):
        sm.split_stereo_pair(np.zeros((4,), np.uint8), 'left-right')


def test_public_functions_refuse_bad_arguments_without_a_gpu():
    """The parameter and image checks of depth_from_stereo come before anything touches the device."""
    from src import _native
    import src.stereo_matching as sm
    l, r = (v[0] for v in sc.pair("planes", (1, 7, 20)))
    for bad in ({'max_disparity': 48}, {'max_disparity': True}, {'min_disparity': 128}, {'p1': 0}, {'p1': 8, 'p2': 7}, {'p2': 256},
                {'uniqueness': 51}, {'uniqueness': float('nan')}, {'lr_check': 4}, {'lr_check': '1'}):
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo(l, r, **bad)
    for bad_l, bad_r in ((l.astype(np.float32), r), (l, r.astype(np.int16)), (l, r[:, :19]), (l[:, :, :2], r[:, :, :2]), (l[:0], r[:0]), (l[None], r[None]),
                         (l, r[:, :, :1])):
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo(bad_l, bad_r)


def _planes():
    shape, params = sc.PLANES_CASE
    l, r = sc.pair("planes", shape)
    _, h, w = shape
    y0, y1, x0, x1 = sc.planes_rect(h, w)
    assert (y1 - y0, x1 - x0) == (20, 40)
    yy, xx = np.mgrid[0:h, 0:w]
    rect = (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
    # the background the rectangle hides from the right eye: its right-image column x - 2 lies under the rectangle there, x1 - 9 > x - 2 >= x0 - 9
    band = (yy >= y0) & (yy < y1) & (xx >= x0 - (sc.PLANES_FG - sc.PLANES_BG)) & (xx < x0)
    return l[0], r[0], params, rect, band


def _grow(mask, r):
    out = np.zeros_like(mask)
    P = np.pad(mask, r)
    h, w = mask.shape
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= P[dy:dy + h, dx:dx + w]
    return out


def test_planes_are_found_away_from_edges_and_occlusions():
    """40 x 120, D = 32, d0 = -4, the defaults otherwise: every pixel 4 or more pixels away from the rectangle's edge, the image border
    and the occluded band is valid, and its disparity, rounded to whole pixels, is the truth."""
    l, r, params, rect, band = _planes()
    o = sc.match_one(l, r, *params)
    h, w = rect.shape
    yy, xx = np.mgrid[0:h, 0:w]
    border = (yy < 4) | (yy >= h - 4) | (xx < 4) | (xx >= w - 4)
    edge = _grow(rect, 4) & _grow(~rect, 4)                                   # within 4 pixels of the rectangle's outline, either side
    sel = ~border & ~edge & ~_grow(band, 4)
    truth = np.where(rect, sc.PLANES_FG, sc.PLANES_BG)
    assert int((sel & rect).sum()) >= 300 and int((sel & ~rect).sum()) >= 1500
    assert (o["valid"][sel] == 1).all()
    assert (((o["disp16"] + 8) >> 4)[sel] == truth[sel]).all()
    assert o["frac"].min() >= -8 and o["frac"].max() <= 8
    # and the three outputs agree with it there: the median and the fill leave these pixels within a sixteenth-rounding of the truth
    assert (((o["disparity"].astype(np.int64) + 8) >> 4)[sel] == truth[sel]).all()
    inner_bg, inner_fg = sel & ~rect, sel & rect
    assert o["depth"][inner_fg].min() > o["depth"][inner_bg].max()           # white = near


def test_each_check_switches_on_in_the_occluded_band():
    l, r, params, rect, band = _planes()
    D, d0, P1, P2, u, lr = params
    share = {}
    for key, (uu, ll) in {"defaults": (u, lr), "uniqueness only": (u, -1), "no check": (0, -1)}.items():
        share[key] = float((sc.match_one(l, r, D, d0, P1, P2, uu, ll)["valid"][band] == 0).mean())
    assert share["no check"] == 0.0
    assert share["defaults"] > share["uniqueness only"] > 0.0, share
    assert share["defaults"] > 0.5, share


def test_flat_images_take_the_smallest_disparity_everywhere():
    l, r = sc.pair("flat", (1, 12, 40))
    o = sc.match_one(l[0], r[0], **sc.DEFAULTS)
    assert (o["dstar"] == 0).all() and (o["frac"] == 0).all() and (o["valid"] == 1).all()
    assert (o["disparity"] == 0).all() and (o["depth"] == 0).all()
    for D in (32, 128):
        o = sc.match_one(l[0], r[0], D, 0, 1, 1, 50, 3)
        assert (o["dstar"] == 0).all() and (o["depth"] == 0).all()


def test_a_periodic_texture_fails_uniqueness():
    assert sc.STRIPES_PERIOD < min(32, sc.DEFAULTS["D"])
    l, r = sc.pair("stripes", (1, 12, 80))
    strict = sc.census(l[0], r[0], 64, 0, 4, 48, 25, 1)
    off = sc.census(l[0], r[0], 64, 0, 4, 48, 0, -1)
    assert strict["uniqueness"] >= 1, strict
    assert off["uniqueness"] == 0 and off["left_right"] == 0 and off["filled"] == 0, off


def test_the_gpu_cases_contain_what_they_claim_to_test():
    """Every entry of census is >= 1 on at least one case tests/test_gpu_stereo_match.py compares (small shape x parameter row, c as
    in the row), so its comparisons cannot pass vacuously."""
    best = dict(uniqueness=0, left_right=0, filled=0, median=0, frac=0)
    for shape in ((3, 5, 67), (2, 9, 130)):
        for D, d0, P1, P2, u, lr, c in sc.SMALL_PARAMS[:3] + sc.SMALL_PARAMS[5:6] + sc.SMALL_PARAMS[8:9]:
            for name in ("planes", "noise", "stripes"):
                l, r = sc.pair(name, shape, c)
                got = sc.census(l[0], r[0], D, d0, P1, P2, u, lr)
                best = {k: max(best[k], got[k]) for k in best}
    assert all(v >= 1 for v in best.values()), best
    shape, params, c = sc.LARGE_CASES[0]
    l, r = sc.pair("planes", shape, c)
    got = sc.census(l[0], r[0], *params)
    assert all(v >= 1 for v in got.values()), got


def test_an_image_alone_equals_its_slice_of_a_batch():
    shape = (3, 5, 67)
    l, r = sc.pair("planes", shape)
    l2, r2 = np.array(l), np.array(r)
    l2[1], r2[1] = sc.pair("noise", shape)[0][1], sc.pair("noise", shape)[1][1]
    whole = sc.model(l2, r2, 32, -7, 4, 48, 5, 1)
    for k in range(3):
        alone = sc.model(l2[k:k + 1], r2[k:k + 1], 32, -7, 4, 48, 5, 1)
        assert all(np.array_equal(a[0], b[k]) for a, b in zip(alone, whole)), k
    assert not np.array_equal(whole[0][0], whole[0][1])


def test_the_depth_rule():
    v = np.array([[-70, -70, 0, 5], [1, 2, 3, 4064]], np.int16)
    d = sc.depth_rule(v)
    assert d.dtype == np.uint16 and d[0, 0] == 0 and d[1, 3] == 65535
    order = np.argsort(v.ravel(), kind="stable")
    assert (np.diff(d.ravel()[order].astype(np.int64)) >= 0).all()            # monotone
    lo, hi = -70, 4064
    for x, got in zip(v.ravel().tolist(), d.ravel().tolist()):               # the half-up rounding of (v - lo) 65535 / (hi - lo)
        assert abs(got * (hi - lo) - (x - lo) * 65535) * 2 <= hi - lo
    assert (sc.depth_rule(np.full((3, 4), -5, np.int16)) == 0).all()
    two = sc.depth_rule(np.array([[7, 8]], np.int16))
    assert two.tolist() == [[0, 65535]]
    # the model's depth output is this rule on its disparity output
    l, r = sc.pair("planes", (1, 7, 20))
    disparity, _, depth = sc.model(l, r, 32, 0, 4, 48, 5, 1)
    assert np.array_equal(depth[0], sc.depth_rule(disparity[0]))
