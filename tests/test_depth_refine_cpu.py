"""Depth refinement without a GPU: the parameter check and the table builder of src/_native.py, and what the DEFINITION
(include/depthstereo.h: ds_joint_bilateral_u16) is good for, shown on its float64 NumPy model (tests/depth_refine_cases.py) alone.
tests/test_gpu_depth_refine.py holds the kernel to that model bit for bit."""
import numpy as np
import pytest

import depth_refine_cases as rc


def test_params_accepts_and_rejects():
    from src import _native
    p = _native.depth_refine_params
    assert p((9, 25.0, 3.0)) == (9, 25.0, 3.0, 1) and p([15, 25, 5, 4]) == (15, 25.0, 5.0, 4)
    assert p((3, 1e-3, 1e-3, 1)) == (3, 1e-3, 1e-3, 1) and p((31, 1e9, 1e9, 8)) == (31, 1e9, 1e9, 8)
    assert p((np.int64(5), np.float32(2.0), 1, np.int32(2))) == (5, 2.0, 1.0, 2) and p((5.0, 1, 1, 2.0)) == (5, 1.0, 1.0, 2)
    out = p((7, 3, 2))
    assert [type(v) for v in out] == [int, float, float, int]
    for bad in ((4, 1, 1), (33, 1, 1), (1, 1, 1), (5.5, 1, 1), (5, 0.0, 1), (5, 1, 0.0), (5, -1.0, 1), (5, float('inf'), 1),
                (5, 1, float('nan')), (5, 1.0), (5,), (), (5, 1, 1, 1, 1), (5, 1, 1, 0), (5, 1, 1, 9), (5, 1, 1, 1.5), (5, 1, 1, True),
                (5, 1, 1, None), (True, 1, 1), (5, "x", 1), "5", "511", 5, None):
        with pytest.raises(ValueError):
            p(bad)


@pytest.mark.parametrize("params", [(3, 3.0, 1.0), (9, 300.0, 2.5), (15, 40.0, 5.0), (31, 25.0, 9.0), (9, 0.05, 2.5)])
def test_tables_equal_the_models_bit_for_bit(params):
    from src import _native
    ws, wc = _native.depth_refine_tables(*params)
    mws, mwc = rc.tables(*params)
    d = params[0]
    assert ws.dtype == np.float64 and wc.dtype == np.float64 and ws.shape == (d * d,) and wc.shape == (766,)
    assert np.array_equal(ws.view(np.uint64), mws.ravel().view(np.uint64)) and np.array_equal(wc.view(np.uint64), mwc.view(np.uint64))
    r = d // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    assert np.array_equal(ws.reshape(d, d) == 0.0, dx * dx + dy * dy > r * r)                              # exactly 0 outside the circle only
    assert wc[0] == 1.0 and ws[(d * d) // 2] == 1.0
    if params[1] == 0.05:
        # exp(-200) = 1.4e-87 at k = 1, far below half an ulp of the centre tap's weight 1; from k = 2 on (exp(-800)) exactly 0
        assert 0.0 < wc[1] < 1e-80 and not wc[2:].any()


def test_flat_depth_stays_flat_under_any_guide():
    for _, g in rc.guide_cases(13, 21, seed=3):
        for level in (0, 1, 12345, 65535):
            d = np.full((13, 21), level, np.uint16)
            for wrap in (False, True):
                assert np.array_equal(rc.model(d, g, (9, 25.0, 3.0), wrap), d), (level, wrap)
                assert np.array_equal(rc.model(d, g, (5, 300.0, 2.0, 3), wrap), d), (level, wrap)


def test_constant_guide_gives_the_plain_circular_gaussian_average():
    h, w, d, ss = 11, 17, 7, 2.0
    r = d // 2
    g = rc.constant_guide(h, w)
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    ws = np.where(dx * dx + dy * dy <= r * r, np.exp(-(dx * dx + dy * dy) / (2.0 * ss * ss)), 0.0)
    for name, dep in rc.depth_cases(h, w, seed=8):
        for wrap in (False, True):
            pad = np.pad(dep, r, mode='wrap' if wrap else 'reflect').astype(np.float64)
            avg = sum(ws[j, i] * pad[j:j + h, i:i + w] for j in range(d) for i in range(d)) / ws.sum()
            got = rc.model(dep, g, (d, 25.0, ss), wrap)
            # the model sums in its own order; the plain average agrees to a rounding of the last level
            assert np.abs(got.astype(np.float64) - avg).max() <= 0.5 + 1e-6, (name, wrap)
            # and sigma_color does not matter under a constant guide: wc[0] == 1 is the only entry read
            assert np.array_equal(got, rc.model(dep, g, (d, 0.05, ss), wrap)), (name, wrap)


def test_output_lies_within_the_windows_min_and_max():
    h, w, d = 12, 19, 7
    r = d // 2
    for _, g in rc.guide_cases(h, w, seed=5):
        for name, dep in rc.depth_cases(h, w, seed=6):
            for wrap in (False, True):
                pad = np.pad(dep, r, mode='wrap' if wrap else 'reflect')
                win = np.lib.stride_tricks.sliding_window_view(pad, (d, d))
                got = rc.model(dep, g, (d, 40.0, 2.0), wrap)
                assert (got >= win.min(axis=(2, 3))).all() and (got <= win.max(axis=(2, 3))).all(), (name, wrap)


def test_tiny_sigma_color_averages_only_taps_of_identical_colour():
    """sigma_color = 0.05: wc[1] = 1.4e-87 vanishes beside the centre tap's weight 1 and wc[k >= 2] is exactly 0, so a pixel is the
    spatially weighted mean of the taps whose colour equals its own."""
    h, w, d, ss = 10, 14, 5, 1.5
    r = d // 2
    rng = np.random.default_rng(17)
    g = rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 200                 # eight colours: identical colours do occur in a window
    dep = rc.random_depth(h, w, seed=18)
    ws, _ = rc.tables(d, 1.0, ss)
    got = rc.model(dep, g, (d, 0.05, ss))
    pad, gpad = np.pad(dep, r, mode='reflect').astype(np.float64), np.pad(g, ((r, r), (r, r), (0, 0)), mode='reflect')
    multi = 0
    for y in range(h):
        for x in range(w):
            same = (gpad[y:y + d, x:x + d] == g[y, x]).all(axis=2) & (ws != 0.0)
            multi += same.sum() > 1
            want = (ws[same] * pad[y:y + d, x:x + d][same]).sum() / ws[same].sum()
            assert abs(float(got[y, x]) - want) <= 0.5 + 1e-6, (y, x)
    assert multi > h * w // 2                                               # (the scene does exercise the averaging)
    # white noise guide: no two taps alike, the map comes back untouched
    assert np.array_equal(rc.model(dep, rc.noise_guide(h, w, seed=19), (d, 0.05, ss)), dep)


def test_silhouette_one_pass_puts_the_largest_step_at_the_colour_edge():
    depth, guide = rc.silhouette_scene()
    edge = 32
    before = rc.row_steps(depth)
    assert 3333 <= before.max() <= 3334 and int(np.argmax(before)) != edge - 1
    after = rc.row_steps(rc.model(depth, guide, (9, 25.0, 3.0)))
    print("input largest step", before.max(), "; after one pass: at the edge", after[edge - 1], ", elsewhere", np.delete(after, edge - 1).max())
    assert int(np.argmax(after)) == edge - 1                               # between columns 31 and 32
    assert after[edge - 1] >= 3 * before.max()


def test_silhouette_four_passes_flatten_every_other_step():
    depth, guide = rc.silhouette_scene()
    edge = 32
    before = rc.row_steps(depth)
    out = rc.model(depth, guide, (15, 25.0, 5.0, 4))
    after = rc.row_steps(out)
    print("input largest step", before.max(), "; after four passes: at the edge", after[edge - 1], ", elsewhere", np.delete(after, edge - 1).max())
    assert int(np.argmax(after)) == edge - 1
    assert np.delete(after, edge - 1).max() < before.max() / 2
    mid = out[out.shape[0] // 2]
    assert mid[0] == 10000 and mid[-1] == 50000                             # the plateaus stay
