"""The 3D-photo depth preparation without a GPU: the NumPy model of tests/sparse_bilateral_cases.py against what the REFERENCE's
sparse_bilateral_filtering returned on the same seeded inputs (tests/golden/sparse_bilateral_cases.npz), bit for bit; the rank table
the kernel is given; and the host half of the drop-in module (what it refuses, it refuses before any device work)."""
import os

import numpy as np
import pytest

import sparse_bilateral_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_bilateral_cases.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_model_equals_the_reference_bit_for_bit(golden):
    seen = 0
    for name, (depth, image, config, num_iter) in sc.cases().items():
        images, depths = sc.model(depth, image, sc.windows_of(config, num_iter), config['depth_threshold'])
        assert len(images) == len(depths) == num_iter
        for i in range(num_iter):
            assert _same_bits(depths[i], golden[f"{name}__depth{i}"]), (name, i)
            assert images[i].dtype == np.uint8 and np.array_equal(images[i], golden[f"{name}__image{i}"]), (name, i)
            seen += 2
        assert f"{name}__depth{num_iter}" not in golden
    assert seen == len(golden)                                                # every golden array was compared
    assert _same_bits(golden["33x70_steps__depth0"], sc.cases()["33x70_steps"][0])
    assert not _same_bits(golden["33x70_steps__depth1"], golden["33x70_steps__depth0"])          # the passes do something
    assert (golden["33x70_steps__image0"] == 0).all(axis=2).any()


def test_cases_meet_every_rank_that_is_not_half(golden):
    seen = sc.census_of_all_cases()
    rank = sc.rank_table()
    assert set(sc.ODD_RANKS_TO_49) <= seen and 0 in seen
    assert any(n > 49 and rank[n] != n // 2 for n in seen)
    assert sc.census_is_complete(seen)


def test_rank_table_is_the_recipe_and_not_half():
    from src import _native
    rank = _native.sparse_bilateral_rank_table()
    assert rank.dtype == np.int32 and rank.shape == (226,) and rank[0] == 0
    for n in range(1, 226):
        c = np.ones(n, np.float32)
        assert rank[n] == np.digitize(0.5, np.cumsum(c / c.sum())), n
        assert 0 <= rank[n] < n
    assert np.array_equal(rank, sc.rank_table())
    differs = [n for n in range(226) if rank[n] != n // 2]
    assert tuple(n for n in differs if n <= 49) == sc.ODD_RANKS_TO_49
    assert len(differs) == 38
    assert np.array_equal(_native.sparse_bilateral_rank_table(49), rank[:50])


def test_window_lists():
    from src import _native
    assert _native.sparse_bilateral_windows([7, 7, 5, 5, 5]) == [7, 7, 5, 5, 5]
    assert _native.sparse_bilateral_windows((np.int64(15), 1)) == [15, 1]
    for bad in ([], [4], [17], [-3], [0], [7, 6], [True], [5.5], ["7"], "7", 7, None):
        with pytest.raises(ValueError):
            _native.sparse_bilateral_windows(bad)


def test_jump_map_follows_ieee():
    t = 0.04
    v = np.full((5, 6), 2.0, np.float32)
    v[2, 2] = 0.0                                                            # disparity inf beside finite ones: a jump for all five
    v[1, 4] = v[2, 4] = 0.0                                                  # inf - inf is NaN: those two do not see each other
    j = sc.jump_map(v, t)
    want = np.zeros((5, 6), bool)
    want[2, 2] = want[1, 2] = want[3, 2] = want[2, 1] = want[2, 3] = True
    want[1, 4] = want[2, 4] = want[3, 4] = want[1, 3] = True                  # (2, 3) already is; (0, 4) and the last column are ring
    assert np.array_equal(j, want)
    assert not sc.jump_map(np.full((3, 3), np.nan, np.float32), t).any()


def test_drop_in_module_refuses_on_the_host():
    """Everything the module refuses, it refuses before any device work: this test has no GPU."""
    from inpaint.bilateral_filtering import bilateral_filter, sparse_bilateral_filtering, vis_depth_discontinuity
    from src import _native
    depth, image, config, num_iter = sc.cases()["9x11_noise"]
    before = dict(_native.CALLS)
    with pytest.raises(NotImplementedError, match="mask"):
        sparse_bilateral_filtering(depth, image, config, num_iter=num_iter, mask=np.ones_like(depth))
    with pytest.raises(NotImplementedError, match="mask"):
        vis_depth_discontinuity(depth, config, mask=np.ones_like(depth))
    with pytest.raises(NotImplementedError, match="label"):
        vis_depth_discontinuity(depth, config, label=True)
    with pytest.raises(NotImplementedError, match="vis_diff"):
        vis_depth_discontinuity(depth, config, vis_diff=True)
    with pytest.raises(NotImplementedError, match="discontinuity_map"):
        bilateral_filter(depth, config)
    with pytest.raises(NotImplementedError, match="discontinuity_map"):
        bilateral_filter(depth, config, discontinuity_map=np.zeros_like(depth), window_size=3)
    E = _native.DepthStereoError
    for bad_depth in (depth.astype(np.float64), depth[None], depth[:2], depth[:, :2], depth.tolist()):
        with pytest.raises(E):
            sparse_bilateral_filtering(bad_depth, image, config, num_iter=num_iter)
    for bad_image in (image[:, :, :2], image[:-1], image.astype(np.float32), image[:, :, 0]):
        with pytest.raises(E):
            sparse_bilateral_filtering(depth, bad_image, config, num_iter=num_iter)
    for value in (-1.0, np.nan, np.inf):
        bad = depth.copy()
        bad[3, 4] = value
        with pytest.raises(E, match="finite"):
            sparse_bilateral_filtering(bad, image, config, num_iter=num_iter)
    for size in (4, 17, 0, -5, 7.5, [7, 4, 3], [7, 5, 17]):
        with pytest.raises(E, match="filter_size"):
            sparse_bilateral_filtering(depth, image, dict(config, filter_size=size), num_iter=num_iter)
    with pytest.raises(E, match="num_iter"):
        sparse_bilateral_filtering(depth, image, config, num_iter=num_iter + 1)
    with pytest.raises(E, match="num_iter"):
        sparse_bilateral_filtering(depth, image, config)                     # the reference's default, None, fails there too
    assert sparse_bilateral_filtering(depth, image, config, num_iter=0) == ([], [])
    assert dict(_native.CALLS) == before


def test_vis_depth_discontinuity_is_the_jump_map_in_four_parts():
    from inpaint.bilateral_filtering import vis_depth_discontinuity
    for name in ("33x70_steps", "12x17_ties_zeros", "3x3"):
        depth, _, config, _ = sc.cases()[name]
        overs = vis_depth_discontinuity(depth, config)
        assert len(overs) == 4 and all(o.dtype == np.float32 and o.shape == depth.shape for o in overs)
        assert all(set(np.unique(o)) <= {0.0, 1.0} for o in overs)
        assert np.array_equal(np.maximum.reduce(overs) > 0, sc.jump_map(depth, config['depth_threshold'])), name
    # each part looks at ONE neighbour: a lone low column is seen from its left by r_over and from its right by l_over
    d = np.full((5, 7), 2.0, np.float32)
    d[:, 3] = 1.0
    u, b, l, r = vis_depth_discontinuity(d, {'depth_threshold': 0.04})
    assert not u.any() and not b.any()
    assert np.array_equal(np.argwhere(l[2] > 0).ravel(), [3, 4]) and np.array_equal(np.argwhere(r[2] > 0).ravel(), [2, 3])
