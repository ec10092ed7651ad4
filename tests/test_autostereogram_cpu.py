"""The autostereogram without a GPU: what the definition (include/depthstereo.h, ds_autostereogram_u8) promises, shown on its NumPy
model (tests/autostereogram_cases.py); a census that keeps tests/test_gpu_autostereogram.py honest: the cases it runs must contain
hidden columns and components of several members; and the product's host half (the validator, the separation)."""
import collections

import numpy as np
import pytest

import autostereogram_cases as ac


def test_validator_accepts_and_rejects():
    from PIL import Image
    from src import _native
    V = _native.autostereogram_params
    assert V((96, 1 / 3)) == (96, 85, 'dots', 0)
    assert V([16, 0.5, 'mono', 0xFFFFFFFF]) == (16, 128, 'mono', 4294967295)
    assert V((np.int64(512), np.float32(0.00390625), 'dots', np.uint32(7))) == (512, 1, 'dots', 7)
    assert V((96.0, 0.25, 'mono', 3.0)) == (96, 64, 'mono', 3) and [type(v) for v in V((96.0, 0.25, 'mono', 3.0))] == [int, int, str, int]
    assert V((96, 0.002))[1] == 1 and V((96, 0.5019))[1] == 128              # rint(256 mu): 0.512 -> 1, 128.49 -> 128
    tile = np.arange(2 * 5 * 3, dtype=np.uint8).reshape(2, 5, 3)
    got = V((64, 0.3, tile))
    assert got[:2] == (64, 77) and got[3] == 0 and got[2].dtype == np.uint8 and got[2].flags['C_CONTIGUOUS'] and np.array_equal(got[2], tile)
    assert np.array_equal(V((64, 0.3, tile[:, :, 0]))[2], np.repeat(tile[:, :, :1], 3, axis=2))             # grey: three equal channels
    assert np.array_equal(V((64, 0.3, np.dstack([tile, tile[:, :, :1]])))[2], tile)                         # RGBA: the alpha is dropped
    assert np.array_equal(V((64, 0.3, Image.fromarray(tile)))[2], tile)
    assert np.array_equal(V((64, 0.3, Image.fromarray(np.ascontiguousarray(tile[:, :, 0]))))[2], np.repeat(tile[:, :, :1], 3, axis=2))
    assert V((64, 0.3, np.zeros((4096, 1, 3), np.uint8)))[2].shape == (4096, 1, 3)
    nan, inf = float('nan'), float('inf')
    for bad in ((15, 0.3), (513, 0.3), (True, 0.3), (96.5, 0.3), ('96', 0.3), (None, 0.3), (nan, 0.3), (inf, 0.3), (b'96', 0.3),
                (96, 0.0), (96, 0.0019), (96, 0.503), (96, -0.3), (96, 1.0), (96, nan), (96, inf), (96, True), (96, '0.3'), (96, None), (96, 33),
                (96, 0.3, 'stripes'), (96, 0.3, None), (96, 0.3, b'dots'), (96, 0.3, 5), (96, 0.3, np.zeros((2, 5, 3), np.float32)),
                (96, 0.3, np.zeros((2, 5, 2), np.uint8)), (96, 0.3, np.zeros((5,), np.uint8)), (96, 0.3, np.zeros((0, 5, 3), np.uint8)),
                (96, 0.3, np.zeros((2, 4097, 3), np.uint8)), (96, 0.3, np.zeros((4097, 1), np.uint8)), (96, 0.3, np.zeros((2, 2, 3, 1), np.uint8)),
                (96, 0.3, 'dots', -1), (96, 0.3, 'dots', 2**32), (96, 0.3, 'dots', True), (96, 0.3, 'dots', 1.5), (96, 0.3, 'dots', '1'),
                (96, 0.3, 'dots', None), (96, 0.3, 'dots', nan),
                (96,), (), (96, 0.3, 'dots', 0, 0), "dots", b"ab", 96, None, {0: 96, 1: 0.3}):
        with pytest.raises(ValueError):
            V(bad)


def test_public_functions_refuse_bad_arguments_without_a_gpu():
    """The parameter and depth-map checks of create_autostereogram come before anything touches the device."""
    from src import _native
    import src.autostereogram_generation as ag
    d = ac.depth_input("rect", (3, 5, 67))[0]
    for bad in ({'period': 15}, {'period': True}, {'depth_factor': 0.6}, {'depth_factor': float('nan')}, {'pattern': 'stripes'},
                {'pattern': np.zeros((2, 2, 3), np.int16)}, {'seed': -1}, {'seed': 2**32}):
        with pytest.raises(_native.DepthStereoError):
            ag.create_autostereogram(d, **bad)
    for bad_depth in (d.astype(np.float32), d.astype(np.int32), d.astype(np.uint8), d.astype(np.int16), d[None], d[:0]):
        with pytest.raises(_native.DepthStereoError):
            ag.create_autostereogram(bad_depth)


@pytest.mark.parametrize("P,m", [(16, 128), (96, 85), (512, 1), (64, 128)])
def test_separation_starts_at_the_period_and_never_increases(P, m):
    from src import _native
    z = np.arange(65536)
    s = _native.autostereogram_separation(z, P, m)
    assert s.dtype == np.int64 and s[0] == P and (np.diff(s) <= 0).all() and s[-1] >= 1
    assert np.array_equal(s, ac.separation(z, P, m))
    # against exact integers: s is the half-up rounding of num / den
    for zz in (0, 1, 777, 32768, 65534, 65535):
        den, num = 2 * 256 * 65535 - m * zz, 2 * P * (256 * 65535 - m * zz)
        assert int(s[zz]) == (2 * num + den) // (2 * den) and abs(int(s[zz]) * den - num) * 2 <= den
    assert int(_native.autostereogram_separation(65535, P, m)) == int(s[-1])


def test_separation_example_of_the_definition():
    from src import _native
    assert _native.autostereogram_separation([0, 16384, 32768, 49152, 65535], 96, 85).tolist() == [96, 92, 87, 82, 77]


def test_pinned_hash_values():
    """lowbias32(seed ^ (y * 0x9E3779B1) ^ (rep * 0x85EBCA77)), computed once with plain Python integers."""
    pinned = {(0, 0, 0): 0x0, (0, 0, 1): 0xc4a0e45c, (0, 1, 0): 0x6d523710, (1, 0, 0): 0x688990c0, (0xDEADBEEF, 1079, 1919): 0x5650871c,
              (0xFFFFFFFF, 16383, 16383): 0x2ffdd6ea, (12345, 7, 300): 0x22b6b02}
    for (seed, y, rep), want in pinned.items():
        reps = np.full((y + 1, 1), rep, np.int64)
        rgb = ac.colours(reps, 0, seed)[y, 0]
        assert rgb.tolist() == [want & 255, (want >> 8) & 255, (want >> 16) & 255], (seed, y, rep)
        assert ac.colours(reps, 1, seed)[y, 0].tolist() == [255 * (want >> 31)] * 3, (seed, y, rep)


def test_a_flat_map_repeats_with_its_separation():
    for level in (0, 30000, 65535):
        for P, m in ((16, 128), (96, 85), (40, 1)):
            for invert in (False, True):
                flat = np.full((3, 200), level, np.uint16)
                s = int(ac.separation(65535 - level if invert else level, P, m))
                for mode, tile in ((0, None), (1, None), (2, ac.tile_input(1))):
                    out = ac.model(flat, P, m, mode, 5, tile, invert)
                    assert np.array_equal(out[:, :-s], out[:, s:]), (level, P, m, invert, mode)
                rep = ac.rep_map(flat, P, m, invert)
                assert sorted(rep[0, :s].tolist()) == list(range(200 - s, 200))                  # s components, their roots the last strip


def test_the_ends_of_every_offered_link_share_a_colour_on_random_maps():
    for seed in range(6):
        rng = np.random.default_rng(seed)
        w = int(rng.integers(200, 400))
        P, m = int(rng.integers(16, 120)), int(rng.integers(1, 129))
        # random walks: gentle ones (even seeds), on which nearly every link survives the visibility test, and rough ones
        step = 900 if seed % 2 == 0 else 6000
        depth = np.clip(np.cumsum(rng.integers(-step, step + 1, (4, w)), axis=1) + 30000, 0, 65535).astype(np.uint16)
        for invert in (False, True):
            out = ac.model(depth, P, m, 0, seed, None, invert)
            rep = ac.rep_map(depth, P, m, invert)
            offered_total = 0
            for y in range(4):
                l, r, offered = ac.links(ac.nearness(depth[y], invert), P, m)
                xs = np.flatnonzero(offered)
                offered_total += len(xs)
                assert np.array_equal(rep[y, l[xs]], rep[y, r[xs]])
                assert np.array_equal(out[y, l[xs]], out[y, r[xs]]), (seed, y)
            assert offered_total > 0, (seed, w, P, m)


def _brute_force_rep(z, P, m):
    """Breadth-first over the offered links: the largest column reachable from each column."""
    w = len(z)
    l, r, offered = ac.links(z, P, m)
    nb = collections.defaultdict(set)
    for x in np.flatnonzero(offered).tolist():
        nb[int(l[x])].add(int(r[x]))
        nb[int(r[x])].add(int(l[x]))
    rep = []
    for x in range(w):
        seen, queue = {x}, collections.deque([x])
        while queue:
            for v in nb[queue.popleft()]:
                if v not in seen:
                    seen.add(v)
                    queue.append(v)
        rep.append(max(seen))
    return np.array(rep)


def test_rep_is_the_breadth_first_maximum_on_short_rows():
    rng = np.random.default_rng(11)
    members = 0
    for trial in range(60):
        w = int(rng.integers(1, 41))
        P, m = int(rng.integers(16, 25)), int(rng.integers(1, 129))
        kind = trial % 3
        if kind == 0:
            row = rng.integers(0, 65536, w)
        elif kind == 1:
            row = np.clip(np.cumsum(rng.integers(-3000, 3001, w)) + 30000, 0, 65535)
        else:
            row = np.where((np.arange(w) > w // 3) & (np.arange(w) < 2 * w // 3), 62000, 1000)
        z = row.astype(np.int64)
        rep = ac.representatives(z, P, m)
        assert np.array_equal(rep, _brute_force_rep(z, P, m)), (trial, w, P, m)
        members = max(members, int(np.bincount(rep).max()))
    assert members >= 3


def test_rep_is_never_left_of_its_column():
    for name in ac.DEPTHS:
        for shape in ((3, 5, 257), (3, 1, 130)):
            for P, m in ((16, 128), (96, 85)):
                for invert in (False, True):
                    rep = ac.want_rep(name, shape, P, m, invert)
                    assert (rep >= np.arange(shape[2])).all() and (rep < shape[2]).all()
                    assert np.array_equal(np.take_along_axis(rep, rep, axis=2), rep)                # a representative represents itself


def test_hidden_columns_sit_beside_a_step():
    """A near block on a far ground hides ground columns next to its edges, none of its own and none far away."""
    z = np.where((np.arange(400) >= 150) & (np.arange(400) < 250), 60000, 3000).astype(np.int64)
    hid = ac.hidden(z, 96, 85)
    assert hid[149] and hid[250] and not hid[150:250].any() and not hid[:120].any() and not hid[280:].any()
    assert hid.sum() == 2 * int(hid[:150].sum()) > 2
    assert not ac.hidden(np.full(400, 65535, np.int64), 96, 85).any() and not ac.hidden(np.zeros(400, np.int64), 512, 128).any()


def test_census_of_the_gpu_cases():
    """From the model alone: the rectangle case of tests/test_gpu_autostereogram.py has hidden columns and a component of >= 3 members,
    the noise case has hidden columns, the chain has its 137 members, and width 20 links nothing at period 32."""
    shape, params, _ = ac.LARGE_CASES[0]
    P, m = params[0]
    rect, noise = (ac.census(ac.depth_input(name, shape)[0], P, m) for name in ("rect", "noise"))
    print(shape, (P, m), "rect", rect, "noise", noise)
    assert rect['hidden'] >= 1 and rect['largest'] >= 3 and noise['hidden'] >= 1 and noise['links'] >= 1
    shape, P, m = ac.CHAIN
    chain = ac.census(ac.depth_input("full", shape)[0], P, m)
    print(shape, (P, m), "chain", chain)
    assert chain['largest'] == 137 and chain['hidden'] == 0
    for name in ac.DEPTHS:
        assert ac.census(ac.depth_input(name, (3, 1, 20))[0], 32, 85)['links'] == 0
    # P = 512 links only on the wide case
    shape, params, _ = ac.LARGE_CASES[1]
    assert params[0][0] == 512 and ac.census(ac.depth_input("rect", shape)[0], *params[0])['links'] > 0
    assert all(ac.census(ac.depth_input("zeros", s)[0], 512, 128)['links'] == 0 for s in ac.SMALL_SHAPES)


def test_an_image_does_not_depend_on_its_batch():
    depth = ac.depth_input("noise", (3, 5, 130))
    whole = ac.model(depth, 16, 128, 0, 9)
    assert all(np.array_equal(ac.model(depth[i], 16, 128, 0, 9), whole[i]) for i in range(3))
