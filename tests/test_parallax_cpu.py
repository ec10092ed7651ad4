"""The parallax renderer without a GPU: what the definition (include/depthstereo.h, ds_parallax_u8) promises, shown on its NumPy model
(tests/parallax_cases.py); a census that keeps tests/test_gpu_parallax.py honest: every case it runs must contain the targets on which
a wrong depth test, a one-wide footprint, a missing bounds test, a wrong scan order or a missing fallback would show; and the
product's host half (the validator, the camera paths, the poses)."""
import numpy as np
import pytest

import parallax_cases as pc


def test_identity_pose_returns_the_image_for_any_depth():
    for shape, G, focus in pc.KERNEL_CASES:
        image, depths = pc.inputs(shape)
        for name in pc.DEPTHS:
            for invert in (False, True):
                out, mask = pc.model(image, depths[name], focus, [(0, 0, 0)], G, invert)
                assert np.array_equal(out[:, 0], image) and not mask.any(), (shape, name, invert)


def test_depth_at_the_focus_returns_the_image_for_any_pose():
    for shape, G, _ in pc.KERNEL_CASES:
        image, _ = pc.inputs(shape)
        for level in (0, 777, 65535):
            flat = np.full(shape, level, np.uint16)
            for invert in (False, True):
                out, mask = pc.model(image, flat, [level] * shape[0], pc.POSES, G, invert)
                assert all(np.array_equal(out[:, k], image) for k in range(len(pc.POSES))) and not mask.any(), (shape, level, invert)


def test_views_and_images_are_independent():
    shape, G, focus = pc.KERNEL_CASES[1]
    image, depths = pc.inputs(shape)
    depth = depths["noise"]
    out, mask = pc.model(image, depth, focus, pc.POSES, G)
    for k, pose in enumerate(pc.POSES):
        one = pc.model(image, depth, focus, [pose], G)
        assert np.array_equal(one[0][:, 0], out[:, k]) and np.array_equal(one[1][:, 0], mask[:, k])
    alone = pc.model(image[1], depth[1], focus[1], pc.POSES, G)
    assert np.array_equal(alone[0], out[1]) and np.array_equal(alone[1], mask[1])
    # poses beyond +-1024 are clamped
    assert np.array_equal(pc.model(image, depth, focus, [(5000, -1025, 1024)], G)[0], pc.model(image, depth, focus, [(1024, -1024, 1024)], G)[0])


def test_the_nearer_pixel_wins_and_holes_take_the_background():
    """A near rectangle on a far ground, focus on the ground: the rectangle moves, covers ground pixels (it is nearer) and leaves a hole
    that is filled with ground, never with the rectangle's colour."""
    h, w = 12, 30
    image = np.zeros((h, w, 3), np.uint8)
    depth = np.full((h, w), 1000, np.uint16)
    depth[3:9, 10:16] = 61000
    image[3:9, 10:16] = 255                                                # the rectangle is white, the ground black
    out, mask = pc.model(image, depth, 1000, [(160, 0, 0)], 8)             # e = 60000: sx = 146 sixteenths, 9 pixels to the right
    white = (out[0] == 255).all(-1)
    assert white[3:9, 19:25].all() and white.sum() >= 36 and not white[:, :19].any()
    assert (mask[0][3:9, 10:16] == 1).all() and (mask[0] == 2).sum() == 0  # the hole it left: filled, from the ground
    inv, _ = pc.model(image, (65535 - depth).astype(np.uint16), 64535, [(160, 0, 0)], 8, invert=True)
    assert np.array_equal(inv, out)


@pytest.mark.parametrize("case", range(len(pc.KERNEL_CASES)), ids=pc.KERNEL_IDS)
def test_census_of_the_gpu_cases(case):
    """From the model alone: over its depth kinds and poses, every case of tests/test_gpu_parallax.py contains a target offered more
    than one key, a two-wide footprint, a dropped splat, a hole won by each of the four directions and a mask == 2 pixel."""
    shape, G, focus = pc.KERNEL_CASES[case]
    image, depths = pc.inputs(shape)
    census = {}
    for name in pc.DEPTHS:
        pc.model(image, depths[name], focus, pc.POSES, G, census=census)
    print(pc.KERNEL_IDS[case], census)
    for what in ('collided', 'two_wide', 'dropped', 'fallback') + pc.DIRECTIONS:
        assert census[what] > 0, (what, census)


def test_validator_accepts_and_rejects():
    from src import _native
    P = _native.parallax_params
    assert P(('circle', 24, 12.0, 6.0, 0.04)) == ('circle', 24, 12.0, 6.0, 0.04, ('point', 0.5, 0.5), 32)
    assert P(['line', 1, -64, 64, -0.25, 65535, 64]) == ('line', 1, -64.0, 64.0, -0.25, 65535, 64)
    assert P(('circle', np.int64(256), np.float32(2.0), 0, 0.25, ['point', 0, 1], np.int32(1))) == ('circle', 256, 2.0, 0.0, 0.25, ('point', 0.0, 1.0), 1)
    assert [type(v) for v in P(('line', 3.0, 1, 2, 0, 5.0, 7.0))] == [str, int, float, float, float, int, int]
    explicit = P(([[1.0, -2.0, 0.1], [0, 0, 0]], None, 0, 0, 0))
    assert np.array_equal(explicit[0], np.array([[1.0, -2.0, 0.1], [0, 0, 0]])) and explicit[1:] == (2, 0.0, 0.0, 0.0, ('point', 0.5, 0.5), 32)
    assert P((np.zeros((3, 3)), 3, 0, 0, 0))[1] == 3
    nan, inf = float('nan'), float('inf')
    for bad in (('spiral', 24, 1, 1, 0), (None, 24, 1, 1, 0), (b'circle', 24, 1, 1, 0), ('circle', 0, 1, 1, 0), ('circle', 257, 1, 1, 0),
                ('circle', True, 1, 1, 0), ('circle', 2.5, 1, 1, 0), ('circle', '24', 1, 1, 0), ('circle', None, 1, 1, 0), ('circle', nan, 1, 1, 0),
                ('circle', 24, 64.5, 1, 0), ('circle', 24, 1, -64.5, 0), ('circle', 24, nan, 1, 0), ('circle', 24, 1, inf, 0),
                ('circle', 24, '1', 1, 0), ('circle', 24, True, 1, 0), ('circle', 24, 1, None, 0),
                ('circle', 24, 1, 1, 0.26), ('circle', 24, 1, 1, -0.26), ('circle', 24, 1, 1, nan), ('circle', 24, 1, 1, '0'), ('circle', 24, 1, 1, False),
                ('circle', 24, 1, 1, 0, -1), ('circle', 24, 1, 1, 0, 65536), ('circle', 24, 1, 1, 0, 0.5), ('circle', 24, 1, 1, 0, True),
                ('circle', 24, 1, 1, 0, None), ('circle', 24, 1, 1, 0, 'near'), ('circle', 24, 1, 1, 0, ('point', 1.5, 0.5)),
                ('circle', 24, 1, 1, 0, ('point', nan, 0.5)), ('circle', 24, 1, 1, 0, 0, 0), ('circle', 24, 1, 1, 0, 0, 65), ('circle', 24, 1, 1, 0, 0, True),
                ('circle', 24, 1, 1, 0, 0, 2.5), ('circle', 24, 1, 1, 0, 0, '8'), ('circle', 24, 1, 1, 0, 0, None),
                (np.zeros((3, 3)), 4, 0, 0, 0), (np.zeros((3, 2)), None, 0, 0, 0), (np.zeros(3), None, 0, 0, 0), (np.zeros((0, 3)), None, 0, 0, 0),
                (np.zeros((257, 3)), None, 0, 0, 0), ([[65.0, 0, 0]], None, 0, 0, 0), ([[0, 0, 0.3]], None, 0, 0, 0), ([[nan, 0, 0]], None, 0, 0, 0),
                ([['a', 0, 0]], None, 0, 0, 0), ([[True, False, False]], None, 0, 0, 0),
                ('circle', 24, 1, 1), ('circle',), ('circle', 24, 1, 1, 0, 0, 8, 9), "circle", b"circle", 24, None,
                {0: 'circle', 1: 24, 2: 1, 3: 1, 4: 0}):
        with pytest.raises(ValueError):
            P(bad)


def test_paths_and_poses():
    from src import _native
    import src.parallax_generation as pg
    F = 24
    circle = pg.camera_path('circle', F)
    a = 2 * np.pi * np.arange(F, dtype=np.float64) / F
    assert circle.dtype == np.float64 and circle.shape == (F, 3)
    assert np.array_equal(circle, np.stack([12.0 * np.cos(a), 6.0 * np.sin(a), 0.04 * np.cos(a)], axis=1))
    assert np.array_equal(circle[0], [12.0, 0.0, 0.04]) and abs(circle[F // 2][0] + 12.0) < 1e-12
    swing = pg.camera_path('circle', 8, shift=(5.0, 0.0), zoom=0.0)
    assert not swing[:, 1:].any() and swing[0, 0] == 5.0
    line = pg.camera_path('line', 5, shift=(8.0, -4.0), zoom=0.1)
    assert np.array_equal(line, np.outer([-1.0, -0.5, 0.0, 0.5, 1.0], [8.0, -4.0, 0.1]))
    assert np.array_equal(pg.camera_path('line', 1), [[0.0, 0.0, 0.0]])                      # F = 1: the origin
    assert np.array_equal(pg.camera_path('circle', 1, (3.0, 2.0), 0.01), [[3.0, 0.0, 0.01]])  # a_0 = 0
    assert np.array_equal(pg.camera_path('line', 2, (64, 64), 0.25), [[-64, -64, -0.25], [64, 64, 0.25]])
    # poses: rint(16 x), rint(16 y), rint(4096 z), half to even, int32, within +-1024
    poses = _native.parallax_poses('line', 2, 64, -64, 0.25)
    assert poses.dtype == np.int32 and np.array_equal(poses, [[-1024, 1024, -1024], [1024, -1024, 1024]])
    assert np.array_equal(_native.parallax_poses([[0.03125, 0.09375, 0.0], [-0.03125, 1.0, 1.5 / 4096]], None, 0, 0, 0), [[0, 2, 0], [0, 16, 2]])
    assert np.array_equal(_native.parallax_poses('circle', F, 12.0, 6.0, 0.04), np.rint(circle * [16.0, 16.0, 4096.0]).astype(np.int32))
    assert np.abs(_native.parallax_poses('circle', 256, 64, 64, 0.25)).max() == 1024
    assert np.array_equal(_native.parallax_poses('circle', 7, 0, 0, 0), np.zeros((7, 3), np.int32))
    for bad in (dict(kind='spiral', frames=4), dict(kind='circle', frames=0), dict(kind='circle', frames=257), dict(kind='circle', frames=True),
                dict(kind='circle', frames='4'), dict(kind='circle', frames=4, shift=(65.0, 0)), dict(kind='circle', frames=4, shift=(0, float('nan'))),
                dict(kind='circle', frames=4, shift=5.0), dict(kind='circle', frames=4, shift='ab'), dict(kind='circle', frames=4, shift=(1, 2, 3)),
                dict(kind='circle', frames=4, shift=(True, 0)), dict(kind='circle', frames=4, zoom=0.3), dict(kind='circle', frames=4, zoom='0'),
                dict(kind='circle', frames=4, zoom=float('nan')), dict(kind=np.zeros((2, 3)), frames=2)):
        with pytest.raises(_native.DepthStereoError):
            pg.camera_path(**bad)
    for bad in (('circle', 0, 1, 1, 0), ('circle', 4, 65, 1, 0), ('circle', 4, 1, 1, 1), ('ring', 4, 1, 1, 0), ('circle', 4, '1', 1, 0)):
        with pytest.raises(ValueError):
            _native.parallax_poses(*bad)


def test_save_animation_checks_its_arguments(tmp_path):
    from PIL import Image
    from src import _native
    import src.parallax_generation as pg
    frames = [Image.fromarray(np.full((4, 6, 3), 40 * k, np.uint8)) for k in range(3)]
    for ext in ('gif', 'webp', 'png'):
        name = pg.save_animation(frames, str(tmp_path / ('clip.' + ext)), fps=10)
        with Image.open(name) as im:
            assert getattr(im, 'n_frames', 1) == 3 and im.size == (6, 4), ext
    for bad in (dict(frames=frames, filename=str(tmp_path / 'clip.mp4')), dict(frames=[], filename=str(tmp_path / 'a.gif')),
                dict(frames=[np.zeros((4, 6, 3), np.uint8)], filename=str(tmp_path / 'a.gif')), dict(frames=frames, filename=str(tmp_path / 'a.gif'), fps=0),
                dict(frames=frames, filename=str(tmp_path / 'a.gif'), fps=True)):
        with pytest.raises(_native.DepthStereoError):
            pg.save_animation(**bad)
