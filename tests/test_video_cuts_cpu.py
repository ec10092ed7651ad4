"""Video mode with scene cuts (src/video_mode.py: process_predicitons(cuts=), cut_scores, detect_cuts), no GPU needed.
The normalisation is pinned by the REFERENCE's own function run scene by scene (tests/golden/make_golden_video_cuts.py ->
video_cuts_cases.npz), bit for bit, dtype included; the cut rule by its NumPy model (tests/video_cuts_cases.py), which shares no
code with src/.  Sharded over gloo: tests/test_video_cuts_gloo.py; the kernels: tests/test_gpu_video_cuts.py."""
import os

import numpy as np
import pytest
import torch

import conftest
import make_golden_video_cuts as mgc
import video_cuts_cases as vc

GOLD = os.path.join(conftest.ROOT, "tests", "golden")


@pytest.mark.parametrize("mode", ["none", "experimental"])
@pytest.mark.parametrize("case", sorted(mgc.CUTS))
def test_every_scene_is_the_reference_on_that_scene(case, mode):
    from src import video_mode
    want = np.load(os.path.join(GOLD, "video_cuts_cases.npz"))[f"{case}/{mode}"]
    preds = mgc.predictions(case)
    got = video_mode.process_predicitons([x for x in preds], mode, cuts=mgc.CUTS[case])
    assert isinstance(got, list) and len(got) == preds.shape[0]
    got = np.stack(got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert np.isfinite(got).all()
    whole = np.load(os.path.join(GOLD, "video_cases.npz"))[f"{case}/{mode}"]
    assert not np.array_equal(got, whole), "the cuts changed nothing: the case tests nothing"


@pytest.mark.parametrize("mode", ["none", "experimental", "something else"])
def test_no_cuts_is_the_cutless_call(mode):
    from src import video_mode
    for case in sorted(mgc.CUTS):
        preds = [x for x in mgc.predictions(case)]
        plain = video_mode.process_predicitons(preds, mode)
        for cuts in (None, [], ()):
            got = video_mode.process_predicitons(preds, mode, cuts=cuts)
            assert len(got) == len(plain)
            for a, b in zip(got, plain):
                assert a.dtype == b.dtype and np.array_equal(a, b), (case, cuts)
        if mode != "something else":
            assert np.array_equal(np.stack(plain), np.load(os.path.join(GOLD, "video_cases.npz"))[f"{case}/{mode}"])


@pytest.mark.parametrize("cuts", [[0], [9], [12], [3, 3], [4, 2], [-1], [2.0], [1.5], ["3"], [True], [1, 4, 9, 9]])
def test_bad_cuts_raise(cuts):
    from src import video_mode
    preds = [x for x in mgc.predictions("n9")]                   # F = 9: legal cuts are 1..8, strictly increasing
    for mode in ("none", "experimental"):
        with pytest.raises(ValueError):
            video_mode.process_predicitons(preds, mode, cuts=cuts)
        with pytest.raises(ValueError):
            video_mode.process_predictions_sharded(torch.from_numpy(np.stack(preds)), mode, cuts=cuts)


def test_flat_scene_gives_what_the_reference_gives_for_a_flat_clip():
    """A scene whose every value is the same: (x - mn) / (mx - mn) = 0 / 0.  The expected side is the NumPy restatement of the
    reference in oracle/ (which the goldens pin) on each scene alone; the other scene must not notice."""
    from oracle import oracle as orc
    from src import video_mode
    preds = mgc.predictions("n9").copy()
    preds[2:5] = np.float32(1.25)
    with np.errstate(all="ignore"):
        for mode in ("none", "experimental"):
            got = np.stack(video_mode.process_predicitons([x for x in preds], mode, cuts=[2, 5]))
            want = np.stack([y for a, b in ((0, 2), (2, 5), (5, 9)) for y in orc.process_predicitons([x for x in preds[a:b]], mode)])
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), mode
            assert np.isnan(got[2:5]).all() and np.isfinite(got[:2]).all() and np.isfinite(got[5:]).all()


# ---- the cut rule -----------------------------------------------------------------------------------------------------------------
def _both(frames, **kw):
    """detect_cuts / cut_scores on numpy and torch input against the model."""
    from src import video_mode
    bins = kw.get("bins", 64)
    want_s = vc.cut_scores_model(frames, bins)
    want_c = vc.detect_cuts_model(frames, **kw)
    for f in (frames, torch.from_numpy(frames)):
        s = video_mode.cut_scores(f, bins=bins)
        assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == (frames.shape[0],)
        assert np.array_equal(s, want_s), (s, want_s)
        assert s[0] == 0.0 and (s >= 0).all() and (s <= 1).all()
        c = video_mode.detect_cuts(f, **kw)
        assert isinstance(c, list) and all(type(t) is int for t in c) and c == want_c, (c, want_c)
    return want_c, want_s


def test_two_scenes_one_cut():
    frames = vc.clip_of(21, [5, 4], [60, 190])
    cuts, score = _both(frames)
    assert cuts == [5] and score[5] > 0.9 and score[1:5].max() < 0.4 and score[6:].max() < 0.4


@pytest.mark.parametrize("c", [0, 1, 3, 4])
def test_channel_layouts(c):
    """c = 0: [F,H,W]; 1: the sample is Y; 3 / 4: the integer luma of R, G, B (a fourth channel, here noise, is ignored)."""
    frames = vc.clip_of(30 + c, [3, 1, 4], [50, 220, 120], h=9, w=13, c=c)
    cuts, _ = _both(frames)
    assert cuts == [3, 4]
    if c == 4:
        from src import video_mode
        other = frames.copy()
        other[..., 3] = 255 - other[..., 3]
        assert np.array_equal(video_mode.cut_scores(other), video_mode.cut_scores(frames))


def test_luma_is_the_integer_formula_white_is_255():
    from src import video_mode
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (2, 6, 7, 3), dtype=np.uint8)
    frames[1] = 255
    h = video_mode._luma_hist(torch.from_numpy(frames)).numpy()
    assert h.dtype == np.int64 and np.array_equal(h, vc.hist_model(frames))
    assert h[1, 255] == 42 and h[1].sum() == 42


def test_min_len_suppresses_a_one_frame_flash():
    frames = vc.clip_of(22, [4, 1, 5], [70, 240, 70])            # frame 4 is a flash inside one scene
    assert _both(frames)[0] == [4, 5]
    assert _both(frames, min_len=2)[0] == [4]                     # 5 - 4 < 2: the way back out of the flash is no cut
    assert _both(frames, min_len=5)[0] == [5]                     # 4 - 0 < 5, then 5 - 0 >= 5 and 10 - 5 >= 5
    assert _both(frames, min_len=6)[0] == []


def test_end_of_clip_rule():
    frames = vc.clip_of(23, [6, 2], [40, 200])                    # the second scene has two frames
    assert _both(frames, min_len=2)[0] == [6]
    assert _both(frames, min_len=3)[0] == []                      # F - t = 2 < 3
    assert _both(frames, threshold=1.0)[0] == []                  # a score never exceeds 1


@pytest.mark.parametrize("bins", [2, 4, 8, 16, 32, 64, 128, 256])
def test_every_legal_bins_value(bins):
    frames = vc.clip_of(24, [3, 3, 2], [30, 100, 101], spread=20.0)
    _both(frames, bins=bins, threshold=0.25)


@pytest.mark.parametrize("bins", [0, 1, 3, 48, 512, 64.5])
def test_illegal_bins_raise(bins):
    from src import video_mode
    with pytest.raises(ValueError):
        video_mode.cut_scores(vc.clip_of(1, [2], [10]), bins=bins)


def test_single_frame_and_bad_frames():
    from src import video_mode
    one = vc.clip_of(2, [1], [10])
    assert video_mode.detect_cuts(one) == [] and np.array_equal(video_mode.cut_scores(one), np.zeros(1))
    with pytest.raises(ValueError):
        video_mode.cut_scores(np.zeros((2, 4, 4, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        video_mode.cut_scores(np.zeros((2, 4, 4, 3), dtype=np.float32))
