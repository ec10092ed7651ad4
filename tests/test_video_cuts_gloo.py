"""CPU, 2 to 4 ranks over gloo: video mode with scene cuts when the frames are sharded in contiguous blocks
(src/video_mode.py: process_predictions_sharded(cuts=), cut_scores / detect_cuts with a group).  The expected side is the
reference's own function run scene by scene (tests/golden/video_cuts_cases.npz) and the unsharded cut list.
  (2, n12) 6+6 and (3, n12) 4+4+4 with cuts [1, 4, 9]: a cut exactly on a shard boundary (4), scenes inside one rank and across two;
  (3, n5_wide) 2+2+1, every frame a scene: cuts on both shard boundaries, single-frame scenes beside a halo;
  (4, n9) 3+3+3+0 with cut [2]: a scene that spans three ranks, and an empty shard that takes part in every collective.
Every rank also detects the cuts of one synthetic clip from its own block of frames: all ranks must hold the same scores and list."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import conftest
import make_golden_video_cuts as mgc
import video_cuts_cases as vc

DETECT_CLIP = dict(seed=41, lengths=[3, 1, 3], means=[60, 200, 110], h=10, w=12)      # F = 7: 2 ranks 4+3, 3 ranks 3+3+1, 4 ranks 2+2+2+1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, mode, out_dir):
    for p in (conftest.ROOT, conftest.PKG, os.path.join(conftest.ROOT, "tests"), os.path.join(conftest.ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src import video_mode, multigpu
    preds = mgc.predictions(case)
    n_frames = preds.shape[0]
    s, e = multigpu.my_shard(n_frames, rank, world)
    out = video_mode.process_predictions_sharded(torch.from_numpy(preds[s:e]), mode, cuts=mgc.CUTS[case])
    assert out.shape[0] == e - s
    full = multigpu.gather_units(out.contiguous(), n_frames)
    if rank == 0:
        np.save(os.path.join(out_dir, "norm.npy"), full.numpy())
    frames = vc.clip_of(**DETECT_CLIP)
    score = video_mode.cut_scores(torch.from_numpy(frames))                  # the default group: sharded
    cuts = video_mode.detect_cuts(frames)
    np.save(os.path.join(out_dir, "score%d.npy" % rank), score)
    np.save(os.path.join(out_dir, "cuts%d.npy" % rank), np.asarray(cuts, dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["none", "experimental"])
@pytest.mark.parametrize("world,case", [(2, "n12"), (3, "n12"), (3, "n5_wide"), (4, "n9")])
def test_sharded_scenes_equal_reference_and_every_rank_finds_the_same_cuts(tmp_path, mode, world, case):
    want = np.load(os.path.join(conftest.ROOT, "tests", "golden", "video_cuts_cases.npz"))[f"{case}/{mode}"]
    mp.spawn(_worker, args=(world, _free_port(), case, mode, str(tmp_path)), nprocs=world, join=True)
    got = np.load(str(tmp_path / "norm.npy"))
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    frames = vc.clip_of(**DETECT_CLIP)
    want_score, want_cuts = vc.cut_scores_model(frames), vc.detect_cuts_model(frames)
    assert want_cuts == [3, 4]
    for r in range(world):
        assert np.array_equal(np.load(str(tmp_path / ("score%d.npy" % r))), want_score), r
        assert np.load(str(tmp_path / ("cuts%d.npy" % r))).tolist() == want_cuts, r
