"""CPU, 2 to 4 ranks over gloo: video mode's temporal depth filter when the frames are sharded in contiguous blocks
(src/video_mode.py: stabilize_depth_sharded).  Each rank filters its block from multigpu.my_shard; the blocks are gathered (uint16 as
its uint8 view: gloo has no 16-bit integer collectives) and compared with the NumPy model on the WHOLE clip (tests/video_stabilize_cases.py), bit for bit.
  7 frames, radius 4, worlds 2 (4+3), 3 (3+3+1) and 4 (2+2+2+1): a halo of four frames spans several neighbours, and runs out of
    ranks on both sides;
  9 frames at 4 ranks, 3+3+3+0: an empty shard that takes part in every collective;
  cuts on a shard boundary and inside a shard, single-frame scenes beside a halo."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import conftest
import video_stabilize_cases as sc

H, W = 6, 10


def _clip(n_frames, c=3):
    """Static content with small colour noise (weights near 1: every halo frame changes the result) ..."""
    frames, depth = sc.static_clip(n_frames, H, W, c, seed=20 + n_frames)
    noise_f, _ = sc.noise_clip(n_frames, H, W, c, seed=30 + n_frames)
    frames[:, :, W // 2:] = noise_f[:, :, W // 2:]              # ... on the left half, white noise (every k) on the right
    return frames, depth


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_frames, params, cuts, out_dir):
    for p in (conftest.ROOT, conftest.PKG, os.path.join(conftest.ROOT, "tests"), os.path.join(conftest.ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src import video_mode, multigpu
    frames, depth = _clip(n_frames)
    s, e = multigpu.my_shard(n_frames, rank, world)
    np.save(os.path.join(out_dir, "count%d.npy" % rank), np.asarray([e - s]))
    out = video_mode.stabilize_depth_sharded(torch.from_numpy(frames[s:e]), torch.from_numpy(depth[s:e]), params, cuts=cuts)
    assert out.dtype == torch.uint16 and tuple(out.shape) == (e - s, H, W)
    full = multigpu.gather_units(out.contiguous().view(torch.uint8).reshape(e - s, H, W * 2), n_frames)       # gloo moves no 16-bit integers
    if rank == 0:
        np.save(os.path.join(out_dir, "out.npy"), full.numpy().view(np.uint16).reshape(n_frames, H, W))
    # an RGBA clip at radius 1
    frames4, depth4 = _clip(n_frames, c=4)
    out4 = video_mode.stabilize_depth_sharded(torch.from_numpy(frames4[s:e]), torch.from_numpy(depth4[s:e]), (1,) + tuple(params[1:]), cuts=cuts)
    full4 = multigpu.gather_units(out4.contiguous().view(torch.uint8).reshape(e - s, H, W * 2), n_frames)
    if rank == 0:
        np.save(os.path.join(out_dir, "out4.npy"), full4.numpy().view(np.uint16).reshape(n_frames, H, W))
    dist.barrier()
    dist.destroy_process_group()


CASES = [(2, 7, 4, None, [4, 3]), (3, 7, 4, None, [3, 3, 1]), (4, 7, 4, None, [2, 2, 2, 1]),
         (4, 9, 4, None, [3, 3, 3, 0]), (4, 9, 2, [3], [3, 3, 3, 0]),                      # an empty shard; a cut on a shard boundary
         (4, 7, 4, [2, 3], [2, 2, 2, 1]),                                                 # boundary, and a one-frame scene inside a shard
         (3, 7, 3, [1, 4, 6], [3, 3, 1]),                                                 # inside shards and on a boundary; the last frame a scene
         (2, 7, 2, [4], [4, 3])]


@pytest.mark.parametrize("world,n_frames,radius,cuts,split", CASES, ids=["w%d-n%d-r%d-%s" % (c[0], c[1], c[2], c[3]) for c in CASES])
def test_sharded_filter_equals_the_model_on_the_whole_clip(tmp_path, world, n_frames, radius, cuts, split):
    params = (radius, 12.0, 2.0)
    mp.spawn(_worker, args=(world, _free_port(), n_frames, params, cuts, str(tmp_path)), nprocs=world, join=True)
    assert [int(np.load(str(tmp_path / ("count%d.npy" % r)))[0]) for r in range(world)] == split
    frames, depth = _clip(n_frames)
    want = sc.model(depth, frames, params, cuts=cuts)
    got = np.load(str(tmp_path / "out.npy"))
    assert got.dtype == np.uint16 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert (want != depth).mean() > 0.25                                              # the filter did something
    frames4, depth4 = _clip(n_frames, c=4)
    assert np.array_equal(np.load(str(tmp_path / "out4.npy")), sc.model(depth4, frames4, (1,) + params[1:], cuts=cuts))
