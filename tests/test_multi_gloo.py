"""The N>1 path on CPU: world_size-2 (and 3) gloo groups.  Each rank renders ITS row strip
(the oracle stands in for the GPU renderer -- tests may use it), the strips are gathered by the
same `distributed.gather_strips` bench.py uses, and rank 0 compares with a single-rank frame."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import CAM, ROOT
from render_common import free_port as _free_port

W, H, DEPTH = 96, 60, 4      # 60 rows: strips of unequal height (8-row tiles: 32/28 and 24/24/12)


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from example_gui_opencl_raytracer_amd import distributed as D, scene, textures
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    from oracle.oracle_py import Oracle
    r, w, _ = D.init_process_group("gloo")
    assert (r, w) == (rank, world)
    o = Oracle()
    sc, tex, sky = scene.render_map_scene(), textures.texture_layers(), textures.skybox_cross(512)
    cam = o.camera(CAM["origin"], CAM["look"], 90.0, 1.0, W, H)
    r0, rows = strip_rows(H, world, rank)
    strip, _, _ = o.render(cam, sc, tex, sky, DEPTH, id_begin=r0 * W, id_end=(r0 + rows) * W, threads=1)
    full = D.gather_strips(torch.from_numpy(strip.view(np.int32)), W, H, rank, world)
    dist.barrier()
    if rank == 0:
        np.save(out_path, full.numpy().view(np.uint32))
    else:
        assert full is None
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_strips_gather_to_the_single_rank_frame(oracle, demo_scene, tex, sky, tmp_path, world):
    out = str(tmp_path / f"full_{world}.npy")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    got = np.load(out)
    cam = oracle.camera(CAM["origin"], CAM["look"], 90.0, 1.0, W, H)
    want, _, _ = oracle.render(cam, demo_scene, tex, sky, DEPTH)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_single_rank_gather_is_identity():
    from example_gui_opencl_raytracer_amd import distributed as D
    t = torch.arange(12, dtype=torch.int32)
    assert D.gather_strips(t, 4, 3, 0, 1) is t


def _band_worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from example_gui_opencl_raytracer_amd import distributed as D, scene, textures
    from oracle.oracle_py import Oracle
    D.init_process_group("gloo")
    o = Oracle()
    sc, tex, sky = scene.render_map_scene(), textures.texture_layers(), textures.skybox_cross(512)
    w, h = 96, 16 * world * 2                       # height % (8 * world) == 0
    cam = o.camera(CAM["origin"], CAM["look"], 90.0, 1.0, w, h)
    # rank r owns bands r, r + world, ...: band b = rows [8b, 8b + 8) with GLOBAL ids
    share = np.concatenate([o.render(cam, sc, tex, sky, DEPTH, id_begin=8 * b * w, id_end=8 * (b + 1) * w, threads=1)[0]
                            for b in range(rank, h // 8, world)])
    gat = D.BandGatherer(w, h, rank, world, torch.device("cpu"))
    for frame in range(3):                          # both slots, and reuse of slot 0
        gat.before_render(frame & 1)
        gat.submit(frame & 1, torch.from_numpy(share.view(np.int32)))
    gat.drain()
    dist.barrier()
    if rank == 0:
        assert torch.equal(gat.assemble(0), gat.assemble(1))
        np.save(out_path, gat.assemble(0).numpy().view(np.uint32))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_interleaved_bands_gather_to_the_single_rank_frame(oracle, demo_scene, tex, sky, tmp_path, world):
    """bench.py's multi-GPU path: interleaved 8-row bands + BandGatherer (double-buffered async gather)."""
    out = str(tmp_path / f"bands_{world}.npy")
    mp.spawn(_band_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    got = np.load(out)
    w, h = 96, 16 * world * 2
    cam = oracle.camera(CAM["origin"], CAM["look"], 90.0, 1.0, w, h)
    want, _, _ = oracle.render(cam, demo_scene, tex, sky, DEPTH)
    assert np.array_equal(got, want)


def _strip_gatherer_worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from example_gui_opencl_raytracer_amd import distributed as D, scene, textures
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    from oracle.oracle_py import Oracle
    D.init_process_group("gloo")
    o = Oracle()
    sc, tex, sky = scene.render_map_scene(), textures.texture_layers(), textures.skybox_cross(512)
    cam = o.camera(CAM["origin"], CAM["look"], 90.0, 1.0, W, H)
    r0, rows = strip_rows(H, world, rank)
    strip, _, _ = o.render(cam, sc, tex, sky, DEPTH, id_begin=r0 * W, id_end=(r0 + rows) * W, threads=1)
    gat = D.FrameGatherer(W, H, rank, world, torch.device("cpu"), layout="strips")
    assert gat.transport == "gather" and gat.rows == [strip_rows(H, world, r)[1] for r in range(world)]
    for frame in range(3):                          # both slots, and reuse of slot 0
        gat.before_render(frame & 1)
        gat.submit(frame & 1, torch.from_numpy(strip.view(np.int32)))
    gat.drain()
    dist.barrier()
    if rank == 0:
        assert torch.equal(gat.assemble(0), gat.assemble(1))
        np.save(out_path, gat.assemble(0).numpy().view(np.uint32))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_unequal_row_strips_through_the_frame_gatherer(oracle, demo_scene, tex, sky, tmp_path, world):
    """bench.py --scaling strong / --config c5: contiguous strips of unequal height (60 rows: 32/28 and 24/24/12),
    padded to the tallest for the transfer, assembled on rank 0."""
    out = str(tmp_path / f"strips_{world}.npy")
    mp.spawn(_strip_gatherer_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    cam = oracle.camera(CAM["origin"], CAM["look"], 90.0, 1.0, W, H)
    want, _, _ = oracle.render(cam, demo_scene, tex, sky, DEPTH)
    assert np.array_equal(np.load(out), want)


def _consumer_worker(rank, world, port, out_path):
    """Every frame is DIFFERENT and rank 0 consumes every frame (complete -> assemble -> compare) while the ranks keep submitting:
    the slot-reuse rule of FrameGatherer (release / the consumer's event before a slot is overwritten)."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from example_gui_opencl_raytracer_amd import distributed as D
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    D.init_process_group("gloo")
    gat = D.FrameGatherer(W, H, rank, world, torch.device("cpu"), layout="strips", transport="rccl-gather")
    assert gat.transport == "gather"
    r0, rows = strip_rows(H, world, rank)

    def frame_pixels(k):         # 0x00RRGGBB words that depend on the frame and on the GLOBAL pixel index
        idx = np.arange(W * H, dtype=np.int64)
        return ((idx * 2654435761 + k * 40503) & 0xFFFFFF).astype(np.int32)

    bad = 0
    for k in range(7):
        s = k & 1
        gat.before_render(s)
        gat.submit(s, torch.from_numpy(frame_pixels(k)[r0 * W:(r0 + rows) * W].copy()))
        if rank == 0:
            gat.complete(s)
            bad += int(not np.array_equal(gat.assemble(s).numpy(), frame_pixels(k)))
    gat.drain()
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([bad]))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_per_frame_consumer_sees_every_frame_whole(tmp_path, world):
    out = str(tmp_path / f"consumer_{world}.npy")
    mp.spawn(_consumer_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert int(np.load(out)[0]) == 0
