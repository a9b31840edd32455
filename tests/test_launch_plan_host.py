"""The decision half of a trace launch (csrc/launch_plan.c) on the CPU: the flag word of every launch the GPU tests assert, the depth and
high-occupancy flavours at their edges, grids, the virtual frame, the per-lane tables, the tail's pool arithmetic, every refusal with its
text, the choice of the tile order, and that every flag word the planner can return has a compiled kernel (whitted_launch.inc)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import flags_common as F
import plan_common as pc
from conftest import ROOT
from plan_common import LAUNCH, NONE, PASS_BASE, PASS_PLAIN, PASS_REFINE, REFUSED, plan, plan_in, refusal

CSRC = os.path.join(ROOT, "example_gui_opencl_raytracer_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    return pc.seam()


def ceil_div(a, b):
    return -(-a // b)


def disp_of(ns):
    return np.arange(1, 3 * ns + 1, dtype=np.float32) / 8


# ------------------------------------------------------------------ the vocabulary
def test_flag_names_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "whitted_params.h")).read(), flags=re.S)
    enum = dict((k, eval(v)) for k, v in re.findall(r"\bWT_(F_[A-Z0-9_]+|SHAPE_[A-Z_]+)\s*=\s*([0-9 <]+)", text))
    mine = {k: v for k, v in vars(F).items() if k.startswith(("F_", "SHAPE_"))}
    assert len(enum) == 16 and enum == mine
    assert "#define WT_SHAPE_FLAGS(ns, np, nl) (WT_F_GEOM_LDS | WT_F_SHAPE | ((ns) << 9) | ((np) << 12) | ((nl) << 14))" in text
    # ... and nothing in csrc/ states a flag, a limit or a variant bit a second time
    for name in os.listdir(CSRC):
        body = open(os.path.join(CSRC, name)).read()
        if name != "whitted_params.h":
            assert not re.search(r"\bWT_F_[A-Z0-9_]+\s*=|define\s+WT_(SHAPE_FLAGS|BLOCK|VIS_MAX_SPHERES)\b", body), name
        if name != "launch_plan.h":
            assert not re.search(r"\bWT_V_[A-Z_]+\s*=", body), name


def test_struct_mirror_matches_the_library(L):
    sizes = (pc.u32 * 3)()
    L.wt_plan_sizes(sizes)
    assert list(sizes) == [C.sizeof(pc.PlanIn), C.sizeof(pc.PlanOut), pc.PlanOut.message.offset]


# ------------------------------------------------------------------ flag words
MODES = {"plain": (dict(), 0), "supersampled": (dict(supersample=2), F.F_SS),
         "refine": (dict(supersample=2, adaptive=16, pass_=PASS_REFINE), F.F_SS | F.F_LIST), "moving": (dict(supersample=2), F.F_SS | F.F_MOVE)}


@pytest.mark.parametrize("mode", MODES)
def test_the_flag_words_the_gpu_tests_assert(L, mode):
    kw, extra = MODES[mode]
    words = set()
    for ns, npl, depth in itertools.product((1, 2, 3, 4), (0, 1, 2), (1, 4)):
        o = plan(L, plan_in(scene=(ns, npl, 3), depth=depth, disp=disp_of(ns) if mode == "moving" else None, **kw))
        assert o.status == LAUNCH and o.flags == F.shape_flags(ns, npl, 3) | extra
        assert L.wt_fast_has_trace(o.flags)
        words.add(o.flags)
    assert len(words) == 12      # x 4 modes: the 48 cases of the shaped switch


@pytest.mark.parametrize("kw", [dict(scene=(5, 2, 3)), dict(scene=(4, 3, 3)), dict(scene=(4, 2, 2)), dict(scene=(4, 2, 4)), dict(lpt=False),
                                dict(variant=8192), dict(strict=1), dict(depth=5), dict(counting=1)], ids=str)
def test_no_shaped_kernel_outside_its_counts(L, kw):
    o = plan(L, plan_in(**kw))
    assert o.status == LAUNCH and not o.flags & F.F_SHAPE and o.flags & F.F_GEOM_LDS
    assert (L.wt_strict_has_trace if kw.get("strict") else L.wt_fast_has_trace)(o.flags)


def test_depth_flavours(L):
    want = {4: 0, 5: F.F_DEEP | F.F_D8, 8: F.F_DEEP | F.F_D8, 9: F.F_DEEP | F.F_D16, 16: F.F_DEEP | F.F_D16, 17: F.F_DEEP, 32: F.F_DEEP}
    mask = F.F_DEEP | F.F_D8 | F.F_D16
    for strict in (0, 1):
        for depth, word in want.items():
            assert plan(L, plan_in(depth=depth, strict=strict)).flags & mask == word
            for kw in (dict(counting=1), dict(variant=2048)):
                assert plan(L, plan_in(depth=depth, strict=strict, **kw)).flags & mask == word & F.F_DEEP


def test_high_occupancy_flavour_at_its_edge(L):
    over, under = dict(width=1800, height=1600, depth=5), dict(width=1792, height=1600, depth=5)
    o = plan(L, plan_in(**over))
    assert 8 * o.per_share == 45000 and o.flags & F.F_OCC and not o.tail_wanted
    u = plan(L, plan_in(**under))
    assert 8 * u.per_share == 44800 and not u.flags & F.F_OCC and u.tail_wanted
    assert not plan(L, plan_in(strict=1, **over)).flags & F.F_OCC
    assert not plan(L, plan_in(variant=64, **over)).flags & F.F_OCC
    assert plan(L, plan_in(occ_tiles_per_depth=8960, **under)).flags & F.F_OCC


# ------------------------------------------------------------------ grids
@pytest.mark.parametrize("w,h", [(64, 48), (61, 43), (8, 8), (800, 600), (7, 130)])
def test_grid_sizes(L, w, h):
    trows, tpr = ceil_div(h, 8), ceil_div(w, 8)
    tiled = 8 * ceil_div(trows, 8) * tpr
    o = plan(L, plan_in(w, h))
    assert (o.grid, o.trows, o.tpr, o.per_share, o.per_share_cap) == (tiled, trows, tpr, tiled // 8, tiled // 8) and o.P.tiled == 1
    lin = plan(L, plan_in(w, h, variant=2))
    assert lin.grid == ceil_div(w * h, 64) and lin.P.tiled == 0 and not lin.use_order
    # the split: 1024 more entries per share exactly when the tail is wanted, no grid, a quota, variants 4096 and 4 off, factor < 8
    deep = dict(depth=15)
    for kw, split in ((dict(), 1), (dict(variant=16), 0), (dict(scene=(300, 1, 3), grid_usable=1), 0), (dict(split_min_quota=0), 0),
                      (dict(variant=4096), 0), (dict(variant=4), 0), (dict(supersample=8), 0), (dict(supersample=4), 1), (dict(depth=4), 0),
                      (dict(tpt_max=0), 0), (dict(sched=0), 0)):
        o = plan(L, plan_in(w, h, **{**deep, **kw}))
        n = kw.get("supersample", 1)
        base = 8 * ceil_div(ceil_div(h * n, 8), 8) * ceil_div(w * n, 8)      # the virtual frame's
        assert o.status == LAUNCH and o.split == split and o.grid == base + 8 * 1024 * split and o.per_share_cap == base // 8 + 1024 * split, kw
        assert o.P.cost_sum == (1 if o.tail_wanted and o.use_order and not o.flags & F.F_GRID else 0)
    # the refine pass and the G-buffer pass run the grid of the trace launch over the same range
    ss = plan(L, plan_in(w, h, supersample=2, depth=4))
    rf = plan(L, plan_in(w, h, supersample=2, depth=4, adaptive=16, pass_=PASS_REFINE))
    assert rf.grid == ss.grid and not rf.use_order and not rf.split
    P = pc.Params(ns=4)
    L.wt_plan_fused_range(C.byref(pc.gen(w, h)), w * h, C.byref(P))
    assert L.wt_plan_grid(C.byref(P)) == tiled and (P.tiled, P.rows, P.row_offset, P.unit_dirs) == (1, h, 0, 1)


def test_a_tile_grid_beyond_4095_runs_in_the_default_order(L):
    o = plan(L, plan_in(8 * 4096, 8, depth=15))
    assert o.status == LAUNCH and not o.use_order and not o.split and o.grid == 8 * 4096


# ------------------------------------------------------------------ the virtual frame
@pytest.mark.parametrize("n", [2, 4, 8])
def test_virtual_frame(L, n):
    W, H = 64, 48
    o = plan(L, plan_in(W, H, supersample=n))
    P, g = o.P, pc.gen(W, H)
    assert (P.width, P.height, P.id_offset, P.n_items, P.ss_lg, P.rows, P.row_offset) == (n * W, n * H, 0, n * n * W * H, n.bit_length() - 1, n * H, 0)
    assert (P.w_factor, P.h_factor) == (np.float32(g.w_factor) / np.float32(n), np.float32(g.h_factor) / np.float32(n))
    assert o.out_pixels == W * H and o.out_offset == 0 and (o.sig.width, o.sig.n_items) == (n * W, n * n * W * H)
    # a strip: rows [16, 40) of the frame
    s = plan(L, plan_in(W, H, supersample=n, has_strip=1, strip_row0=16, strip_rows=24))
    P = s.P
    assert (P.width, P.height, P.id_offset, P.n_items, P.rows, P.row_offset) == (n * W, n * H, 16 * n * n * W, 24 * n * n * W, 24 * n, 16 * n)
    assert s.out_offset == 16 * W and s.out_pixels == 24 * W
    assert refusal(L, plan_in(32768 // n, 32768 * 4 // n, supersample=n)) == f"Supersampling: the {n} x {n} samples of this frame exceed 32-bit ids"
    assert plan(L, plan_in(32768 // n, 32768 * 4 // n - 1, supersample=n)).status == LAUNCH


# ------------------------------------------------------------------ the per-lane tables
@pytest.mark.parametrize("n", [2, 4, 8])
def test_lane_tables(L, n):
    ns = 4
    cams = np.arange(n * n * 12, dtype=np.float32).reshape(n * n, 12)
    times = np.linspace(0, 1, n * n, dtype=np.float32)
    disp = disp_of(ns)
    o = plan(L, plan_in(supersample=n, cams=cams, times=times, disp=disp))
    assert o.status == LAUNCH and (o.n_cams, o.n_times, o.motion_floats) == (n * n, n * n, pc.CAM_TABLE_FLOATS)
    table, motion = np.array(o.cam_table).reshape(64, 12), np.array(o.motion_table)[:o.motion_floats]
    for lane in range(64):
        k = ((lane >> 3) % n) * n + (lane & 7) % n
        assert L.wt_plan_lane_sample(lane, n) == k
        assert np.array_equal(table[lane], cams[k]) and motion[lane] == times[k]
    assert np.array_equal(motion[64:64 + 4 * ns].reshape(ns, 4), np.c_[disp.reshape(ns, 3), np.zeros(ns, np.float32)]) and not motion[64 + 4 * ns:].any()
    assert np.array_equal(np.array(o.cams_used)[:12 * n * n].reshape(n * n, 12), cams) and np.array_equal(np.array(o.times_used)[:n * n], times)
    # the shutter times of the factor when the caller gave none
    d = plan(L, plan_in(supersample=n, disp=disp))
    want = (C.c_float * (n * n))()
    L.clw_host_sample_times.argtypes = [pc.u32, C.c_void_p]
    assert L.clw_host_sample_times(n, want) == 1 and list(d.times_used)[:n * n] == list(want) and d.n_cams == 0


def test_the_staging_rule_counts_the_displacement_table(L):
    ns = 200      # geom_f4 = ns + 2 * 2 + 2 * 3 + 2
    for pad, lds in ((1024 - 212 - 200, True), (1024 - 212 - 200 + 1, False)):
        i = plan_in(scene=(ns, 2, 3), supersample=2, disp=disp_of(ns))
        i.geom_f4 += pad
        assert i.geom_f4 + ns == 1024 + (0 if lds else 1)
        o = plan(L, i)
        assert o.status == LAUNCH and bool(o.flags & F.F_GEOM_LDS) == lds and o.dyn_lds == (16 * (i.geom_f4 + ns) if lds else 0)
        assert o.flags & F.F_MOVE and o.motion_floats == 2 * pc.CAM_TABLE_FLOATS
        i.disp, i.n_disp = None, 0      # the static launch of the same scene stages it
        assert plan(L, i).dyn_lds == 16 * i.geom_f4


# ------------------------------------------------------------------ the tail's pool
def test_tail_pool_arithmetic(L):
    for kw, cap in ((dict(depth=15), 8512), (dict(depth=15, strict=1), 6208), (dict(depth=32), 8384)):
        o = plan(L, plan_in(**kw))
        assert o.tail_wanted and (o.tpt_slice, o.tpt_cap, o.tpt_nslots) == (1 << 18, cap, 8192)
        assert (o.P.tpt_slice_words, o.P.tpt_cap, o.P.tpt_slots, o.P.tpt_max, o.P.tpt_min) == (1 << 18, cap, 1024, 40, 4)
    for kw in (dict(tpt_pool_mb=8), dict(supersample=2, disp=disp_of(4)), dict(variant=16), dict(width=1800, height=1600)):
        o = plan(L, plan_in(**{**dict(depth=15, occ_tiles_per_depth=3000), **kw}))
        assert o.status == LAUNCH and not o.tail_wanted and not o.split and o.P.tpt_cap == 0, kw
    assert plan(L, plan_in(depth=15, tpt_max=64 + 9)).P.tpt_max == 64


# ------------------------------------------------------------------ refusals: the texts of the parent's die() calls
FUSED_NEED = " needs the fused raygen + trace launch (CLWRAP_FUSE=1, rays generated by this library and not rewritten)"
REFUSALS = [
    (dict(args_ok=0), "Couldn't run the kernel"),
    (dict(scene_ok=0), "Couldn't run the kernel"),
    (dict(aperture=0.5), "A lens needs samples: aperture 0.5 with supersampling factor 1 (clw_ext_set_supersample / CLWRAP_SUPERSAMPLE)"),
    (dict(cams=np.zeros((4, 12))), "Sample cameras: the table holds 4 cameras, but supersampling factor 1 takes none (set a factor of 2, 4 or 8)"),
    (dict(cams=np.zeros((16, 12)), supersample=2), "Sample cameras: the table holds 16 cameras, but supersampling factor 2 needs 4"),
    (dict(cams=np.zeros((4, 12)), supersample=4), "Sample cameras: the table holds 4 cameras, but supersampling factor 4 needs 16"),
    (dict(cams=np.zeros((4, 12)), supersample=8), "Sample cameras: the table holds 4 cameras, but supersampling factor 8 needs 64"),
    (dict(disp=disp_of(4)), "Moving spheres need samples: a displacement table with supersampling factor 1 (clw_ext_set_supersample / CLWRAP_SUPERSAMPLE)"),
    (dict(disp=disp_of(4), times=np.zeros(3), supersample=2), "Moving spheres: 3 sample times, but supersampling factor 2 needs 4"),
    (dict(disp=disp_of(3), supersample=2), "Moving spheres: the displacement table is for 3 spheres, the scene has 4"),
    (dict(disp=disp_of(300), scene=(300, 1, 3), supersample=2), "Moving spheres: scenes of more than 256 spheres (the uniform grid is built for one set of centres) are not supported"),
    (dict(disp=disp_of(200), scene=(200, 1, 3), grid_usable=1, supersample=2), "Moving spheres: scenes of more than 256 spheres (the uniform grid is built for one set of centres) are not supported"),
    (dict(supersample=2, gen=pc.gen(64, 48, band_stride=2)), "Supersampling does not support interleaved row bands"),
    (dict(supersample=2, variant=2), "Supersampling does not support linear work-item ids (variant 2)"),
    (dict(supersample=2, gen=pc.gen(64, 48, id_offset=10)), "Supersampling needs a launch range of whole rows"),
    (dict(supersample=2, adaptive=16, pass_=PASS_REFINE, variant=2), "Adaptive supersampling does not support linear work-item ids (variant 2)"),
    (dict(supersample=2, rays="own"), "Supersampling" + FUSED_NEED),
    (dict(supersample=2, rays="exposed"), "Supersampling" + FUSED_NEED),
    (dict(supersample=2, rays="caller", adaptive=16, pass_=PASS_REFINE), "Adaptive supersampling" + FUSED_NEED),
    (dict(rays="own", rays_size=64 * 64 * 48 - 1), "Couldn't run the kernel"),
    (dict(rays="caller", band_stride=2), "Row bands need a raygen launch"),
    (dict(width=8 * 4096, height=2, supersample=2, adaptive=16, pass_=PASS_REFINE), "Adaptive supersampling: 8192 x 1 blocks are more than a tile list can address (4095 each way)"),
    # the modes
    (dict(acc_frame=0, rays="own"), "Frame accumulation" + FUSED_NEED),
    (dict(acc_frame=0, supersample=2, cams=np.zeros((4, 12))), "Frame accumulation does not combine with a table of sample cameras (clw_ext_set_sample_cameras)"),
    (dict(acc_frame=0, supersample=2, aperture=0.5), "Frame accumulation does not combine with a lens (clw_ext_set_lens)"),
    (dict(acc_frame=0, supersample=2, disp=disp_of(4)), "Frame accumulation does not combine with moving spheres (clw_ext_set_sphere_motion)"),
    (dict(acc_frame=0, supersample=2, adaptive=16), "Frame accumulation does not combine with adaptive supersampling (clw_ext_set_adaptive)"),
    (dict(adaptive=16, pass_=PASS_BASE), "Adaptive supersampling needs samples: threshold 16 with supersampling factor 1 (clw_ext_set_supersample / CLWRAP_SUPERSAMPLE)"),
    (dict(adaptive=16, pass_=PASS_BASE, supersample=2, aperture=0.5), "Adaptive supersampling does not combine with a lens (clw_ext_set_lens): every pixel of such a frame needs its samples"),
    (dict(adaptive=16, pass_=PASS_BASE, supersample=2, cams=np.zeros((4, 12))),
     "Adaptive supersampling does not combine with a table of sample cameras (clw_ext_set_sample_cameras): every pixel of such a frame needs its samples"),
    (dict(adaptive=16, pass_=PASS_BASE, supersample=2, disp=disp_of(4)),
     "Adaptive supersampling does not combine with moving spheres (clw_ext_set_sphere_motion): every pixel of such a frame needs its samples"),
    # where two apply, the one printed today: the lens before the camera table, the tables before the bands, the bands before variant 2 ...
    (dict(aperture=0.5, cams=np.zeros((4, 12))), "A lens needs samples: aperture 0.5 with supersampling factor 1 (clw_ext_set_supersample / CLWRAP_SUPERSAMPLE)"),
    (dict(cams=np.zeros((4, 12)), disp=disp_of(4)), "Sample cameras: the table holds 4 cameras, but supersampling factor 1 takes none (set a factor of 2, 4 or 8)"),
    (dict(disp=disp_of(3), supersample=2, gen=pc.gen(64, 48, band_stride=2)), "Moving spheres: the displacement table is for 3 spheres, the scene has 4"),
    (dict(disp=disp_of(4), rays="own"), "Moving spheres need samples: a displacement table with supersampling factor 1 (clw_ext_set_supersample / CLWRAP_SUPERSAMPLE)"),
    (dict(supersample=2, variant=2, gen=pc.gen(64, 48, band_stride=2)), "Supersampling does not support interleaved row bands"),
    (dict(supersample=2, variant=2, gen=pc.gen(64, 48, id_offset=10)), "Supersampling does not support linear work-item ids (variant 2)"),
    (dict(supersample=2, rays="own", cams=np.zeros((16, 12))), "Sample cameras: the table holds 16 cameras, but supersampling factor 2 needs 4"),
    (dict(args_ok=0, scene_ok=0, aperture=0.5), "Couldn't run the kernel"),
    (dict(acc_frame=0, rays="own", aperture=0.5), "Frame accumulation" + FUSED_NEED),
    (dict(acc_frame=0, supersample=2, aperture=0.5, adaptive=16), "Frame accumulation does not combine with a lens (clw_ext_set_lens)"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals(L, kw, text):
    assert refusal(L, plan_in(**kw)) == text


def test_a_lens_that_cannot_be_derived(L):
    g = pc.gen(64, 48)
    g.corner[:] = (-1.0, 0.75, 0.0)      # corner + right * w / 2 - up * h / 2 = 0: the image plane passes through the origin
    assert refusal(L, plan_in(supersample=2, aperture=0.5, gen=g)) == "A lens cannot be derived from this camera (its image plane passes through its origin)"


def test_an_empty_range_is_no_launch_and_is_decided_before_the_scene(L):
    for kw in (dict(array_size=0), dict(total=0), dict(out_size=3)):
        o = plan(L, plan_in(scene_ok=0, aperture=0.5, **kw))
        assert o.status == NONE and not o.samples_decided
    assert plan(L, plan_in(args_ok=0, array_size=0)).status == REFUSED      # ... but after the ray handle
    assert plan(L, plan_in(gen=pc.gen(64, 48, n_items=0))).status == NONE
    # the range: rounded up to 256 work-items, guarded by `total` and by the framebuffer
    assert [L.wt_plan_range(a, t, o) for a, t, o in ((1, 3072, 1 << 20), (257, 3072, 1 << 20), (5000, 3072, 1 << 20), (5000, 3072, 4 * 100 + 3))] == [256, 512, 3072, 100]


# ------------------------------------------------------------------ which tile order a launch reads
def replay(L, changed, grid=False):
    """-> per frame (rd, wr, rebuild, wait_wr, wait_rd, newest after the launch)"""
    s, log = pc.OrderState(), []
    for ch in changed:
        wr = s.wr
        c = L.wt_order_choose(C.byref(s))
        rebuild = L.wt_order_rebuild(C.byref(s), ch, grid)
        L.wt_order_launched(C.byref(s), rebuild)
        assert s.wr == wr ^ 1
        log.append((c.rd, wr, rebuild, c.wait_wr, c.wait_rd, s.newest))
    return log


def test_order_choice(L):
    # first frame: the default order, its costs sorted behind it into order[0], nothing to wait for
    assert replay(L, [0]) == [(-1, 0, 1, 0, 0, 0)]
    # a still camera: one build, and every later frame reads it -- the newest -- waiting for it once (frame 1, where it may still run;
    # from then on a wait on the event of a finished build)
    still = replay(L, [0, 0, 0, 0])
    assert [f[0] for f in still] == [-1, 0, 0, 0] and [f[2] for f in still] == [1, 0, 0, 0] and all(f[0] == f[5] for f in still[1:])
    assert [f[1] for f in still] == [0, 1, 0, 1] and still[1][3:5] == (0, 1)
    # a moving camera: every frame is sorted behind it, and frame k reads the order built behind frame k - 2 (never the one that may still run)
    moving = replay(L, [1] * 6)
    assert all(f[2] for f in moving) and [f[0] for f in moving] == [-1, 0, 0, 1, 0, 1]
    for k, (rd, wr, _, wait_wr, wait_rd, newest) in enumerate(moving):
        if k >= 2:
            assert rd == wr == k & 1 and wait_wr == 1 and wait_rd == 0      # order[k & 1] was built behind frame k - 2; this frame overwrites it after it
            assert newest == wr
    # the scene changes once, at frame 3 of a still view: one more build, then the view settles on it
    once = replay(L, [0, 0, 0, 1, 0, 0, 0])
    assert [f[2] for f in once] == [1, 0, 0, 1, 0, 0, 0] and once[3][5] == 1
    assert [f[0] for f in once] == [-1, 0, 0, 0, 0, 1, 1]      # frame 4 still reads the old order (the new one may still run), then the newest
    # a grid build refines its first order once, from the first sorted frame
    assert [f[2] for f in replay(L, [0] * 5, grid=True)] == [1, 1, 0, 0, 0]
    assert [f[2] for f in replay(L, [0, 0, 0, 1, 0, 0], grid=True)] == [1, 1, 0, 1, 1, 0]


# ------------------------------------------------------------------ every flag word has a kernel
SCENES = [(0, 0, 0, 0), (1, 0, 3, 0), (4, 2, 3, 0), (5, 2, 3, 0), (16, 1, 3, 0), (17, 3, 4, 0), (64, 2, 3, 0), (256, 2, 3, 0), (300, 1, 3, 1)]      # (.., grid)
DEPTHS = (1, 4, 5, 8, 9, 16, 17, 32)
RANGES = [pc.gen(64, 48), pc.gen(64, 48, id_offset=10), pc.gen(64, 48, band_stride=2, band_phase=1), pc.gen(1800, 1600)]
KNOWN_HOLES = []      # (build, flag word, reason): points of the walk whose launch ends in "Couldn't run the kernel" at the parent commit too
assert len(KNOWN_HOLES) <= 5


def test_every_plan_has_a_compiled_kernel(L):
    """The walk of every combination of build, depth, counting, scene, side table, ray buffer, factor, sample table, motion, pass, seed offset,
    accumulation frame, range and variant bit (59.7 million launches): the mode check or the planner refuses, or there is no launch, or the flag
    word has a kernel in that build."""
    dt = np.dtype(pc.PlanIn)
    inner = list(itertools.product((0, 1), DEPTHS, (0, 1), range(len(SCENES)), (0, 1), (0, 5), range(len(RANGES)), (0,) + pc.VARIANT_BITS))
    strict, depth, counting, scene, lpt, seed, rng, variant = (np.array(c) for c in zip(*inner))
    base = np.zeros(len(inner), dt)
    base[:] = np.frombuffer(bytes(plan_in()), dt)[0]
    sc = np.array(SCENES)[scene]
    base["strict"], base["depth"], base["counting"], base["seed_offset"], base["variant"] = strict, depth, counting, seed, variant
    base["ns"], base["np"], base["nl"], base["grid_usable"], base["have_lpt"] = sc[:, 0], sc[:, 1], sc[:, 2], sc[:, 3], lpt
    base["geom_f4"] = [pc.geom_f4(*SCENES[s][:3], l) for s, l in zip(scene, lpt)]
    gens = np.frombuffer(b"".join(bytes(g) for g in RANGES), np.dtype(pc.Raygen))
    base["gen"] = gens[rng]
    n = gens["n_items"][rng].astype(np.uint64)
    base["array_size"], base["total"], base["out_size"], base["rays_size"] = n, n, 4 * n, 64 * n
    cams = np.zeros((64, 12), np.float32)
    disp = np.ones(3 * 300, np.float32)
    status, flags = np.zeros(len(inner), np.int32), np.zeros(len(inner), np.int32)
    seen, launches, points = {}, 0, 0
    for rays, n_ss, table, moving, pas, acc in itertools.product(("fused", "own", "caller", "exposed"), (1, 2, 4, 8), ("none", "cams", "lens"), (0, 1),
                                                                 (PASS_PLAIN, PASS_BASE, PASS_REFINE), (-1, 0, 3)):
        a = base.copy()
        a["fuse"], a["rays_generated"], a["rays_exposed"] = rays != "own", rays != "caller", rays == "exposed"
        a["supersample"], a["pass_"], a["adaptive"], a["acc_frame"] = n_ss, pas, -1 if pas == PASS_PLAIN else 16, acc
        if table == "cams":
            a["cams"], a["n_cams"] = cams.ctypes.data, n_ss * n_ss
        if table == "lens":
            a["aperture"] = 0.25
        if moving:
            a["disp"], a["n_disp"] = disp.ctypes.data, 3 * a["ns"]
        L.wt_plan_many(a.ctypes.data, len(a), status.ctypes.data, flags.ctypes.data)
        points += len(a)
        ok = status == LAUNCH
        launches += int(ok.sum())
        assert np.isin(status, (LAUNCH, NONE, REFUSED)).all() and (flags[~ok] == -1).all()
        for key in np.unique(flags[ok].astype(np.int64) * 2 + a["strict"][ok]):
            seen.setdefault((int(key) & 1, int(key) >> 1), (rays, n_ss, table, moving, pas, acc))
    assert points == 59719680 and launches > 1000000 and len(seen) > 200
    holes = {(s, f): why for (s, f), why in seen.items() if not (L.wt_strict_has_trace if s else L.wt_fast_has_trace)(f)}
    assert set(holes) == {(s, f) for s, f, _ in KNOWN_HOLES}, {k: (hex(k[1]), v) for k, v in holes.items()}
