"""The ctypes mirror of the launch planner's test seam (csrc/launch_plan.h: wt_plan_in, wt_plan_out and the wt_* functions the library exports
for the tests), and inputs for it.  test_launch_plan_host.py holds the mirror to the sizes the library reports (wt_plan_sizes)."""
import ctypes as C

import numpy as np

from example_gui_opencl_raytracer_amd import api

f32, u32, i32, u64, vp = C.c_float, C.c_uint32, C.c_int32, C.c_uint64, C.c_void_p
CAM_TABLE_FLOATS = 64 * 12
PASS_PLAIN, PASS_BASE, PASS_REFINE = 0, 1, 2
LAUNCH, NONE, REFUSED = 0, 1, 2
# the bits of clw_ext_set_variant, as include/hip_wrap_ext.h documents them
VARIANT_BITS = (1, 2, 4, 8, 16, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)


class Raygen(C.Structure):
    _fields_ = [("corner", f32 * 3), ("origin", f32 * 3), ("up", f32 * 3), ("right", f32 * 3), ("w_factor", f32), ("h_factor", f32),
                ("width", u32), ("height", u32), ("id_offset", u64), ("n_items", u32), ("band_stride", u32), ("band_phase", u32)]


class Params(C.Structure):      # whitted_params of csrc/whitted_params.h
    _fields_ = [("corner", f32 * 3), ("origin", f32 * 3), ("up", f32 * 3), ("right", f32 * 3), ("w_factor", f32), ("h_factor", f32),
                ("width", u32), ("height", u32), ("id_offset", u64), ("n_items", u32), ("tiled", u32), ("rows", u32), ("row_offset", u32),
                ("band_stride", u32), ("band_phase", u32), ("tile_order", vp), ("tile_cost", vp), ("tpt_pool", vp), ("tpt_flags", vp),
                ("tpt_jump", vp), ("tpt_slice_words", u32), ("tpt_cap", u32), ("tpt_slots", u32), ("tpt_max", u32), ("tpt_min", u32),
                ("tpt_clock", u32), ("cost_sum", u32), ("depth", i32), ("untrimmed", u32), ("geom", vp), ("ptex", vp), ("spheres_raw", vp),
                ("planes_raw", vp), ("ns", u32), ("np", u32), ("nl", u32), ("through", f32), ("geom_f4", u32), ("unit_dirs", u32), ("lpt", u32),
                ("vis", u32), ("diag", u32), ("grid_start", vp), ("grid_items", vp), ("grid_box", vp), ("grid_geom", vp), ("grid_min", f32 * 3),
                ("grid_inv", f32 * 3), ("grid_cell", f32 * 3), ("grid_pair", u32), ("grid_res", i32 * 3), ("tex", vp), ("tex_w", i32),
                ("tex_h", i32), ("tex_layers", i32), ("sky", vp), ("sky_w", i32), ("sky_h", i32), ("rays", vp), ("out", vp), ("out_rgb", vp),
                ("counters", vp), ("ss_lg", u32), ("ss_cams", vp), ("ss_disp", vp), ("ss_times", vp), ("list_count", vp), ("acc_sum", vp),
                ("acc_scale", f32), ("seed_offset", u32)]


class PlanIn(C.Structure):
    _fields_ = [("depth", i32), ("strict", i32), ("fuse", i32), ("counting", i32), ("stamps", i32), ("tpt_clock", i32), ("variant", i32),
                ("supersample", i32), ("adaptive", i32), ("seed_offset", u32), ("acc_frame", i32), ("acc_jitter", i32), ("aperture", f32),
                ("focus", f32), ("through", f32), ("tpt_max", u32), ("tpt_pool_mb", u32), ("tpt_min", u32), ("split_min_quota", u32),
                ("occ_tiles_per_depth", u32), ("sched", i32), ("diag", u32), ("id_offset", u64), ("band_stride", u32), ("scene_ok", i32),
                ("ns", u32), ("np", u32), ("nl", u32), ("geom_f4", u32), ("have_lpt", i32), ("grid_usable", i32), ("args_ok", i32),
                ("rays_generated", i32), ("rays_exposed", i32), ("gen", Raygen), ("rays_size", u64), ("array_size", u64), ("out_size", u64),
                ("total", u32), ("has_strip", i32), ("strip_row0", u32), ("strip_rows", u32), ("pass_", i32), ("cams", vp), ("times", vp),
                ("disp", vp), ("n_cams", u32), ("n_times", u32), ("n_disp", u32), ("explicit_times", i32)]


class PlanOut(C.Structure):
    _fields_ = [("status", i32), ("flags", i32), ("grid", u32), ("dyn_lds", u32), ("P", Params), ("out_offset", u64), ("out_pixels", u32),
                ("fused", i32), ("need_counters", i32), ("ss", i32), ("trows", u32), ("tpr", u32), ("per_share", u32), ("per_share_cap", u32),
                ("use_order", i32), ("split", i32), ("split_max_lg", u32), ("tail_wanted", i32), ("tpt_slice", u32), ("tpt_cap", u32),
                ("tpt_nslots", u32), ("sig", Raygen), ("samples_decided", i32), ("n_cams", u32), ("n_times", u32), ("motion_floats", u32),
                ("message", C.c_char * 200), ("cams_used", f32 * (64 * 12)), ("times_used", f32 * 64), ("cam_table", f32 * CAM_TABLE_FLOATS),
                ("motion_table", f32 * (2 * CAM_TABLE_FLOATS))]


class OrderState(C.Structure):
    _fields_ = [("have", i32 * 2), ("wr", i32), ("newest", i32), ("sig_valid", i32), ("sig_age", i32), ("frame", u64), ("newest_frame", u64)]


class OrderChoice(C.Structure):
    _fields_ = [("rd", i32), ("wait_wr", i32), ("wait_rd", i32)]


class GeomClass(C.Structure):
    _fields_ = [("flags", i32), ("dyn_lds", u32), ("lpt", u32), ("vis", u32)]


def seam():
    """The library with the planner's functions typed."""
    L = api.load_library()
    L.wt_plan.argtypes = [C.POINTER(PlanIn), C.POINTER(PlanOut)]
    L.wt_plan.restype = C.c_int
    L.wt_plan_mode_check.argtypes = [C.POINTER(PlanIn), C.c_int, C.c_char_p]
    L.wt_plan_mode_check.restype = C.c_int
    L.wt_plan_range.argtypes = [u64, u32, u64]
    L.wt_plan_range.restype = u64
    L.wt_plan_lane_sample.argtypes = [u32, u32]
    L.wt_plan_lane_sample.restype = u32
    L.wt_plan_grid.argtypes = [C.POINTER(Params)]
    L.wt_plan_grid.restype = u32
    L.wt_plan_fused_range.argtypes = [C.POINTER(Raygen), u32, C.POINTER(Params)]
    L.wt_plan_fused_range.restype = None
    L.wt_plan_geometry.argtypes = [C.c_int, C.c_int, u32, u32, u32, C.c_int, C.c_int]
    L.wt_plan_geometry.restype = GeomClass
    L.wt_order_choose.argtypes = [C.POINTER(OrderState)]
    L.wt_order_choose.restype = OrderChoice
    L.wt_order_rebuild.argtypes = [C.POINTER(OrderState), C.c_int, C.c_int]
    L.wt_order_rebuild.restype = C.c_int
    L.wt_order_launched.argtypes = [C.POINTER(OrderState), C.c_int]
    L.wt_order_launched.restype = None
    for f in (L.wt_fast_has_trace, L.wt_strict_has_trace):
        f.argtypes, f.restype = [C.c_int], C.c_int
    L.wt_plan_sizes.argtypes = [u32 * 3]
    L.wt_plan_sizes.restype = None
    L.wt_plan_many.argtypes = [vp, C.c_size_t, vp, vp]
    L.wt_plan_many.restype = None
    return L


def geom_f4(ns, npl, nl, lpt):
    """float4s of the prepared geometry (scene_prep.c: wprep_geom_f4 + wprep_lpt_f4)"""
    side = (nl + 2) // 3 * npl
    return ns + 2 * npl + 2 * nl + (side if lpt and side <= 64 else 0)


def gen(width, height, id_offset=0, n_items=None, band_stride=1, band_phase=0):
    """What a raygen launch over the whole frame (or the given range of it) latches; the camera is CAMERA-like but arbitrary"""
    g = Raygen()
    g.corner[:], g.origin[:], g.up[:], g.right[:] = (-1.0, 0.75, 1.0), (0.8, 2.5, -8.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
    g.w_factor, g.h_factor, g.width, g.height = 2.0 / width, 1.5 / height, width, height
    g.id_offset, g.band_stride, g.band_phase = id_offset, band_stride, band_phase
    g.n_items = width * height // band_stride - id_offset if n_items is None else n_items
    return g


_keep = []      # the tables the inputs point to


def plan_in(width=64, height=48, scene=(4, 2, 3), lpt=None, rays="fused", cams=None, times=None, disp=None, **kw):
    """A launch as hip_wrap.cpp describes it to the planner.  Defaults: the fast build at depth 4, a fused whole-frame launch of width x
    height over a (spheres, planes, lights) scene with its side table, every knob at the shim's default.  rays: 'fused' | 'own' (this
    library's rays, CLWRAP_FUSE=0) | 'caller' (rays the caller wrote) | 'exposed' (generated, then handed out)."""
    ns, npl, nl = scene
    lpt = (npl > 0 and nl > 0) if lpt is None else lpt
    i = PlanIn(depth=4, fuse=rays != "own", supersample=1, adaptive=-1, acc_frame=-1, acc_jitter=1, focus=1.0, through=0.8, tpt_max=40,
               tpt_pool_mb=8192, tpt_min=4, split_min_quota=1500, occ_tiles_per_depth=9000, sched=1, band_stride=1, scene_ok=1, ns=ns, np=npl,
               nl=nl, geom_f4=geom_f4(ns, npl, nl, lpt), have_lpt=lpt, args_ok=1, rays_generated=rays != "caller", rays_exposed=rays == "exposed",
               gen=gen(width, height), rays_size=64 * width * height, array_size=width * height, out_size=4 * width * height,
               total=width * height, pass_=PASS_PLAIN)
    for name, table, per in (("cams", cams, 12), ("times", times, 1), ("disp", disp, 1)):
        if table is not None:
            a = np.ascontiguousarray(table, np.float32)
            _keep.append(a)
            setattr(i, name, a.ctypes.data)
            setattr(i, "n_" + name, a.size // per)
    i.explicit_times = times is not None
    for k, v in kw.items():
        assert hasattr(i, k), k
        setattr(i, k, v)
    return i


def plan(L, i):
    o = PlanOut()
    st = L.wt_plan(C.byref(i), C.byref(o))
    assert st == o.status
    return o


def refusal(L, i, accumulating=None):
    """The text a trace call of this launch ends with ('' = none): the mode check first, as run_raytracer applies it, then the plan."""
    msg = C.create_string_buffer(200)
    if L.wt_plan_mode_check(C.byref(i), i.acc_frame >= 0 if accumulating is None else accumulating, msg):
        return msg.value.decode()
    o = plan(L, i)
    return o.message.decode() if o.status == REFUSED else ""
