"""ctypes mirror of the C-ABI boundary (include/opencl_wrap.h, include/hip_wrap_ext.h).

The functions keep the reference's names, argument order and meaning
(reference src/opencl_wrap.h:29-42).  ``ClWrap`` is a thin object wrapper so tests read
like the reference drivers (raypng.c:31-89).  There is no CPU fallback here: if the
HIP library is missing the import of the library raises, and without a GPU
``cl_wrap_init`` terminates the process exactly like the reference does without an
OpenCL device (opencl_wrap.c:31-34).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLWRAP_LIB") or os.path.join(HERE, "libopencl_wrap_hip.so")   # CLWRAP_LIB: A/B builds

MAX_KERNELS = 16  # __MAX_KERNELS, opencl_wrap.h:6
MAX_BUFFERS = 32  # __MAX_BUFFERS, opencl_wrap.h:7

CL_DEVICE_TYPE_GPU = 1 << 2
CL_MEM_READ_WRITE = 1 << 0
CL_MEM_WRITE_ONLY = 1 << 1
CL_MEM_READ_ONLY = 1 << 2
CL_MEM_COPY_HOST_PTR = 1 << 5

# the channels of the primary-hit pass (hip_wrap_ext.h: CLW_GB_*), the id of a miss and the pass's id in the timing log
GB_DEPTH, GB_ID, GB_NORMAL, GB_POINT, GB_ALBEDO, GB_ALL = 1, 2, 4, 8, 16, 31
ID_NONE = 0xFFFFFFFF
ID_SPHERE, ID_PLANE, ID_LIGHT = 0, 1, 2
TIMING_GBUFFER = 0x47425546
GB_CHANNELS = {"depth": (GB_DEPTH, np.float32, 1), "id": (GB_ID, np.uint32, 1), "normal": (GB_NORMAL, np.float32, 3),
               "point": (GB_POINT, np.float32, 3), "albedo": (GB_ALBEDO, np.float32, 3)}     # name -> (bit, dtype, entries per work-item)

# the selection overlay (hip_wrap_ext.h: CLW_OV_*): what a style draws, and the pass's id in the timing log
OV_OUTLINE, OV_FILL, OV_EDGES, OV_ALL = 1, 2, 4, 7
TIMING_OVERLAY = 0x4F564C59

# the visible-object table (hip_wrap_ext.h: clw_object_stat; OBJECT_STAT below is a record as a numpy dtype): the pass's id in the timing log
TIMING_OBJECTS = 0x4F424A53

# the camera models (hip_wrap_ext.h: CLW_PROJ_*)
PROJ_PERSPECTIVE, PROJ_ORTHO, PROJ_EQUIRECT = 0, 1, 2
PROJ_MODELS = {"perspective": PROJ_PERSPECTIVE, "ortho": PROJ_ORTHO, "equirect": PROJ_EQUIRECT}

# ambient occlusion (hip_wrap_ext.h: CLW_AO_*): the flags of a clw_ao, what clw_ext_read_ao reads, and the two kernels' ids in the timing log
AO_FILTER, AO_COMPOSE = 1, 2
AO_FRAME, AO_COUNTS = 0, 1
TIMING_AO = 0x414F5452
TIMING_AO_RESOLVE = 0x414F5253

# ray queries (hip_wrap_ext.h: clw_ray, clw_hit, CLW_CAST_*; RAY_QUERY and HIT below are a ray and a hit as numpy dtypes): the kinds a query
# tests, and the kernel's id in the timing log
CAST_SPHERES, CAST_PLANES, CAST_LIGHTS, CAST_KINDS, CAST_OPAQUE = 1, 2, 4, 7, 8
CAST_KIND_NAMES = {"sphere": CAST_SPHERES, "plane": CAST_PLANES, "light": CAST_LIGHTS}
TIMING_CAST = 0x43415354

# layered ray queries (hip_wrap_ext.h: clw_layer, clw_host_cast_layers; LAYER below is one entry of a ray's list as a numpy dtype): the
# largest K, what clw_ext_read_layers reads, and the two kernels' ids in the timing log
LAYERS_MAX = 8
LAYERS_T, LAYERS_ID = 0, 1
TIMING_LAYERS = 0x4C415952
TIMING_CAMRAYS = 0x43524159

# path queries (hip_wrap_ext.h: CLW_PATH_*, clw_host_cast_paths): the two flags beside the ray queries', the largest number of segments, why a
# path ended (the high half of its status byte; the low half is the count of recorded hits), and the kernel's id in the timing log
PATH_TRANSMIT, PATH_ALL_SURFACES = 16, 32
PATH_MAX_BOUNCES = 8
PATH_REASON_BOUNCES, PATH_REASON_MISSED, PATH_REASON_ENDED = 0, 1, 2
PATH_EPSILON = np.float32(0.001)      # the reference's EPSILON: a segment starts at point + normal * EPSILON of the hit before it
TIMING_PATHS = 0x50415448

# proximity queries (hip_wrap_ext.h: clw_probe, clw_host_nearest_surface; PROBE below is a probe as a numpy dtype): the kernel's id in the
# timing log
TIMING_NEAR = 0x4E454152


def id_kind(ids):
    """Kind of the entries of an id channel (0 sphere, 1 plane, 2 light; 3 for ID_NONE)."""
    return np.asarray(ids, np.uint32) >> np.uint32(30)


def id_index(ids):
    """Index into the caller's sphere / plane / light array of the entries of an id channel (meaningless for ID_NONE)."""
    return np.asarray(ids, np.uint32) & np.uint32(0x3FFFFFFF)


def make_id(kind, index):
    """kind << 30 | index, as the id channel stores it."""
    return (np.asarray(kind, np.uint32) << np.uint32(30)) | np.asarray(index, np.uint32)


def id_entry(word, **more) -> dict:
    """{"id", "kind", "index"} of one id word as Python ints, then `more`: what ``Renderer.pick`` and ``pick_through`` answer per object."""
    word = int(word)
    return dict(id=word, kind=word >> 30, index=word & 0x3FFFFFFF, **more)


def library_version() -> str:
    """clw_ext_version(): 'opencl_wrap_hip <ver> gfx950 fast+strict kernels:<sha256/16 of the device sources>'."""
    return load_library().clw_ext_version().decode()


def kernel_source_hash() -> str:
    return library_version().rsplit("kernels:", 1)[-1]


class cl_wrap(C.Structure):
    """Layout of ``struct cl_wrap`` in include/opencl_wrap.h."""
    _fields_ = [
        ("impl", C.c_void_p),
        ("kernels_num", C.c_uint32),
        ("buffers_num", C.c_uint32 * MAX_KERNELS),
        ("buffers_ids", (C.c_uint32 * MAX_BUFFERS) * MAX_KERNELS),
        ("buffers", (C.c_void_p * MAX_BUFFERS) * MAX_KERNELS),
    ]


class clw_camera(C.Structure):
    _fields_ = [("im_corner", C.c_float * 3), ("origin", C.c_float * 3), ("up", C.c_float * 3),
                ("right", C.c_float * 3), ("w_factor", C.c_float), ("h_factor", C.c_float),
                ("width", C.c_uint32), ("height", C.c_uint32)]


class clw_sample_camera(C.Structure):
    """One entry of a table of sample cameras (48 bytes): row k of the float32 [n*n, 12] arrays below."""
    _fields_ = [("im_corner", C.c_float * 3), ("origin", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3)]


class clw_pick(C.Structure):
    """What clw_ext_pick returns (44 bytes): the entries of one pixel in the channels of the primary-hit pass."""
    _fields_ = [("id", C.c_uint32), ("depth", C.c_float), ("point", C.c_float * 3), ("normal", C.c_float * 3), ("albedo", C.c_float * 3)]


class clw_overlay(C.Structure):
    """The style of a selection overlay (24 bytes): what to draw (OV_* bits), the outline's width and the three colours, 0x00RRGGBB."""
    _fields_ = [("flags", C.c_uint32), ("radius", C.c_uint32), ("outline_rgb", C.c_uint32), ("fill_rgb", C.c_uint32), ("fill_alpha", C.c_uint32),
                ("edge_rgb", C.c_uint32)]


class clw_ao(C.Structure):
    """The parameters of an ambient occlusion pass (16 bytes): AO_* flags, rays per pixel (1..32), the rays' length, strength 0..256."""
    _fields_ = [("flags", C.c_uint32), ("rays", C.c_uint32), ("radius", C.c_float), ("strength", C.c_uint32)]


class clw_ray(C.Structure):
    """A query ray (32 bytes): origin, the largest t it reaches (inf = unlimited), direction (not normalised: t is in units of its length),
    the id word of the one primitive it does not test (ID_NONE = none)."""
    _fields_ = [("origin", C.c_float * 3), ("tmax", C.c_float), ("dir", C.c_float * 3), ("ignore", C.c_uint32)]


class clw_hit(C.Structure):
    """What a nearest-hit query answers per ray (32 bytes): t (inf = a miss), the id word (ID_NONE = a miss), the normal and the point."""
    _fields_ = [("t", C.c_float), ("id", C.c_uint32), ("normal", C.c_float * 3), ("point", C.c_float * 3)]


class clw_layer(C.Structure):
    """One entry of a ray's layer list (8 bytes): t (inf = empty) and the id word (ID_NONE = empty)."""
    _fields_ = [("t", C.c_float), ("id", C.c_uint32)]


class clw_probe(C.Structure):
    """One probe of a proximity query (16 bytes): a point and how far it reaches (inf = unlimited; negative = only penetrations that deep)."""
    _fields_ = [("point", C.c_float * 3), ("reach", C.c_float)]


class clw_rect(C.Structure):
    """A rectangle in frame pixels (16 bytes)."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class clw_object_stat(C.Structure):
    """One record of the visible-object table (48 bytes): an element of an OBJECT_STAT array."""
    _fields_ = [("id", C.c_uint32), ("pixels", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32),
                ("depth_min", C.c_float), ("depth_max", C.c_float), ("sum_x", C.c_uint64), ("sum_y", C.c_uint64)]


class clw_object_summary(C.Structure):
    """What comes with a visible-object table (16 bytes): records, pixels inside the rectangle, pixels whose id is not known."""
    _fields_ = [("objects", C.c_uint32), ("pixels", C.c_uint32), ("foreign", C.c_uint32), ("reserved", C.c_uint32)]


class clw_projection(C.Structure):
    """A camera model beside the pinhole (32 bytes): PROJ_ORTHO or PROJ_EQUIRECT, the view axis (all zero = the camera's own centre direction),
    the world width an orthographic frame spans (0 = the camera's image plane as it stands), the degrees a panorama covers (0 = 360 / 180)."""
    _fields_ = [("model", C.c_uint32), ("axis", C.c_float * 3), ("ortho_width", C.c_float), ("h_span", C.c_float), ("v_span", C.c_float),
                ("reserved", C.c_uint32)]


class clw_grid_info(C.Structure):
    """What clw_ext_get_grid returns: the uniform grid of the scene as last prepared."""
    _fields_ = [("built", C.c_int32), ("pair", C.c_int32), ("res", C.c_int32 * 3), ("ncells", C.c_uint32), ("pairs", C.c_uint64),
                ("cell", C.c_float * 3), ("gmin", C.c_float * 3), ("reg_pad", C.c_float)]


# the records that travel in arrays, as numpy dtypes: derived from their Structure, so each layout is written once (32, 32, 8, 48 and 16 bytes)
RAY_QUERY, HIT, LAYER, OBJECT_STAT = np.dtype(clw_ray), np.dtype(clw_hit), np.dtype(clw_layer), np.dtype(clw_object_stat)
PROBE = np.dtype(clw_probe)

_int, _u32, _u64, _sz, _f32, _vp, _str = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float, C.c_void_p, C.c_char_p
_f3, _pu32 = C.c_float * 3, C.POINTER(C.c_uint32)
_W, _CAM, _PROJ, _OV, _AO = C.POINTER(cl_wrap), C.POINTER(clw_camera), C.POINTER(clw_projection), C.POINTER(clw_overlay), C.POINTER(clw_ao)
_RECT, _SUM = C.POINTER(clw_rect), C.POINTER(clw_object_summary)

# THE prototype table: every function include/opencl_wrap.h and include/hip_wrap_ext.h declare, name -> (return type, argument types), in the
# headers' order.  None as the return type is `void`; None as the argument types is a variadic function, whose callers convert each argument
# themselves.  tests/test_api_prototypes_host.py holds every line to its header prototype.  A new entry point is its header prototype, one
# line here and its method below.
PROTOTYPES = {
    "cl_wrap_init": (None, None),
    "cl_wrap_load_global_data": (None, [_W, _u32, _u32, _vp, _sz, _u64]),
    "cl_wrap_load_single_data": (None, [_W, _u32, _u32, _vp, _sz]),
    "cl_wrap_load_images": (None, None),
    "cl_wrap_output": (None, [_W, _sz, _sz, _u32, _u32, C.c_int32, _vp]),
    "cl_wrap_release": (None, [_W]),
    "clw_ext_set_depth": (None, [_W, _int]),
    "clw_ext_get_depth": (_int, [_W]),
    "clw_ext_set_strict": (None, [_W, _int]),
    "clw_ext_set_fuse": (None, [_W, _int]),
    "clw_ext_set_id_offset": (None, [_W, _u64]),
    "clw_ext_set_row_bands": (None, [_W, _u32, _u32]),
    "clw_ext_set_async": (None, [_W, _int]),
    "clw_ext_sync": (None, [_W]),
    "clw_ext_set_stream": (None, [_W, _vp]),
    "clw_ext_timing_reset": (None, [_W]),
    "clw_ext_timing_get": (None, [_W, _u32, _pu32, C.POINTER(C.c_double)]),
    "clw_ext_set_pipeline": (None, [_W, _int]),
    "clw_ext_set_timing_every": (None, [_W, _u32]),
    "clw_ext_load_images_raw": (None, [_W, _u32, _u32, _vp, _u32, _u32, _u32]),
    "clw_ext_bind_device_buffer": (None, [_W, _u32, _u32, _vp, _sz]),
    "clw_ext_invalidate_scene": (None, [_W]),
    "clw_ext_device_ptr": (_vp, [_W, _u32, _u32]),
    "clw_ext_set_debug_rgb": (None, [_W, _vp]),
    "clw_ext_set_supersample": (None, [_W, _int]),
    "clw_ext_get_supersample": (_int, [_W]),
    "clw_ext_set_sample_cameras": (None, [_W, _vp, _u32]),
    "clw_ext_get_sample_cameras": (_u32, [_W, _vp, _u32]),
    "clw_ext_set_lens": (None, [_W, _f32, _f32]),
    "clw_ext_set_sphere_motion": (None, [_W, _vp, _u32, _vp, _u32]),
    "clw_ext_get_sample_times": (_u32, [_W, _vp, _u32]),
    "clw_ext_set_adaptive": (None, [_W, _int]),
    "clw_ext_get_adaptive": (_int, [_W]),
    "clw_ext_read_refine_mask": (_u32, [_W, _vp, _u32]),
    "clw_ext_set_seed_offset": (None, [_W, _u32]),
    "clw_ext_get_seed_offset": (_u32, [_W]),
    "clw_ext_set_accumulate": (None, [_W, _int, _int]),
    "clw_ext_get_accumulated": (_u32, [_W]),
    "clw_ext_reset_accumulation": (None, [_W]),
    "clw_ext_render_gbuffer": (_u32, [_W, _u32]),
    "clw_ext_read_gbuffer": (_u32, [_W, _u32, _vp, _u32]),
    "clw_ext_gbuffer_device_ptr": (_vp, [_W, _u32]),
    "clw_ext_pick": (_int, [_W, _u32, _u32, C.POINTER(clw_pick)]),
    "clw_host_overlay": (_int, [_vp, _vp, _u32, _u32, _OV, _vp, _u32, _vp]),
    "clw_ext_render_overlay": (_u32, [_W, _OV, _vp, _u32]),
    "clw_ext_read_overlay": (_u32, [_W, _vp, _u32]),
    "clw_ext_overlay_device_ptr": (_vp, [_W]),
    "clw_ext_unit_overlay": (_u32, [_W, _vp, _vp, _u32, _u32, _OV, _vp, _u32, _vp]),
    "clw_host_object_stats": (_int, [_vp, _vp, _u32, _u32, _u32, _RECT, _vp, _vp, _u32, _SUM]),
    "clw_host_merge_object_stats": (_u32, [_vp, _u32, _vp, _u32, _vp, _u32]),
    "clw_ext_object_stats": (_int, [_W, _RECT, _vp, _u32, _SUM]),
    "clw_ext_unit_object_stats": (_int, [_W, _vp, _vp, _u32, _u32, _u32, _RECT, _vp, _vp, _u32, _SUM]),
    "clw_host_projection_rays": (_int, [_CAM, _PROJ, _u64, _u64, _vp]),
    "clw_host_projection_tables": (_int, [_CAM, _PROJ, _vp, _vp]),
    "clw_host_ortho_camera": (_int, [_f3, _f3, _f32, _u32, _u32, _CAM, _PROJ]),
    "clw_ext_set_projection": (None, [_W, _PROJ]),
    "clw_ext_get_projection": (None, [_W, _PROJ]),
    "clw_ext_unit_projection": (_int, [_W, _CAM, _PROJ, _u64, _u64, _vp]),
    "clw_host_ao_dirs": (_int, [_u32, _vp]),
    "clw_host_ao_open": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _AO, _vp, _vp]),
    "clw_host_ao_resolve": (_int, [_vp, _vp, _vp, _u32, _u32, _AO, _vp]),
    "clw_ext_render_ao": (_u32, [_W, _AO]),
    "clw_ext_read_ao": (_u32, [_W, _u32, _vp, _u32]),
    "clw_ext_ao_device_ptr": (_vp, [_W, _u32]),
    "clw_ext_unit_ao_open": (_u32, [_W, _vp, _vp, _vp, _u32, _u32, _u32, _AO, _vp]),
    "clw_ext_unit_ao_resolve": (_u32, [_W, _vp, _vp, _vp, _u32, _u32, _AO, _vp]),
    "clw_host_cast_rays": (_int, [_vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "clw_host_occluded_rays": (_int, [_vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "clw_ext_cast_rays": (_u32, [_W, _vp, _u32, _u32, _vp]),
    "clw_ext_occluded_rays": (_u32, [_W, _vp, _u32, _u32, _vp]),
    "clw_ext_cast_rays_device": (_u32, [_W, _vp, _u32, _u32, _vp, _vp]),
    "clw_host_cast_layers": (_int, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "clw_host_camera_rays": (_int, [_CAM, _PROJ, _u64, _u64, _vp]),
    "clw_ext_cast_layers": (_u32, [_W, _vp, _u32, _u32, _u32, _vp, _vp]),
    "clw_ext_cast_layers_device": (_u32, [_W, _vp, _u32, _u32, _u32, _vp, _vp]),
    "clw_ext_camera_rays": (_u32, [_W, _vp, _u32]),
    "clw_ext_camera_rays_device": (_u32, [_W, _vp, _u32]),
    "clw_ext_render_layers": (_u32, [_W, _u32, _u32]),
    "clw_ext_read_layers": (_u32, [_W, _u32, _vp, _u32]),
    "clw_ext_layers_device_ptr": (_vp, [_W, _u32]),
    "clw_ext_pick_layers": (_int, [_W, _u32, _u32, _u32, _u32, _vp]),
    "clw_host_cast_paths": (_int, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "clw_ext_cast_paths": (_u32, [_W, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "clw_ext_cast_paths_device": (_u32, [_W, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "clw_ext_pick_path": (_int, [_W, _u32, _u32, _u32, _u32, _vp, _vp]),
    "clw_host_nearest_surface": (_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "clw_host_within_reach": (_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp]),
    "clw_host_near_surfaces": (_int, [_vp, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _vp, _vp]),
    "clw_ext_nearest_surface": (_u32, [_W, _vp, _vp, _u32, _u32, _vp]),
    "clw_ext_within_reach": (_u32, [_W, _vp, _vp, _u32, _u32, _vp]),
    "clw_ext_near_surfaces": (_u32, [_W, _vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "clw_ext_probe_device": (_u32, [_W, _vp, _vp, _u32, _u32, _vp, _vp]),
    "clw_ext_near_surfaces_device": (_u32, [_W, _vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "clw_ext_enable_counters": (None, [_W, _int]),
    "clw_ext_read_counters": (None, [_W, C.POINTER(_u64 * 8)]),
    "clw_ext_read_counters_ex": (None, [_W, C.POINTER(_u64 * 32), _u32]),
    "clw_ext_set_shadow_through": (None, [_W, _f32]),
    "clw_ext_set_grid": (None, [_W, _int]),
    "clw_ext_get_grid": (_int, [_W, C.POINTER(clw_grid_info)]),
    "clw_ext_set_grid_pair": (None, [_W, _int]),
    "clw_ext_set_tile_sched": (None, [_W, _int]),
    "clw_ext_read_tile_costs": (_u32, [_W, _vp, _u32]),
    "clw_ext_unit": (None, [_W, _int, _vp, _u32, _vp, _u32, _u32, _u32]),
    "clw_ext_unit_sched": (_u32, [_W, _vp, _u32, _u32, _int, _u32, _u32, _u32, _u32, _vp, _u32]),
    "clw_ext_read_tile_order": (_u32, [_W, _vp, _u32, _pu32]),
    "clw_ext_set_split": (None, [_W, _int, _int]),
    "clw_ext_get_split": (None, [_W, _pu32, _pu32, _pu32]),
    "clw_ext_unit_scene": (None, [_W, _u32, _int, _vp, _u32, _vp, _u32, _u32]),
    "clw_ext_set_variant": (None, [_W, _int]),
    "clw_ext_last_trace_flags": (_int, [_W]),
    "clw_host_primary_cull": (_u32, [_CAM, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp]),
    "clw_ext_read_primary_cull": (_u32, [_W, _vp, _u32, C.POINTER(_u64)]),
    "clw_host_bounce_cull": (_u32, [_CAM, _u32, _u32, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _u32, _vp]),
    "clw_ext_read_bounce_cull": (_u32, [_W, _vp, _u32]),
    "clw_ext_set_bounce_cull": (None, [_W, _int]),
    "clw_ext_set_tpt": (None, [_W, _int, _int, _int]),
    "clw_ext_get_tpt": (None, [_W, _pu32, _pu32, _pu32]),
    "clw_host_perspective": (_int, [_f3, _f3, _f32, _f32, _u32, _u32, _CAM]),
    "clw_host_lens_cameras": (_int, [_CAM, _f32, _f32, _u32, _vp]),
    "clw_host_shutter_cameras": (_int, [_CAM, _CAM, _u32, _vp]),
    "clw_host_sample_times": (_int, [_u32, _vp]),
    "clw_host_spheres_at": (_int, [_vp, _u32, _vp, _f32, _vp]),
    "clw_host_frame_seed": (_u32, [_u32]),
    "clw_host_jitter_camera": (_int, [_CAM, _u32, _u32, _CAM]),
    "clw_host_refine_mask": (_int, [_vp, _u32, _u32, _u32, _int, _vp]),
    "clw_host_write_png": (_int, [_str, _vp, _u32, _u32]),
    "clw_host_write_png_rgba": (_int, [_str, _vp, _u32, _u32]),
    "clw_host_read_png": (_int, [_str, _pu32, _pu32, C.POINTER(_vp)]),
    "clw_host_free": (None, [_vp]),
    "clw_ext_version": (_str, []),
}
SYMBOLS = list(PROTOTYPES)


def bind_prototypes(L, may_be_missing: bool, table=PROTOTYPES):
    """Give every function of `table` its types on the loaded library `L`.  A symbol `L` lacks ends the binding with the AttributeError ctypes
    raises, which names it -- unless `may_be_missing` (an A/B build of another commit): then it is skipped and stays unbound, so
    `hasattr(L, name)` still tells whether the library has it."""
    for name, (restype, argtypes) in table.items():
        if may_be_missing and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    return L


_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the HIP shim.  Fails loudly if it has not been built, and -- unless CLWRAP_LIB names the library, for an A/B run against a build of
    another commit -- if it lacks a symbol of the table."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -m example_gui_opencl_raytracer_amd.build` "
                          "(there is no CPU fallback for the trace path)")
    _lib = bind_prototypes(C.CDLL(path), may_be_missing=bool(os.environ.get("CLWRAP_LIB")))
    return _lib

def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.cast(a, C.c_void_p)


def _fits_u32(*values) -> bool:
    """Whether every value can be passed as a uint32_t (ctypes would wrap a larger or a negative one silently)."""
    return all(0 <= int(v) < 2 ** 32 for v in values)


def _flat(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype).reshape(-1)


def _frame_channels(width, rows, *channels, optional=()):
    """The channels -- (array, dtype, entries per pixel) each -- of a width x rows frame -> (width, rows, [the arrays, contiguous and flat]), the
    `optional` ones (None = left out, and stays None) after the others; None when there is no such frame or a channel has not its entries."""
    width, rows = int(width), int(rows)
    given = [(_flat(a, dtype), per) for a, dtype, per in channels] + [(a if a is None else _flat(a, dtype), per) for a, dtype, per in optional]
    if width <= 0 or rows <= 0 or any(a is not None and a.size != per * width * rows for a, per in given):
        return None
    return width, rows, [a for a, _ in given]


def _read_counted(read, dtype, unit: int | None = None) -> np.ndarray:
    """Something the library holds, of a length only it knows: `read(out, capacity)` is asked for the count with no room at all, then again with
    an array that holds it -> that array, flat; empty when the count is 0.  The count and the capacity are in units of `unit` bytes (None = in
    entries of `dtype`)."""
    itemsize = np.dtype(dtype).itemsize
    n = int(read(None, 0))
    out = np.zeros(n * (unit or itemsize) // itemsize, dtype)
    if n:
        assert read(_ptr(out), n) == n
    return out


def perspective(origin, look, fov, focal, width, height) -> clw_camera:
    """rinit_camera + rgen_perspective (reference src/cpu_ray.c:24-35, 42-106)."""
    L = load_library()
    cam = clw_camera()
    ok = L.clw_host_perspective((C.c_float * 3)(*origin), (C.c_float * 3)(*look), fov, focal, width, height,
                                C.byref(cam))
    if not ok:
        raise ValueError("rgen_perspective rejects this camera (cpu_ray.c:58-63)")
    return cam


def lens_cameras(cam: clw_camera, aperture: float, focus: float, n: int) -> np.ndarray:
    """clw_host_lens_cameras: the thin-lens table of `cam` -> float32 [n*n, 12], rows {im_corner, origin, up, right} in sy * n + sx order."""
    out = np.zeros((max(int(n), 0) ** 2 or 1, 12), np.float32)
    if not load_library().clw_host_lens_cameras(C.byref(cam), aperture, focus, n, _ptr(out)):
        raise ValueError("clw_host_lens_cameras rejects these arguments (n in 2, 4, 8; aperture >= 0; focus > 0)")
    return out


def shutter_cameras(cam0: clw_camera, cam1: clw_camera, n: int) -> np.ndarray:
    """clw_host_shutter_cameras: the n*n cameras of a shutter open from `cam0` to `cam1` -> float32 [n*n, 12]."""
    out = np.zeros((max(int(n), 0) ** 2 or 1, 12), np.float32)
    if not load_library().clw_host_shutter_cameras(C.byref(cam0), C.byref(cam1), n, _ptr(out)):
        raise ValueError("clw_host_shutter_cameras rejects these arguments (n in 2, 4, 8; cameras of one size and one pair of factors)")
    return out


def sample_times(n: int) -> np.ndarray:
    """clw_host_sample_times: the default scene times of the n*n samples of a pixel (the shutter's clock) -> float32 [n*n], sy * n + sx order."""
    out = np.zeros(max(int(n), 0) ** 2 or 1, np.float32)
    if not load_library().clw_host_sample_times(n, _ptr(out)):
        raise ValueError("clw_host_sample_times rejects this factor (n in 2, 4, 8)")
    return out


def spheres_at(spheres: np.ndarray, disp, t: float) -> np.ndarray:
    """clw_host_spheres_at: the 96-byte sphere records of the scene at time t -- centre i = fma(t, disp[i], centre i) in float32, every
    other byte copied -> a new record array of the same dtype."""
    spheres = np.ascontiguousarray(spheres)
    assert spheres.dtype.itemsize == 96
    disp = np.ascontiguousarray(disp, np.float32).reshape(-1, 3)
    assert len(disp) == len(spheres)
    out = spheres.copy()
    if not load_library().clw_host_spheres_at(_ptr(spheres), len(spheres), _ptr(disp), float(t), _ptr(out)):
        raise ValueError("clw_host_spheres_at rejects these arguments")
    return out


def refine_mask(xrgb, width: int, rows: int, n: int, threshold: int) -> np.ndarray:
    """clw_host_refine_mask: the blocks of b x b pixels (b = 8 / n) of a packed width x rows frame that adaptive supersampling refines at this
    contrast threshold -> uint8 [ceil(rows / b), ceil(width / b)] of 0 / 1."""
    got, n = _frame_channels(width, rows, (xrgb, np.uint32, 1)), int(n)
    if n not in (2, 4, 8) or got is None:
        raise ValueError("clw_host_refine_mask rejects these arguments (n in 2, 4, 8; a frame of width * rows pixels)")
    width, rows, (xrgb,) = got
    b = 8 // n
    out = np.zeros((-(-rows // b), -(-width // b)), np.uint8)
    if not load_library().clw_host_refine_mask(_ptr(xrgb), width, rows, n, int(threshold), _ptr(out)):
        raise ValueError("clw_host_refine_mask rejects these arguments (threshold in [0, 256])")
    return out


def overlay_style(flags: int, radius: int = 2, outline: int = 0xFFFF00, fill: int = 0, alpha: int = 0, edges: int = 0) -> clw_overlay:
    """A clw_overlay from its six words (nothing is checked here: the library refuses what hip_wrap_ext.h says it refuses)."""
    return clw_overlay(int(flags), int(radius), int(outline), int(fill), int(alpha), int(edges))


def _selection(sel) -> np.ndarray:
    return _flat(np.zeros(0, np.uint32) if sel is None else sel, np.uint32)


def overlay(frame, ids, width: int, rows: int, style: clw_overlay, sel) -> np.ndarray:
    """clw_host_overlay: the selection overlay of a packed width x rows frame and its id channel, on the host -- THE definition the device pass is
    held to -> uint32 [width * rows].  `sel`: the selected ids (at most 64 words, or None)."""
    got = _frame_channels(width, rows, (frame, np.uint32, 1), (ids, np.uint32, 1))
    if got is None:
        raise ValueError("clw_host_overlay rejects these arguments (a frame and ids of width * rows words each)")
    width, rows, (frame, ids) = got
    sel = _selection(sel)
    out = np.empty(width * rows, np.uint32)
    if not load_library().clw_host_overlay(_ptr(frame), _ptr(ids), width, rows, C.byref(style), _ptr(sel) if sel.size else None, sel.size, _ptr(out)):
        raise ValueError("clw_host_overlay rejects this style or selection (flags in 1..7, radius in 1..4, alpha in 0..256, at most 64 ids)")
    return out


def ao_params(rays: int = 8, radius: float = 1.0, strength: int = 256, filter: bool = True, compose: bool = False) -> clw_ao:
    """A clw_ao from its values (nothing is checked here: the library refuses what hip_wrap_ext.h says it refuses)."""
    return clw_ao((AO_FILTER if filter else 0) | (AO_COMPOSE if compose else 0), int(rays), float(radius), int(strength))


def ao_dirs(rays: int) -> np.ndarray:
    """clw_host_ao_dirs: the direction table of K rays per pixel -> float32 [16, K, 4] (pattern, ray, {x, y, z, 0})."""
    out = np.empty((16, max(int(rays), 0), 4), np.float32)
    if not _fits_u32(rays) or not load_library().clw_host_ao_dirs(int(rays), _ptr(out)):
        raise ValueError("clw_host_ao_dirs rejects this number of rays (1..32)")
    return out


def ao_open(point, normal, ids, width: int, rows: int, first_row: int, spheres, planes, ao: clw_ao, dirs=None) -> np.ndarray:
    """clw_host_ao_open: the open rays of every pixel of a range of whole rows, on the host -- THE definition the device pass is held to ->
    uint8 [width * rows].  point, normal: float32 [n, 3]; ids: uint32 [n]; spheres, planes: the scene's record arrays (or None)."""
    got = _frame_channels(width, rows, (point, np.float32, 3), (normal, np.float32, 3), (ids, np.uint32, 1))
    if got is None:
        raise ValueError("clw_host_ao_open rejects these arguments (point and normal of 3, ids of 1 entry per pixel of width * rows)")
    width, rows, (point, normal, ids) = got
    if dirs is None:
        dirs = ao_dirs(ao.rays)
    dirs = np.ascontiguousarray(dirs, np.float32)
    ns, np_ = (0 if spheres is None else len(spheres)), (0 if planes is None else len(planes))
    out = np.empty(ids.size, np.uint8)
    if dirs.size != 64 * ao.rays or not load_library().clw_host_ao_open(_ptr(point), _ptr(normal), _ptr(ids), width, rows, int(first_row),
                                                                        _ptr(spheres) if ns else None, ns, _ptr(planes) if np_ else None, np_,
                                                                        C.byref(ao), _ptr(dirs), _ptr(out)):
        raise ValueError("clw_host_ao_open rejects these parameters (rays in 1..32, radius > 0, strength in 0..256, known flags)")
    return out


def ao_resolve(open_u8, ids, frame, width: int, rows: int, ao: clw_ao) -> np.ndarray:
    """clw_host_ao_resolve: open-ray counts -> packed pixels, on the host -- THE definition the device pass is held to -> uint32 [width * rows].
    `frame` (read with AO_COMPOSE only) may be None without it."""
    got = _frame_channels(width, rows, (open_u8, np.uint8, 1), (ids, np.uint32, 1), optional=[(frame, np.uint32, 1)])
    if got is None:
        raise ValueError("clw_host_ao_resolve rejects these arguments (counts, ids and frame of width * rows entries each)")
    width, rows, (open_u8, ids, frame) = got
    out = np.empty(width * rows, np.uint32)
    if not load_library().clw_host_ao_resolve(_ptr(open_u8), _ptr(ids), _ptr(frame), width, rows, C.byref(ao), _ptr(out)):
        raise ValueError("clw_host_ao_resolve rejects these parameters (rays in 1..32, radius > 0, strength in 0..256, known flags, a frame with AO_COMPOSE)")
    return out


def cast_flags(kinds=("sphere", "plane"), opaque_only: bool = False) -> int:
    """The flag word of a ray query from the names of the kinds it tests ('sphere', 'plane', 'light'; or a ready CAST_* mask)."""
    if isinstance(kinds, (int, np.integer)):
        flags = int(kinds)
    else:
        flags = 0
        for k in kinds:
            flags |= CAST_KIND_NAMES[k]
    return flags | (CAST_OPAQUE if opaque_only else 0)


def make_rays(origins, dirs, tmax=np.inf, ignore=None) -> np.ndarray:
    """RAY_QUERY [n] from origins and dirs of [n, 3]; tmax and ignore (id words; None = ID_NONE) are scalar or per ray."""
    origins = np.asarray(origins, np.float32).reshape(-1, 3)
    rays = np.empty(origins.shape[0], RAY_QUERY)
    rays["origin"] = origins
    rays["dir"] = np.asarray(dirs, np.float32).reshape(-1, 3)
    rays["tmax"] = np.asarray(tmax, np.float32)
    rays["ignore"] = ID_NONE if ignore is None else np.asarray(ignore, np.uint32)
    return rays


def _cast_args(rays, spheres, planes, lights):
    rays = _flat(rays, RAY_QUERY)
    arrs = [None if a is None else np.ascontiguousarray(a) for a in (spheres, planes, lights)]
    counts = [0 if a is None else int(a.shape[0]) for a in arrs]
    return rays, arrs, counts


def cast_rays_host(rays, flags: int, spheres, planes, lights=None) -> np.ndarray:
    """clw_host_cast_rays: the nearest hit of every ray, on the host -- THE definition the device pass is held to -> HIT [n]."""
    rays, (s, p, l), (ns, np_, nl) = _cast_args(rays, spheres, planes, lights)
    out = np.empty(rays.size, HIT)
    if not _fits_u32(flags) or not load_library().clw_host_cast_rays(_ptr(rays), rays.size, int(flags), _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, _ptr(out)):
        raise ValueError("clw_host_cast_rays rejects these arguments (at least one ray, fewer than 2^30, a kind bit and only CAST_* bits in flags)")
    return out


def occluded_rays_host(rays, flags: int, spheres, planes, lights=None) -> np.ndarray:
    """clw_host_occluded_rays: whether every ray meets anything within its tmax, on the host -- THE definition -> uint8 [n] of 0 / 1."""
    rays, (s, p, l), (ns, np_, nl) = _cast_args(rays, spheres, planes, lights)
    out = np.empty(rays.size, np.uint8)
    if not _fits_u32(flags) or not load_library().clw_host_occluded_rays(_ptr(rays), rays.size, int(flags), _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, _ptr(out)):
        raise ValueError("clw_host_occluded_rays rejects these arguments (at least one ray, fewer than 2^30, a kind bit and only CAST_* bits in flags)")
    return out


def cast_layers_host(rays, flags: int, K: int, spheres, planes, lights=None) -> dict:
    """clw_host_cast_layers: the K nearest listed candidates of every ray, on the host -- THE definition the device pass is held to ->
    {"t": float32 [K, n], "id": uint32 [K, n]}, nearest first, empty entries {inf, ID_NONE}."""
    rays, (s, p, l), (ns, np_, nl) = _cast_args(rays, spheres, planes, lights)
    K = int(K)
    t, ids = np.empty((max(K, 0), rays.size), np.float32), np.empty((max(K, 0), rays.size), np.uint32)
    if not _fits_u32(flags, K) or not load_library().clw_host_cast_layers(
            _ptr(rays), rays.size, int(flags), K, _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, _ptr(t), _ptr(ids)):
        raise ValueError("clw_host_cast_layers rejects these arguments (at least one ray, fewer than 2^30, a kind bit and only CAST_* bits in flags, K in 1..8)")
    return {"t": t, "id": ids}


def path_flags(kinds=("sphere", "plane", "light"), opaque_only: bool = False, transmit: bool = False, all_surfaces: bool = False) -> int:
    """The flag word of a path query: cast_flags(kinds, opaque_only), PATH_TRANSMIT, PATH_ALL_SURFACES."""
    return cast_flags(kinds, opaque_only) | (PATH_TRANSMIT if transmit else 0) | (PATH_ALL_SURFACES if all_surfaces else 0)


def paths_result(hits, status, nxt) -> dict:
    """What a path query answers, from its three arrays (HIT [B, n], uint8 [n], RAY_QUERY [n]) -> {"t", "id", "normal", "point"} as [B, n]
    (normal and point [B, n, 3]; entries from a path's count on are misses), "count" and "reason" as uint8 [n] (PATH_REASON_*), "next" as
    RAY_QUERY [n], and the arrays themselves as "hits" and "status"."""
    return {"t": hits["t"], "id": hits["id"], "normal": hits["normal"], "point": hits["point"], "count": status & np.uint8(15),
            "reason": status >> np.uint8(4), "next": nxt, "hits": hits, "status": status}


def cast_paths_host(rays, flags: int, bounces: int, spheres, planes, lights=None) -> dict:
    """clw_host_cast_paths: the path of every ray -- its hit, the reference's reflected or refracted ray from there, that ray's hit ... for up
    to `bounces` segments --, on the host: THE definition the device pass is held to -> paths_result()."""
    rays, (s, p, l), (ns, np_, nl) = _cast_args(rays, spheres, planes, lights)
    B = int(bounces)
    hits, status, nxt = np.empty((max(B, 0), rays.size), HIT), np.empty(rays.size, np.uint8), np.empty(rays.size, RAY_QUERY)
    if not _fits_u32(flags, B) or not load_library().clw_host_cast_paths(
            _ptr(rays), rays.size, int(flags), B, _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, _ptr(hits), _ptr(status), _ptr(nxt)):
        raise ValueError("clw_host_cast_paths rejects these arguments (at least one ray, fewer than 2^30, a kind bit and only CAST_* and PATH_* bits in flags, bounces in 1..8)")
    return paths_result(hits, status, nxt)


def make_probes(points, reach=np.inf) -> np.ndarray:
    """PROBE [n] from points of [n, 3]; reach is scalar or per probe."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    probes = np.empty(points.shape[0], PROBE)
    probes["point"] = points
    probes["reach"] = np.asarray(reach, np.float32)
    return probes


def _near_args(probes, ignore, spheres, planes, lights):
    """The probes (PROBE [n]) and their ignore words (uint32 [n], a scalar for all, or None = nothing is ignored), flat, and the scene arrays."""
    probes = _flat(probes, PROBE)
    if ignore is not None:
        ignore = np.ascontiguousarray(np.broadcast_to(np.asarray(ignore, np.uint32).reshape(-1), probes.shape))
    arrs = [None if a is None else np.ascontiguousarray(a) for a in (spheres, planes, lights)]
    counts = [0 if a is None else int(a.shape[0]) for a in arrs]
    return probes, ignore, arrs, counts


_NEAR_REJECTS = "rejects these arguments (at least one probe, fewer than 2^30, a kind bit and only CAST_* bits in flags"


def nearest_surface_host(probes, flags: int, spheres, planes, lights=None, ignore=None) -> np.ndarray:
    """clw_host_nearest_surface: the nearest surface within reach of every probe, on the host -- THE definition the device pass is held to ->
    HIT [n] with t = the signed distance (negative inside a sphere)."""
    probes, ignore, (s, p, l), (ns, np_, nl) = _near_args(probes, ignore, spheres, planes, lights)
    out = np.empty(probes.size, HIT)
    if not _fits_u32(flags) or not load_library().clw_host_nearest_surface(
            _ptr(probes), _ptr(ignore), probes.size, int(flags), _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, _ptr(out)):
        raise ValueError("clw_host_nearest_surface " + _NEAR_REJECTS + ")")
    return out


def within_reach_host(probes, flags: int, spheres, planes, lights=None, ignore=None) -> np.ndarray:
    """clw_host_within_reach: whether any surface lies within reach of every probe, on the host -- THE definition -> uint8 [n] of 0 / 1."""
    probes, ignore, (s, p, l), (ns, np_, nl) = _near_args(probes, ignore, spheres, planes, lights)
    out = np.empty(probes.size, np.uint8)
    if not _fits_u32(flags) or not load_library().clw_host_within_reach(
            _ptr(probes), _ptr(ignore), probes.size, int(flags), _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, _ptr(out)):
        raise ValueError("clw_host_within_reach " + _NEAR_REJECTS + ")")
    return out


def near_surfaces_host(probes, flags: int, K: int, spheres, planes, lights=None, ignore=None) -> dict:
    """clw_host_near_surfaces: the K nearest surfaces within reach of every probe, on the host -- THE definition the device pass is held to ->
    {"d": float32 [K, n], "id": uint32 [K, n]}, nearest first, empty entries {inf, ID_NONE}."""
    probes, ignore, (s, p, l), (ns, np_, nl) = _near_args(probes, ignore, spheres, planes, lights)
    K = int(K)
    d, ids = np.empty((max(K, 0), probes.size), np.float32), np.empty((max(K, 0), probes.size), np.uint32)
    if not _fits_u32(flags, K) or not load_library().clw_host_near_surfaces(
            _ptr(probes), _ptr(ignore), probes.size, int(flags), _ptr(s), ns, _ptr(p), np_, _ptr(l), nl, K, _ptr(d), _ptr(ids)):
        raise ValueError("clw_host_near_surfaces " + _NEAR_REJECTS + ", K in 1..8)")
    return {"d": d, "id": ids}


def camera_rays_host(cam: clw_camera, proj: clw_projection | None = None, id_begin: int = 0, id_end: int | None = None) -> np.ndarray:
    """clw_host_camera_rays: the rays of the global ids [id_begin, id_end) of the camera's frame (id_end None = its last) under a camera model
    (None = the pinhole) as query rays -> RAY_QUERY [id_end - id_begin] with tmax = inf and ignore = ID_NONE."""
    proj = clw_projection() if proj is None else proj
    id_end = cam.width * cam.height if id_end is None else int(id_end)
    rays = np.zeros(max(id_end - int(id_begin), 0), RAY_QUERY)
    if not load_library().clw_host_camera_rays(C.byref(cam), C.byref(proj), int(id_begin), id_end, _ptr(rays)):
        raise ValueError("clw_host_camera_rays rejects these arguments (what clw_host_projection_rays rejects)")
    return rays


CULL_SPHERES, CULL_LIGHTS = 1, 2      # the bits of a primary-ray cull table's bytes (hip_wrap_ext.h: clw_host_primary_cull)
VARIANT_NO_CULL = 32768               # clw_ext_set_variant: no cull table


def host_primary_cull(cam: clw_camera, spheres, lights, rows: int | None = None, row_offset: int = 0, band_stride: int = 1, band_phase: int = 0) -> np.ndarray:
    """clw_host_primary_cull: THE definition of the primary-ray cull table of a launch over `rows` rows (default: the camera's height) of the
    camera's frame -> uint8 [tile rows, tiles per row], bit 0 = the tile's rays miss the line test of every sphere, bit 1 = of every light."""
    rows = int(cam.height) if rows is None else int(rows)
    s = None if spheres is None else np.ascontiguousarray(spheres)
    l = None if lights is None else np.ascontiguousarray(lights)
    ns, nl = (0 if a is None else int(a.shape[0]) for a in (s, l))
    trows, tpr = (rows + 7) // 8, (int(cam.width) + 7) // 8
    out = np.empty(max(trows * tpr, 1), np.uint8)
    n = load_library().clw_host_primary_cull(C.byref(cam), int(row_offset), rows, int(band_stride), int(band_phase), _ptr(s), ns, _ptr(l), nl, _ptr(out))
    if n != trows * tpr or n == 0:
        raise ValueError("clw_host_primary_cull rejects these arguments (a frame with tiles, band_phase below band_stride)")
    return out[:n].reshape(trows, tpr)


BC_SHADOW, BC_REFL_SPHERES, BC_REFL_LIGHTS = 15, 16, 32      # the bits of a bounce cull table's bytes (hip_wrap_ext.h: clw_host_bounce_cull)
BC_PART_SHADOW, BC_PART_REFL = 1, 2                          # its parts (clw_ext_set_bounce_cull)


def host_bounce_cull(cam: clw_camera, spheres, planes, lights, depth: int = 4, parts: int = 3, rows: int | None = None, row_offset: int = 0,
                     band_stride: int = 1, band_phase: int = 0) -> np.ndarray:
    """clw_host_bounce_cull: THE definition of the bounce cull table of a launch (the ranges of host_primary_cull) -> uint8 [tile rows, tiles per
    row], bits 0-3 = the first shade's shadow rays miss the line test of every sphere i with i % 4 = the bit, bit 4 / 5 = the second iteration's
    rays miss every sphere / every light."""
    rows = int(cam.height) if rows is None else int(rows)
    s, p, l = (None if a is None else np.ascontiguousarray(a) for a in (spheres, planes, lights))
    ns, npl, nl = (0 if a is None else int(a.shape[0]) for a in (s, p, l))
    trows, tpr = (rows + 7) // 8, (int(cam.width) + 7) // 8
    out = np.empty(max(trows * tpr, 1), np.uint8)
    n = load_library().clw_host_bounce_cull(C.byref(cam), int(row_offset), rows, int(band_stride), int(band_phase), _ptr(s), ns, _ptr(p), npl,
                                            _ptr(l), nl, int(depth), int(parts), _ptr(out))
    if n != trows * tpr or n == 0:
        raise ValueError("clw_host_bounce_cull rejects these arguments (a frame with tiles, band_phase below band_stride)")
    return out[:n].reshape(trows, tpr)


def _rect(rect):
    """None (the whole frame), a clw_rect or (x, y, width, height) -> what ctypes passes for a `const clw_rect*`"""
    if rect is None:
        return None
    if not isinstance(rect, clw_rect):
        rect = clw_rect(*(int(v) for v in rect))
    return C.byref(rect)


def _summary(s: clw_object_summary) -> dict:
    return dict(objects=int(s.objects), pixels=int(s.pixels), foreign=int(s.foreign))


def _object_table(call, first_capacity: int = 16384):
    """`call(out pointer, capacity, summary pointer)` -> (records, summary dict), or None when it is refused: once with room for
    `first_capacity` records (generous: a second device pass costs more than 768 KB of host memory), and once more with room for all of them
    when there are more"""
    s = clw_object_summary()
    out = np.zeros(first_capacity, OBJECT_STAT)
    if not call(_ptr(out), out.size, C.byref(s)):
        return None
    if s.objects > out.size:
        out = np.zeros(s.objects, OBJECT_STAT)
        if not call(_ptr(out), out.size, C.byref(s)):
            return None
    return out[:min(s.objects, out.size)].copy(), _summary(s)


def object_stats(ids, depth, width: int, rows: int, counts, first_row: int = 0, rect=None):
    """clw_host_object_stats: the visible-object table of a width x rows range of an id channel (and its depth channel, or None) whose first row
    is row `first_row` of the frame, on the host -- THE definition the device pass is held to -> (OBJECT_STAT [objects], {"objects", "pixels",
    "foreign"}).  counts = (spheres, planes, lights); rect = (x, y, width, height) in frame pixels, None = the whole frame."""
    got = _frame_channels(width, rows, (ids, np.uint32, 1))
    if got is None:
        raise ValueError("clw_host_object_stats rejects these arguments (an id channel of width * rows words)")
    width, rows, (ids,) = got
    got = _frame_channels(width, rows, optional=[(depth, np.float32, 1)])
    if got is None:
        raise ValueError("clw_host_object_stats rejects these arguments (a depth channel of width * rows words)")
    depth = got[2][0]
    counts = _flat(counts, np.uint32).reshape(3)
    L = load_library()
    got = _object_table(lambda out, cap, s: L.clw_host_object_stats(_ptr(ids), _ptr(depth), width, rows, int(first_row), _rect(rect), _ptr(counts),
                                                                    out, cap, s))
    if got is None:
        raise ValueError("clw_host_object_stats rejects these arguments (an empty rectangle, more than 2^24 - 1 primitives, 2^30 pixels or more)")
    return got


def merge_object_stats(a, b) -> np.ndarray:
    """clw_host_merge_object_stats: two tables sorted by id -> the table of both (the tables of two strips of a frame -> the frame's)."""
    a, b = _flat(a, OBJECT_STAT), _flat(b, OBJECT_STAT)
    out = np.zeros(a.size + b.size or 1, OBJECT_STAT)
    n = load_library().clw_host_merge_object_stats(_ptr(a), a.size, _ptr(b), b.size, _ptr(out), out.size)
    return out[:n].copy()


def projection(model, axis=None, ortho_width: float = 0.0, span=(360.0, 180.0)) -> clw_projection:
    """A clw_projection from a model (PROJ_* or 'perspective' / 'ortho' / 'equirect'), the view axis (None = the camera's own centre
    direction), the world width of an orthographic frame (0 = the camera's image plane as it stands) and the (horizontal, vertical) degrees of
    a panorama.  Nothing is checked here: the library refuses what hip_wrap_ext.h says it refuses."""
    p = clw_projection()
    p.model = PROJ_MODELS[model] if isinstance(model, str) else int(model)
    if axis is not None:
        p.axis[:] = [float(v) for v in axis]
    p.ortho_width, p.h_span, p.v_span = float(ortho_width), float(span[0]), float(span[1])
    return p


def projection_rays(cam: clw_camera, proj: clw_projection, id_begin: int = 0, id_end: int | None = None) -> np.ndarray:
    """clw_host_projection_rays: THE definition of the rays of a camera model -> float32 [id_end - id_begin, 16], the 64-byte records
    {origin, 0, direction, 0, 0 ...} of the global ids [id_begin, id_end) of the camera's frame (id_end None = its last)."""
    id_end = cam.width * cam.height if id_end is None else int(id_end)
    rays = np.zeros((max(id_end - int(id_begin), 0), 16), np.float32)
    if not load_library().clw_host_projection_rays(C.byref(cam), C.byref(proj), int(id_begin), id_end, _ptr(rays)):
        raise ValueError("clw_host_projection_rays rejects these arguments (model 0..2, a finite axis, ortho_width >= 0, spans in [0, 360] / "
                         "[0, 180], reserved 0, ids inside the frame)")
    return rays


def projection_tables(cam: clw_camera, proj: clw_projection):
    """clw_host_projection_tables: the two tables of a panorama -> (float32 [W, 4] {sin(theta) r + cos(theta) a, 0}, float32 [H, 4]
    {cos(phi), sin(phi) u}); ray (x, y) = normalize(col[x].xyz * row[y].x + row[y].yzw) in float32."""
    col, row = np.zeros((cam.width, 4), np.float32), np.zeros((cam.height, 4), np.float32)
    if not load_library().clw_host_projection_tables(C.byref(cam), C.byref(proj), _ptr(col), _ptr(row)):
        raise ValueError("clw_host_projection_tables rejects these arguments (an equirectangular projection the library accepts)")
    return col, row


def ortho_camera(origin, look, view_width: float, width: int, height: int):
    """clw_host_ortho_camera: an orthographic view from `origin` along `look` whose frame spans `view_width` world units -> (clw_camera,
    clw_projection): the image plane passes through the origin, pixels are square."""
    cam, proj = clw_camera(), clw_projection()
    if not load_library().clw_host_ortho_camera((C.c_float * 3)(*origin), (C.c_float * 3)(*look), float(view_width), int(width), int(height),
                                                C.byref(cam), C.byref(proj)):
        raise ValueError("clw_host_ortho_camera rejects these arguments (a finite look that is not vertical, view_width > 0, a frame)")
    return cam, proj


def frame_seed(f: int) -> int:
    """clw_host_frame_seed: the seed offset frame f of an accumulated view adds (0 for frame 0, distinct for every frame of a run)."""
    return int(load_library().clw_host_frame_seed(int(f) & 0xFFFFFFFF))


def jitter_camera(cam: clw_camera, f: int, n: int = 1) -> clw_camera:
    """clw_host_jitter_camera: the camera frame f of an accumulated view looks through -- `cam` moved by the frame's Halton (2, 3) point inside
    the cell of a sample of supersampling factor n (1, 2, 4, 8); frame 0 is `cam` itself."""
    out = clw_camera()
    if not load_library().clw_host_jitter_camera(C.byref(cam), int(f), int(n), C.byref(out)):
        raise ValueError("clw_host_jitter_camera rejects these arguments (n in 1, 2, 4, 8)")
    return out


def write_png(path: str, xrgb: np.ndarray, width: int, height: int) -> None:
    xrgb = np.ascontiguousarray(xrgb, np.uint32)
    assert xrgb.size == width * height
    rc = load_library().clw_host_write_png(path.encode(), _ptr(xrgb), width, height)
    if rc:
        raise OSError(f"png write failed ({rc}): {path}")


def write_png_rgba(path: str, rgba: np.ndarray) -> None:
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    rc = load_library().clw_host_write_png_rgba(path.encode(), _ptr(rgba), w, h)
    if rc:
        raise OSError(f"png write failed ({rc}): {path}")


def read_png(path: str) -> np.ndarray:
    """-> uint8 [h, w, 4] (A = 255); raises ValueError with the decoder's code otherwise."""
    L = load_library()
    w, h, p = C.c_uint32(), C.c_uint32(), C.c_void_p()
    rc = L.clw_host_read_png(path.encode(), C.byref(w), C.byref(h), C.byref(p))
    if rc:
        raise ValueError(f"png read failed ({rc}): {path}")
    try:
        buf = (C.c_uint8 * (w.value * h.value * 4)).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(h.value, w.value, 4).copy()
    finally:
        L.clw_host_free(p)


class ClWrap:
    """Object form of the six cl_wrap_* calls plus the extensions."""

    def __init__(self, *sources_and_names, device_type=CL_DEVICE_TYPE_GPU):
        self.L = load_library()
        self.w = cl_wrap()
        if not sources_and_names:
            sources_and_names = ("src/cl/raygen.cl", "raygen", "src/cl/raytracing.cl", "raytracer")
        args = [C.c_char_p(s.encode()) for s in sources_and_names] + [C.c_char_p(None)]
        self.L.cl_wrap_init(C.byref(self.w), C.c_uint64(device_type), *args)
        self._keep = []

    # ---- the reference API ----
    def load_global_data(self, kernel_id, arg_id, data, size=None, mem_flags=CL_MEM_READ_WRITE):
        if isinstance(data, np.ndarray):
            data = np.ascontiguousarray(data)
            size = data.nbytes if size is None else size
        self.L.cl_wrap_load_global_data(C.byref(self.w), kernel_id, arg_id, _ptr(data), size, mem_flags)

    def load_single_data(self, kernel_id, arg_id, obj):
        """obj: a ctypes object / bytes / numpy scalar or array (passed by value)."""
        if isinstance(obj, (bytes, bytearray)):
            buf = C.create_string_buffer(bytes(obj), len(obj))
            self.L.cl_wrap_load_single_data(C.byref(self.w), kernel_id, arg_id, C.cast(buf, C.c_void_p), len(obj))
        elif isinstance(obj, np.ndarray) or isinstance(obj, np.generic):
            a = np.ascontiguousarray(obj)
            self.L.cl_wrap_load_single_data(C.byref(self.w), kernel_id, arg_id, _ptr(a), a.nbytes)
        else:
            self.L.cl_wrap_load_single_data(C.byref(self.w), kernel_id, arg_id, C.cast(C.byref(obj), C.c_void_p),
                                            C.sizeof(obj))

    def load_images(self, kernel_id, arg_id, *paths, mem_flags=CL_MEM_COPY_HOST_PTR):
        args = [C.c_char_p(p.encode()) for p in paths]
        self.L.cl_wrap_load_images(C.byref(self.w), C.c_uint32(kernel_id), C.c_uint32(arg_id),
                                   C.c_uint64(mem_flags), C.c_uint32(len(paths)), *args)

    def output(self, array_size, output_size, kernel_run_id, kernel_id, arg_id, host_output=None):
        self.L.cl_wrap_output(C.byref(self.w), array_size, output_size, kernel_run_id, kernel_id, arg_id,
                              _ptr(host_output))

    def release(self):
        if self.w.impl:
            self.L.cl_wrap_release(C.byref(self.w))

    def buffer_handle(self, kernel_id, arg_id) -> C.c_void_p:
        """&wrap.buffers[k][a] as the drivers use it (raypng.c:61)."""
        return C.c_void_p(self.w.buffers[kernel_id][arg_id])

    # ---- extensions ----
    def set_depth(self, d): self.L.clw_ext_set_depth(C.byref(self.w), d)
    def get_depth(self): return self.L.clw_ext_get_depth(C.byref(self.w))
    def set_strict(self, s): self.L.clw_ext_set_strict(C.byref(self.w), int(s))
    def set_fuse(self, f): self.L.clw_ext_set_fuse(C.byref(self.w), int(f))
    def set_id_offset(self, first_id): self.L.clw_ext_set_id_offset(C.byref(self.w), first_id)
    def set_row_bands(self, stride, phase): self.L.clw_ext_set_row_bands(C.byref(self.w), stride, phase)
    def set_async(self, a): self.L.clw_ext_set_async(C.byref(self.w), int(a))
    def sync(self): self.L.clw_ext_sync(C.byref(self.w))
    def set_stream(self, s): self.L.clw_ext_set_stream(C.byref(self.w), C.c_void_p(s))
    def unit(self, op: int, rows: np.ndarray, out_cols: int, aux: int = 0) -> np.ndarray:
        """Run one device helper (see clw_ext_unit) over float32 rows -> float32 [n, out_cols]."""
        rows = np.ascontiguousarray(rows, np.float32)
        out = np.zeros((rows.shape[0], out_cols), np.float32)
        self.L.clw_ext_unit(C.byref(self.w), op, _ptr(rows), rows.shape[1], _ptr(out), out_cols, rows.shape[0], aux)
        return out

    def read_tile_costs(self) -> np.ndarray:
        return _read_counted(lambda p, cap: self.L.clw_ext_read_tile_costs(C.byref(self.w), p, cap), np.uint32)

    def read_tile_order(self):
        """(order words [8 * per_share_cap], per_share_cap) the last tiled launch read; (empty, 0) = it ran in the default order."""
        share = C.c_uint32()
        out = _read_counted(lambda p, cap: self.L.clw_ext_read_tile_order(C.byref(self.w), p, cap, C.byref(share)), np.uint32)
        return out, int(share.value)

    def unit_sched(self, cost: np.ndarray, tpr: int, trows: int, clamp_outliers: int, per_share_cap: int, split_slots: int, min_quota: int,
                   max_lg: int) -> np.ndarray:
        """Run wt_sched_build once on a cost table (see clw_ext_unit_sched) -> the whole sentinel-filled buffer, uint32."""
        cost = _flat(cost, np.uint32)
        assert cost.size == tpr * trows
        a = (int(tpr), int(trows), int(clamp_outliers), int(per_share_cap), int(split_slots), int(min_quota), int(max_lg))
        return _read_counted(lambda p, words: self.L.clw_ext_unit_sched(C.byref(self.w), _ptr(cost), *a, p, words), np.uint32)

    def get_split(self):
        """(split_slots, min_quota, extra entries per share of a launch that may split) in effect."""
        v = [C.c_uint32() for _ in range(3)]
        self.L.clw_ext_get_split(C.byref(self.w), *[C.byref(x) for x in v])
        return tuple(int(x.value) for x in v)

    def get_tpt(self):
        """(max_lanes, min_paths, pool_mb) of the tree-parallel tail in effect."""
        v = [C.c_uint32() for _ in range(3)]
        self.L.clw_ext_get_tpt(C.byref(self.w), *[C.byref(x) for x in v])
        return tuple(int(x.value) for x in v)

    def set_split(self, slots=-1, min_quota=-1): self.L.clw_ext_set_split(C.byref(self.w), int(slots), int(min_quota))
    def set_shadow_through(self, f): self.L.clw_ext_set_shadow_through(C.byref(self.w), float(f))
    def set_grid(self, on): self.L.clw_ext_set_grid(C.byref(self.w), int(on))

    def get_grid(self):
        """The grid of the scene as last prepared (see clw_ext_get_grid): dict(built, pair, res, ncells, pairs, cell, gmin, reg_pad), or
        None while no scene is prepared.  built 0 = the scene runs the linear scan (the other entries are then 0)."""
        g = clw_grid_info()
        if not self.L.clw_ext_get_grid(C.byref(self.w), C.byref(g)):
            return None
        return dict(built=int(g.built), pair=int(g.pair), res=tuple(int(x) for x in g.res), ncells=int(g.ncells), pairs=int(g.pairs),
                    cell=tuple(float(x) for x in g.cell), gmin=tuple(float(x) for x in g.gmin), reg_pad=float(g.reg_pad))

    def set_grid_pair(self, on=-1):
        """Shadow walk of grid scenes: -1 default (paired unless CLWRAP_GRID_PAIR=0), 0 single, 1 paired where the shim's rule allows it.
        Same image either way; the next launch prepares the scene again."""
        self.L.clw_ext_set_grid_pair(C.byref(self.w), int(on))
    def set_tile_sched(self, on): self.L.clw_ext_set_tile_sched(C.byref(self.w), int(on))
    def set_variant(self, v): self.L.clw_ext_set_variant(C.byref(self.w), int(v))
    def last_trace_flags(self): return int(self.L.clw_ext_last_trace_flags(C.byref(self.w)))

    def read_primary_cull(self):
        """clw_ext_read_primary_cull -> (the cull table the last whole-range trace launch was given as uint8 [tiles], or None when it had
        none; how often the builder has run)."""
        builds = C.c_uint64()
        out = _read_counted(lambda p, cap: self.L.clw_ext_read_primary_cull(C.byref(self.w), p, cap, C.byref(builds)), np.uint8)
        return (out if out.size else None), int(builds.value)

    def read_bounce_cull(self):
        """clw_ext_read_bounce_cull -> the bounce cull table the last whole-range trace launch was given as uint8 [tiles], or None"""
        out = _read_counted(lambda p, cap: self.L.clw_ext_read_bounce_cull(C.byref(self.w), p, cap), np.uint8)
        return out if out.size else None

    def set_bounce_cull(self, parts=3):
        """clw_ext_set_bounce_cull: which parts the tables built from now on carry (BC_PART_*; 0 = the primary bits only).  Same image."""
        self.L.clw_ext_set_bounce_cull(C.byref(self.w), int(parts))
    def set_tpt(self, max_lanes=-1, min_paths=-1, pool_mb=-1): self.L.clw_ext_set_tpt(C.byref(self.w), int(max_lanes), int(min_paths), int(pool_mb))
    def timing_reset(self): self.L.clw_ext_timing_reset(C.byref(self.w))
    def set_timing_every(self, n): self.L.clw_ext_set_timing_every(C.byref(self.w), int(n))
    def set_pipeline(self, on): self.L.clw_ext_set_pipeline(C.byref(self.w), int(on))

    def timing_get(self, kernel_id):
        n, ms = C.c_uint32(), C.c_double()
        self.L.clw_ext_timing_get(C.byref(self.w), kernel_id, C.byref(n), C.byref(ms))
        return n.value, ms.value

    def load_images_raw(self, kernel_id, arg_id, rgba: np.ndarray):
        rgba = np.ascontiguousarray(rgba, np.uint8)
        layers, h, w, c = rgba.shape
        assert c == 4
        self.L.clw_ext_load_images_raw(C.byref(self.w), kernel_id, arg_id, _ptr(rgba), w, h, layers)

    def bind_device_buffer(self, kernel_id, arg_id, device_ptr, size):
        self.L.clw_ext_bind_device_buffer(C.byref(self.w), kernel_id, arg_id, C.c_void_p(device_ptr), size)

    def device_ptr(self, kernel_id, arg_id): return self.L.clw_ext_device_ptr(C.byref(self.w), kernel_id, arg_id)
    def set_debug_rgb(self, ptr): self.L.clw_ext_set_debug_rgb(C.byref(self.w), C.c_void_p(ptr))
    def set_supersample(self, n): self.L.clw_ext_set_supersample(C.byref(self.w), int(n))
    def get_supersample(self): return int(self.L.clw_ext_get_supersample(C.byref(self.w)))

    def set_seed_offset(self, s): self.L.clw_ext_set_seed_offset(C.byref(self.w), int(s) & 0xFFFFFFFF)
    def get_seed_offset(self): return int(self.L.clw_ext_get_seed_offset(C.byref(self.w)))
    def set_accumulate(self, max_frames, jitter=True): self.L.clw_ext_set_accumulate(C.byref(self.w), int(max_frames), int(jitter))
    def get_accumulated(self): return int(self.L.clw_ext_get_accumulated(C.byref(self.w)))
    def reset_accumulation(self): self.L.clw_ext_reset_accumulation(C.byref(self.w))

    def render_gbuffer(self, channels=GB_ALL) -> int:
        """Launch the primary-hit pass over the range the next trace launch would cover -> work-items (0 = no camera latched / no known channel)."""
        return int(self.L.clw_ext_render_gbuffer(C.byref(self.w), int(channels)))

    def _read_pass(self, read, dtype) -> np.ndarray:
        """What a range pass left on the device: the counted read-back whose `read(out, capacity_bytes)` counts in bytes."""
        return _read_counted(read, dtype, unit=1)

    def read_gbuffer(self, channel) -> np.ndarray:
        """One channel (a GB_* bit) of the last pass -> float32 [n] / uint32 [n] / float32 [n, 3]; empty for a channel it did not write."""
        _, dtype, per = next(v for v in GB_CHANNELS.values() if v[0] == channel)
        out = self._read_pass(lambda p, cap: self.L.clw_ext_read_gbuffer(C.byref(self.w), int(channel), p, cap), dtype)
        return out.reshape(-1, 3) if per == 3 else out

    def gbuffer_device_ptr(self, channel):
        """Device address of one channel of the last pass (None for a channel it did not write)."""
        return self.L.clw_ext_gbuffer_device_ptr(C.byref(self.w), int(channel))

    def pick(self, x, y):
        """clw_ext_pick: the clw_pick of frame pixel (x, y), or None (no camera latched, or the pixel is not one of this wrapper's)."""
        p = clw_pick()
        return p if self.L.clw_ext_pick(C.byref(self.w), int(x), int(y), C.byref(p)) else None

    def render_overlay(self, style: clw_overlay, sel) -> int:
        """clw_ext_render_overlay: compose the selection overlay of the wrapper's range on the device -> work-items (0 = refused, nothing launched)."""
        sel = _selection(sel)
        return int(self.L.clw_ext_render_overlay(C.byref(self.w), C.byref(style), _ptr(sel) if sel.size else None, sel.size))

    def read_overlay(self) -> np.ndarray:
        """The overlay frame of the last render_overlay -> uint32 [n]; empty before the first."""
        return self._read_pass(lambda p, cap: self.L.clw_ext_read_overlay(C.byref(self.w), p, cap), np.uint32)

    def overlay_device_ptr(self):
        """Device address of the overlay frame of the last render_overlay (None before the first)."""
        return self.L.clw_ext_overlay_device_ptr(C.byref(self.w))

    def unit_overlay(self, frame, ids, width: int, rows: int, style: clw_overlay, sel):
        """clw_ext_unit_overlay: the device pass on a synthetic frame and id channel -> uint32 [width * rows], or None when it is refused."""
        frame, ids = _flat(frame, np.uint32), _flat(ids, np.uint32)
        assert frame.size == int(width) * int(rows) == ids.size
        sel = _selection(sel)
        out = np.empty(frame.size, np.uint32)
        n = self.L.clw_ext_unit_overlay(C.byref(self.w), _ptr(frame), _ptr(ids), int(width), int(rows), C.byref(style),
                                        _ptr(sel) if sel.size else None, sel.size, _ptr(out))
        return out if n == frame.size and n else None

    def object_stats(self, rect=None):
        """clw_ext_object_stats: the visible-object table of the wrapper's range, reduced on the device -> (OBJECT_STAT [objects], {"objects",
        "pixels", "foreign"}), or None when it is refused (nothing launched).  rect = (x, y, width, height) in frame pixels, None = the whole frame."""
        return _object_table(lambda out, cap, s: self.L.clw_ext_object_stats(C.byref(self.w), _rect(rect), out, cap, s))

    def unit_object_stats(self, ids, depth, width: int, rows: int, counts, first_row: int = 0, rect=None):
        """clw_ext_unit_object_stats: the device pass on a synthetic id channel (and depth channel, or None) -> (records, summary), or None when
        it is refused."""
        ids = _flat(ids, np.uint32)
        assert ids.size == int(width) * int(rows)
        if depth is not None:
            depth = _flat(depth, np.float32)
            assert depth.size == ids.size
        counts = _flat(counts, np.uint32).reshape(3)
        return _object_table(lambda out, cap, s: self.L.clw_ext_unit_object_stats(C.byref(self.w), _ptr(ids), _ptr(depth), int(width), int(rows), int(first_row),
                                                                                  _rect(rect), _ptr(counts), out, cap, s),
                             first_capacity=max(1024, min(ids.size, int(counts.astype(np.uint64).sum()) + 1)))

    def render_ao(self, ao: clw_ao) -> int:
        """clw_ext_render_ao: trace and resolve the ambient occlusion of the wrapper's range on the device -> work-items (0 = refused, nothing launched)."""
        return int(self.L.clw_ext_render_ao(C.byref(self.w), C.byref(ao)))

    def read_ao(self, what: int = AO_FRAME) -> np.ndarray:
        """What the last render_ao left: AO_FRAME -> uint32 [n], AO_COUNTS -> uint8 [n]; empty before the first."""
        return self._read_pass(lambda p, cap: self.L.clw_ext_read_ao(C.byref(self.w), int(what), p, cap), np.uint8 if what == AO_COUNTS else np.uint32)

    def ao_device_ptr(self, what: int = AO_FRAME):
        """Device address of the frame or the counts of the last render_ao (None before the first)."""
        return self.L.clw_ext_ao_device_ptr(C.byref(self.w), int(what))

    def cast_rays(self, rays, flags: int = CAST_SPHERES | CAST_PLANES):
        """clw_ext_cast_rays: the nearest hit of every ray (RAY_QUERY [n]) against the bound scene, on the device -> HIT [n], or None when it is
        refused (no scene bound, no ray, unknown flag bits, no kind)."""
        rays = _flat(rays, RAY_QUERY)
        out = np.empty(rays.size, HIT)
        if not _fits_u32(rays.size, flags):
            return None
        n = self.L.clw_ext_cast_rays(C.byref(self.w), _ptr(rays), rays.size, int(flags), _ptr(out))
        return out if n == rays.size and n else None

    def occluded_rays(self, rays, flags: int = CAST_SPHERES | CAST_PLANES):
        """clw_ext_occluded_rays: whether every ray meets anything within its tmax, on the device -> uint8 [n] of 0 / 1, or None when it is refused."""
        rays = _flat(rays, RAY_QUERY)
        out = np.empty(rays.size, np.uint8)
        if not _fits_u32(rays.size, flags):
            return None
        n = self.L.clw_ext_occluded_rays(C.byref(self.w), _ptr(rays), rays.size, int(flags), _ptr(out))
        return out if n == rays.size and n else None

    def cast_rays_device(self, rays_ptr: int, n: int, flags: int = CAST_SPHERES | CAST_PLANES, hits_ptr: int | None = None, blocked_ptr: int | None = None) -> int:
        """clw_ext_cast_rays_device: the query over the caller's device memory (integer addresses: n RAY_QUERY records; n HIT records or n bytes --
        exactly one of the two), on the wrapper's stream, without waiting -> n, or 0 when it is refused."""
        if not _fits_u32(n, flags):
            return 0
        return int(self.L.clw_ext_cast_rays_device(C.byref(self.w), C.c_void_p(rays_ptr or None), int(n), int(flags), C.c_void_p(hits_ptr or None),
                                                   C.c_void_p(blocked_ptr or None)))

    def cast_layers(self, rays, flags: int = CAST_SPHERES | CAST_PLANES, K: int = 4):
        """clw_ext_cast_layers: the K nearest listed candidates of every ray (RAY_QUERY [n]) against the bound scene, on the device ->
        {"t": float32 [K, n], "id": uint32 [K, n]}, or None when it is refused (no scene bound, no ray, unknown flag bits, no kind, K outside 1..8)."""
        rays = _flat(rays, RAY_QUERY)
        if not _fits_u32(rays.size, flags, K):
            return None
        t, ids = np.empty((int(K), rays.size), np.float32), np.empty((int(K), rays.size), np.uint32)
        n = self.L.clw_ext_cast_layers(C.byref(self.w), _ptr(rays), rays.size, int(flags), int(K), _ptr(t), _ptr(ids))
        return {"t": t, "id": ids} if n == rays.size and n else None

    def cast_layers_device(self, rays_ptr: int, n: int, flags: int, K: int, t_ptr: int, id_ptr: int) -> int:
        """clw_ext_cast_layers_device: the layered query over the caller's device memory (integer addresses: n RAY_QUERY records; K * n floats;
        K * n words, layer-major), on the wrapper's stream, without waiting -> n, or 0 when it is refused."""
        if not _fits_u32(n, flags, K):
            return 0
        return int(self.L.clw_ext_cast_layers_device(C.byref(self.w), C.c_void_p(rays_ptr or None), int(n), int(flags), int(K), C.c_void_p(t_ptr or None),
                                                     C.c_void_p(id_ptr or None)))

    def _probes(self, probes, ignore):
        probes = _flat(probes, PROBE)
        if ignore is not None:
            ignore = np.ascontiguousarray(np.broadcast_to(np.asarray(ignore, np.uint32).reshape(-1), probes.shape))
        return probes, ignore

    def nearest_surface(self, probes, flags: int = CAST_SPHERES | CAST_PLANES, ignore=None):
        """clw_ext_nearest_surface: the nearest surface within reach of every probe (PROBE [n]; ignore: uint32 [n], a scalar, or None) against
        the bound scene, on the device -> HIT [n] with t = the signed distance, or None when it is refused (no scene bound, no probe, unknown
        flag bits, no kind)."""
        probes, ignore = self._probes(probes, ignore)
        out = np.empty(probes.size, HIT)
        if not _fits_u32(probes.size, flags):
            return None
        n = self.L.clw_ext_nearest_surface(C.byref(self.w), _ptr(probes), _ptr(ignore), probes.size, int(flags), _ptr(out))
        return out if n == probes.size and n else None

    def within_reach(self, probes, flags: int = CAST_SPHERES | CAST_PLANES, ignore=None):
        """clw_ext_within_reach: whether any surface lies within reach of every probe, on the device -> uint8 [n] of 0 / 1, or None when it is
        refused."""
        probes, ignore = self._probes(probes, ignore)
        out = np.empty(probes.size, np.uint8)
        if not _fits_u32(probes.size, flags):
            return None
        n = self.L.clw_ext_within_reach(C.byref(self.w), _ptr(probes), _ptr(ignore), probes.size, int(flags), _ptr(out))
        return out if n == probes.size and n else None

    def near_surfaces(self, probes, flags: int = CAST_SPHERES | CAST_PLANES, K: int = 4, ignore=None):
        """clw_ext_near_surfaces: the K nearest surfaces within reach of every probe, on the device -> {"d": float32 [K, n], "id": uint32
        [K, n]}, or None when it is refused (as nearest_surface; K outside 1..8)."""
        probes, ignore = self._probes(probes, ignore)
        if not _fits_u32(probes.size, flags, K):
            return None
        d, ids = np.empty((int(K), probes.size), np.float32), np.empty((int(K), probes.size), np.uint32)
        n = self.L.clw_ext_near_surfaces(C.byref(self.w), _ptr(probes), _ptr(ignore), probes.size, int(flags), int(K), _ptr(d), _ptr(ids))
        return {"d": d, "id": ids} if n == probes.size and n else None

    def probe_device(self, probes_ptr: int, n: int, flags: int = CAST_SPHERES | CAST_PLANES, ignore_ptr: int | None = None, hits_ptr: int | None = None,
                     within_ptr: int | None = None) -> int:
        """clw_ext_probe_device: the nearest or the within query over the caller's device memory (integer addresses: n PROBE records; n ignore
        words or None; n HIT records or n bytes -- exactly one of the two), on the wrapper's stream, without waiting -> n, or 0 when it is refused."""
        if not _fits_u32(n, flags):
            return 0
        return int(self.L.clw_ext_probe_device(C.byref(self.w), C.c_void_p(probes_ptr or None), C.c_void_p(ignore_ptr or None), int(n), int(flags),
                                               C.c_void_p(hits_ptr or None), C.c_void_p(within_ptr or None)))

    def near_surfaces_device(self, probes_ptr: int, n: int, flags: int, K: int, d_ptr: int, id_ptr: int, ignore_ptr: int | None = None) -> int:
        """clw_ext_near_surfaces_device: the K-nearest query over the caller's device memory (integer addresses: n PROBE records; K * n floats;
        K * n words, layer-major; n ignore words or None), on the wrapper's stream, without waiting -> n, or 0 when it is refused."""
        if not _fits_u32(n, flags, K):
            return 0
        return int(self.L.clw_ext_near_surfaces_device(C.byref(self.w), C.c_void_p(probes_ptr or None), C.c_void_p(ignore_ptr or None), int(n), int(flags),
                                                       int(K), C.c_void_p(d_ptr or None), C.c_void_p(id_ptr or None)))

    def camera_rays(self, capacity: int):
        """clw_ext_camera_rays: the query rays of the range the next trace launch would cover -> RAY_QUERY [n], or None when it is refused (no
        camera latched, row bands, a projection that does not resolve, fewer than n records of capacity)."""
        out = np.zeros(max(int(capacity), 1), RAY_QUERY)
        n = self.L.clw_ext_camera_rays(C.byref(self.w), _ptr(out), int(capacity))
        return out[:n].copy() if n else None

    def camera_rays_device(self, rays_ptr: int, capacity: int) -> int:
        """clw_ext_camera_rays_device: the same into the caller's device memory of `capacity` records, without waiting -> n, or 0."""
        return int(self.L.clw_ext_camera_rays_device(C.byref(self.w), C.c_void_p(rays_ptr or None), int(capacity)))

    def render_layers(self, flags: int = CAST_SPHERES | CAST_PLANES, K: int = 4) -> int:
        """clw_ext_render_layers: the K layers of the launch camera's rays over the wrapper's range, on the device -> work-items (0 = refused)."""
        if not _fits_u32(flags, K):
            return 0
        return int(self.L.clw_ext_render_layers(C.byref(self.w), int(flags), int(K)))

    def read_layers(self, what: int = LAYERS_T) -> np.ndarray:
        """What the last render_layers left: LAYERS_T -> float32 [K * n], LAYERS_ID -> uint32 [K * n], layer-major; empty before the first."""
        return self._read_pass(lambda p, cap: self.L.clw_ext_read_layers(C.byref(self.w), int(what), p, cap), np.uint32 if what == LAYERS_ID else np.float32)

    def layers_device_ptr(self, what: int = LAYERS_T):
        """Device address of the t or the id layers of the last render_layers (None before the first)."""
        return self.L.clw_ext_layers_device_ptr(C.byref(self.w), int(what))

    def pick_layers(self, x, y, flags: int = CAST_SPHERES | CAST_PLANES, K: int = 8):
        """clw_ext_pick_layers: the K layers under frame pixel (x, y) -> LAYER [K], or None (no camera latched, the pixel is not one of this
        wrapper's, refused flags or K)."""
        if not _fits_u32(flags) or not 1 <= int(K) <= LAYERS_MAX:
            return None
        out = np.zeros(int(K), LAYER)
        return out if self.L.clw_ext_pick_layers(C.byref(self.w), int(x), int(y), int(flags), int(K), _ptr(out)) else None

    def cast_paths(self, rays, flags: int = CAST_KINDS, bounces: int = 4):
        """clw_ext_cast_paths: the path of every ray (RAY_QUERY [n]) through the bound scene, on the device, in one launch -> paths_result(), or
        None when it is refused (no scene bound, no ray, unknown flag bits, no kind, bounces outside 1..8)."""
        rays = _flat(rays, RAY_QUERY)
        if not _fits_u32(rays.size, flags, bounces) or int(bounces) < 1:
            return None
        hits, status, nxt = np.empty((int(bounces), rays.size), HIT), np.empty(rays.size, np.uint8), np.empty(rays.size, RAY_QUERY)
        n = self.L.clw_ext_cast_paths(C.byref(self.w), _ptr(rays), rays.size, int(flags), int(bounces), _ptr(hits), _ptr(status), _ptr(nxt))
        return paths_result(hits, status, nxt) if n == rays.size and n else None

    def cast_paths_device(self, rays_ptr: int, n: int, flags: int, bounces: int, hits_ptr: int, status_ptr: int, next_ptr: int | None = None) -> int:
        """clw_ext_cast_paths_device: the path query over the caller's device memory (integer addresses: n RAY_QUERY records; bounces * n HIT
        records, segment-major; n bytes; n RAY_QUERY records or None), on the wrapper's stream, without waiting -> n, or 0 when it is refused."""
        if not _fits_u32(n, flags, bounces):
            return 0
        return int(self.L.clw_ext_cast_paths_device(C.byref(self.w), C.c_void_p(rays_ptr or None), int(n), int(flags), int(bounces),
                                                    C.c_void_p(hits_ptr or None), C.c_void_p(status_ptr or None), C.c_void_p(next_ptr or None)))

    def pick_path(self, x, y, bounces: int = 4, flags: int = CAST_KINDS):
        """clw_ext_pick_path: the path of the camera ray of frame pixel (x, y) -> (HIT [bounces], status byte), or None (no camera latched, the
        pixel is not one of this wrapper's, refused flags or bounces, no scene bound)."""
        if not _fits_u32(flags) or not 1 <= int(bounces) <= PATH_MAX_BOUNCES:
            return None
        hits, status = np.zeros(int(bounces), HIT), np.zeros(1, np.uint8)
        ok = self.L.clw_ext_pick_path(C.byref(self.w), int(x), int(y), int(bounces), int(flags), _ptr(hits), _ptr(status))
        return (hits, int(status[0])) if ok else None

    def unit_ao_open(self, point, normal, ids, width: int, rows: int, first_row: int, ao: clw_ao):
        """clw_ext_unit_ao_open: wt_ao_trace on synthetic channels against the bound scene -> uint8 [width * rows], or None when it is refused."""
        point, normal, ids = _flat(point, np.float32), _flat(normal, np.float32), _flat(ids, np.uint32)
        assert ids.size == int(width) * int(rows) and point.size == normal.size == 3 * ids.size
        out = np.empty(ids.size, np.uint8)
        n = self.L.clw_ext_unit_ao_open(C.byref(self.w), _ptr(point), _ptr(normal), _ptr(ids), int(width), int(rows), int(first_row), C.byref(ao), _ptr(out))
        return out if n == ids.size and n else None

    def unit_ao_resolve(self, open_u8, ids, frame, width: int, rows: int, ao: clw_ao):
        """clw_ext_unit_ao_resolve: wt_ao_resolve on synthetic counts, ids and frame (or None) -> uint32 [width * rows], or None when it is refused."""
        open_u8, ids = _flat(open_u8, np.uint8), _flat(ids, np.uint32)
        if frame is not None:
            frame = _flat(frame, np.uint32)
        assert open_u8.size == int(width) * int(rows) == ids.size
        out = np.empty(ids.size, np.uint32)
        n = self.L.clw_ext_unit_ao_resolve(C.byref(self.w), _ptr(open_u8), _ptr(ids), _ptr(frame), int(width), int(rows), C.byref(ao), _ptr(out))
        return out if n == ids.size and n else None

    def set_projection(self, proj: clw_projection | None):
        """clw_ext_set_projection: the camera model of the following launches and inspection passes; None = the pinhole."""
        self.L.clw_ext_set_projection(C.byref(self.w), None if proj is None else C.byref(proj))

    def get_projection(self) -> clw_projection:
        p = clw_projection()
        self.L.clw_ext_get_projection(C.byref(self.w), C.byref(p))
        return p

    def unit_projection(self, cam: clw_camera, proj: clw_projection, id_begin: int = 0, id_end: int | None = None):
        """clw_ext_unit_projection: wt_raygen_proj on a synthetic camera -> float32 [id_end - id_begin, 16], or None when it is refused."""
        id_end = cam.width * cam.height if id_end is None else int(id_end)
        rays = np.zeros((max(id_end - int(id_begin), 0), 16), np.float32)
        ok = self.L.clw_ext_unit_projection(C.byref(self.w), C.byref(cam), C.byref(proj), int(id_begin), id_end, _ptr(rays))
        return rays if ok else None

    def set_adaptive(self, threshold): self.L.clw_ext_set_adaptive(C.byref(self.w), int(threshold))
    def get_adaptive(self): return int(self.L.clw_ext_get_adaptive(C.byref(self.w)))

    def read_refine_mask(self) -> np.ndarray:
        """The block mask of the last trace launch if it was adaptive -> uint8 [blocks], row-major (empty = it was not)."""
        return _read_counted(lambda p, cap: self.L.clw_ext_read_refine_mask(C.byref(self.w), p, cap), np.uint8)

    def set_sample_cameras(self, cams):
        """float32 [n*n, 12] ({im_corner, origin, up, right} per sample, sy * n + sx order), copied; None / empty = no table."""
        if cams is None or len(cams) == 0:
            self.L.clw_ext_set_sample_cameras(C.byref(self.w), None, 0)
            return
        cams = np.ascontiguousarray(cams, np.float32)
        assert cams.ndim == 2 and cams.shape[1] == 12
        self.L.clw_ext_set_sample_cameras(C.byref(self.w), _ptr(cams), cams.shape[0])

    def get_sample_cameras(self) -> np.ndarray:
        """The table the last trace launch used -> float32 [count, 12] (count 0 = none)."""
        cams = _read_counted(lambda p, cap: self.L.clw_ext_get_sample_cameras(C.byref(self.w), p, cap), np.float32, unit=C.sizeof(clw_sample_camera))
        return cams.reshape(-1, 12)

    def set_lens(self, aperture, focus): self.L.clw_ext_set_lens(C.byref(self.w), float(aperture), float(focus))

    def set_sphere_motion(self, disp, times=None):
        """disp float32 [spheres, 3] (the movement of each centre while the shutter is open), times float32 [n*n] or None (the shutter
        times); both copied.  disp None / empty = no table."""
        if disp is None or len(disp) == 0:
            self.L.clw_ext_set_sphere_motion(C.byref(self.w), None, 0, None, 0)
            return
        disp = np.ascontiguousarray(disp, np.float32).reshape(-1, 3)
        times = None if times is None else _flat(times, np.float32)
        self.L.clw_ext_set_sphere_motion(C.byref(self.w), _ptr(disp), disp.shape[0], None if times is None else _ptr(times), 0 if times is None else times.size)

    def get_sample_times(self) -> np.ndarray:
        """The sample times the last trace launch used -> float32 [count] (count 0 = the scene stood still)."""
        return _read_counted(lambda p, cap: self.L.clw_ext_get_sample_times(C.byref(self.w), p, cap), np.float32)

    def enable_counters(self, on): self.L.clw_ext_enable_counters(C.byref(self.w), int(on))

    def read_counters(self):
        """Work counters of the counting build (clw_ext_read_counters_ex); `shadow_rays` counts every shadow ray the
        reference would cast, `shadow_rays_traced` leaves out the ones elided on zero-coefficient surfaces."""
        out = (C.c_uint64 * 32)()
        self.L.clw_ext_read_counters_ex(C.byref(self.w), C.byref(out), 32)
        self.last_raw_counters = [int(x) for x in out]
        names = ["segments", "shadow_rays", "light_probes", "sky_fetches", "texel_fetches", "pushes",
                 "lane_iters", "wave_iters_x64", "shadow_rays_traced", "lights_classified"]
        d = dict(zip(names, [int(x) for x in out]))
        d["vis_mismatches"] = int(out[28])
        d["tpt_gave_up"], d["tpt_tiles"], d["tpt_nodes"] = int(out[29]), int(out[30]), int(out[31])   # tree-parallel tail (deep launches)
        d["tpt_batches"], d["tpt_max_batches"], d["tpt_max_nodes"], d["tpt_longest_us"] = int(out[16]), int(out[17]), int(out[18]), round(int(out[19]) * 0.01, 1)
        d["tpt_phase_max_us"] = [round(int(out[20 + k]) * 0.01, 1) for k in range(6)]
        d["tpt_phase_us"] = [round(int(out[10 + k]) * 0.01, 1) for k in range(6)]   # roots, expansion, order, RNG, shading, replay (summed over tiles)
        return d

    def invalidate_scene(self): self.L.clw_ext_invalidate_scene(C.byref(self.w))

    def unit_scene(self, op: int, rows: np.ndarray, out_cols: int, kernel_id: int = 1) -> np.ndarray:
        """Run one scene-dependent device helper (see clw_ext_unit_scene) over float32 rows -> float32 [n, out_cols]."""
        rows = np.ascontiguousarray(rows, np.float32)
        out = np.zeros((rows.shape[0], out_cols), np.float32)
        self.L.clw_ext_unit_scene(C.byref(self.w), kernel_id, op, _ptr(rows), rows.shape[1], _ptr(out), out_cols, rows.shape[0])
        return out
