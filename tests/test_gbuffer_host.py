"""The primary-hit pass without a GPU: its C ABI against the header and the ctypes mirror, and the expected buffers the GPU tests compare
with (tests/gbuffer_common.py) against the oracle they are built from."""
import ctypes as C
import re

import numpy as np
import pytest

import gbuffer_common as gc
from render_common import header_text

NEW_SYMBOLS = ["clw_ext_render_gbuffer", "clw_ext_read_gbuffer", "clw_ext_gbuffer_device_ptr", "clw_ext_pick"]


def test_header_library_and_mirror_agree_on_the_new_symbols():
    from example_gui_opencl_raytracer_amd import api
    code = header_text(comments=False)
    L = api.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"hip_wrap_ext.h does not declare {name}"
        assert name in api.SYMBOLS
        assert hasattr(L, name), f"the library does not export {name}"
        assert getattr(L, name).argtypes is not None
    assert L.clw_ext_render_gbuffer.restype is C.c_uint32 and L.clw_ext_read_gbuffer.restype is C.c_uint32
    assert L.clw_ext_gbuffer_device_ptr.restype is C.c_void_p and L.clw_ext_pick.restype is C.c_int


def test_constants_match_the_header():
    from example_gui_opencl_raytracer_amd import api
    defs = dict(re.findall(r"#define\s+(CLW_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", header_text()))
    want = dict(CLW_GB_DEPTH=api.GB_DEPTH, CLW_GB_ID=api.GB_ID, CLW_GB_NORMAL=api.GB_NORMAL, CLW_GB_POINT=api.GB_POINT, CLW_GB_ALBEDO=api.GB_ALBEDO,
                CLW_GB_ALL=api.GB_ALL, CLW_ID_NONE=api.ID_NONE, CLW_TIMING_GBUFFER=api.TIMING_GBUFFER)
    for name, value in want.items():
        assert int(defs[name], 0) == value, name
    assert (api.GB_DEPTH, api.GB_ID, api.GB_NORMAL, api.GB_POINT, api.GB_ALBEDO) == (1, 2, 4, 8, 16) and api.GB_ALL == 31
    assert api.ID_NONE == gc.ID_NONE == 0xFFFFFFFF
    assert [v[0] for v in api.GB_CHANNELS.values()] == [1, 2, 4, 8, 16] and list(api.GB_CHANNELS) == ["depth", "id", "normal", "point", "albedo"]


def test_pick_structure_mirrors_the_header():
    from example_gui_opencl_raytracer_amd import api
    assert C.sizeof(api.clw_pick) == 44
    m = re.search(r"typedef struct clw_pick \{(.*?)\} clw_pick;", header_text(), flags=re.S)
    assert m, "hip_wrap_ext.h does not define clw_pick"
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for decl in m.group(1).split(";") if decl.strip()
              for f in re.sub(r"^\s*(uint32_t|float)\s+", "", decl.strip()).split(",")]
    assert fields == ["id", "depth", "point", "normal", "albedo"]
    assert [f[0] for f in api.clw_pick._fields_] == fields
    assert [(getattr(api.clw_pick, f).offset, getattr(api.clw_pick, f).size) for f in fields] == [(0, 4), (4, 4), (8, 12), (20, 12), (32, 12)]


def test_renderer_has_the_two_calls():
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    from example_gui_opencl_raytracer_amd import api
    assert callable(Renderer.gbuffer) and callable(Renderer.pick)
    for name in ("render_gbuffer", "read_gbuffer", "gbuffer_device_ptr", "pick"):
        assert callable(getattr(api.ClWrap, name))


def test_id_helpers_round_trip():
    from example_gui_opencl_raytracer_amd import api
    kinds = np.array([0, 1, 2, 0, 1, 2], np.uint32)
    index = np.array([0, 0, 0, 323, 1, (1 << 30) - 1], np.uint32)
    ids = api.make_id(kinds, index)
    assert ids.dtype == np.uint32
    assert np.array_equal(api.id_kind(ids), kinds) and np.array_equal(api.id_index(ids), index)
    assert int(api.make_id(1, 5)) == (1 << 30 | 5) == gc.make_id(gc.KIND_PLANE, 5)
    assert int(api.id_kind(api.ID_NONE)) == 3                      # no kind: a miss is told by the whole word
    assert (api.ID_SPHERE, api.ID_PLANE, api.ID_LIGHT) == (gc.KIND_SPHERE, gc.KIND_PLANE, gc.KIND_LIGHT)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_expected_buffers_are_consistent_with_the_oracle(oracle, tex, sky, name):
    """The winner the construction finds by itself agrees with wo_find_solid on hit / miss everywhere, a sphere winner's normal recomputed from
    its depth is the oracle's, and the case holds the pixel kinds it is there for."""
    key, w, h, cam, holds = gc.CASES[name]
    e = gc.expected_case(oracle, name, tex, sky)
    sc = gc.case_scene(name)
    n = w * h
    assert all(len(e[k]) == n for k in e)
    ids, kind = e["id"], gc.kind_of(e["id"])
    light = (ids != gc.ID_NONE) & (kind == gc.KIND_LIGHT)
    miss = ids == gc.ID_NONE
    solid = ~light & ~miss
    # the search's own winner / no winner equals wo_find_solid's flag wherever no light ends the search
    assert np.array_equal(e["solid"][~light], solid[~light])
    assert np.isinf(e["depth"][miss]).all() and (e["depth"][~miss] > 0).all() and np.isfinite(e["depth"][~miss]).all()
    for k in ("normal", "point"):
        assert not e[k][miss | light].any()
    assert not e["albedo"][miss].any()
    # a sphere winner: normal = normalize(o + d t - centre)
    rays = oracle.raygen(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], w, h)).astype(np.float64)
    sph = solid & (kind == gc.KIND_SPHERE)
    if sph.any():
        centre = sc.spheres["origin"][ids[sph] & 0x3FFFFFFF].astype(np.float64)
        v = rays[sph, 0:3] + rays[sph, 4:7] * e["depth"][sph, None].astype(np.float64) - centre
        v /= np.linalg.norm(v, axis=1)[:, None]
        assert np.abs(v - e["normal"][sph]).max() < 1e-5
    pl = solid & (kind == gc.KIND_PLANE)
    if pl.any():
        assert np.array_equal(e["normal"][pl], sc.planes["normal"][ids[pl] & 0x3FFFFFFF])
    # indices stay inside the caller's arrays
    for k, count in ((gc.KIND_SPHERE, len(sc.spheres)), (gc.KIND_PLANE, len(sc.planes)), (gc.KIND_LIGHT, len(sc.lights))):
        sel = ~miss & (kind == k)
        assert ((ids[sel] & 0x3FFFFFFF) < count).all()
    for what, least in holds.items():
        have = int(miss.sum()) if what == "miss" else (len(np.unique(ids)) if what == "distinct" else int((~miss & (kind == what)).sum()))
        assert have >= least, (name, what, have)
    if name.startswith("C"):      # the light in view is the one the camera was put in front of, in its own colour
        k = int(name[1])
        assert set(np.unique(ids[light]) & 0x3FFFFFFF) == {k}
        on = sc.lights[k]["rgb"] > 0
        assert (e["albedo"][light][:, on] > 0).all() and not e["albedo"][light][:, ~on].any()
