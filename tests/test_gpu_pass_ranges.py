"""The range passes -- G-buffer, selection overlay, visible-object table, ambient occlusion -- share one description of their range, one owner
of their range-sized buffers and one read-back (csrc/hip_wrap_passes.cpp: pass_range, range_resize, range_mark_done, range_read).  One wrapper whose
range changes under them, twice, must answer like a fresh wrapper given each range directly; the ray queries, which share the geometry
binder with them, must still answer like their definition afterwards."""
import numpy as np
import pytest

import cast_common as cc
from render_common import R, api, bits, rendering  # noqa: F401  (R, api: the fixtures)

W, H, DEPTH = 64, 48, 2
RANGES = [(0, H), (16, 16), (0, H)]      # (first row, rows): the frame, the strip of rows 16..31, the frame again
FLOATS = ("gb_depth", "gb_normal", "gb_point", "gb_albedo")


def move_range(r, first_row, rows):
    """the renderer's range without a new wrapper: the id offset and `pixels`, set as the Renderer of a strip sets them when it is made"""
    r.first_row, r.rows, r.pixels = first_row, rows, rows * r.width
    r.w.set_id_offset(first_row * r.width)
    r.w.load_single_data(1, 7, np.uint32(r.pixels))


def all_passes(r, api):
    """a frame, then the four passes over it, everything read back"""
    out = {"frame": r.render().copy()}
    out.update(("gb_" + k, v) for k, v in r.gbuffer(api.GB_ALL).items())
    out["overlay"] = r.highlight([api.make_id(api.ID_SPHERE, 0), api.make_id(api.ID_PLANE, 0)], radius=3, fill=0x00FF00, edges=0xFF0000)
    out["objects"] = r.objects()
    out["ao"] = r.ambient_occlusion(8, 2.0, compose=True)
    out["ao_counts"] = r.ao_counts()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
def test_passes_follow_a_range_that_changes_under_one_wrapper(R, api, demo_scene, tex, sky, strict):
    want = {}
    for first_row, rows in set(RANGES):
        with rendering(R, demo_scene, tex, sky, W, H, depth=DEPTH, strict=strict, first_row=first_row, rows=rows) as fresh:
            want[first_row, rows] = all_passes(fresh, api)
    with rendering(R, demo_scene, tex, sky, W, H, depth=DEPTH, strict=strict) as r:
        for step, (first_row, rows) in enumerate(RANGES):
            move_range(r, first_row, rows)
            got, fresh = all_passes(r, api), want[first_row, rows]
            assert got.keys() == fresh.keys() and len(got) == 10
            for name in got:
                a, b = got[name], fresh[name]
                assert a.shape == b.shape and a.dtype == b.dtype and a.size, (step, name)
                if name in FLOATS:
                    assert np.array_equal(bits(a), bits(b)), (step, name)
                elif name == "objects":
                    assert a.tobytes() == b.tobytes(), (step, name)      # records of integer and float fields: the same bytes
                else:
                    assert np.array_equal(a, b), (step, name)
            assert got["gb_id"].size == rows * W and got["ao"].shape == (rows, W)
        # the queries after the passes: 65 rays = one full batch of 64 and one ray more
        rays = cc.make_rays(demo_scene, 65, 5)[0]
        assert rays.size == 65
        hits = r.w.cast_rays(rays, cc.KINDS)
        assert hits.tobytes() == api.cast_rays_host(rays, cc.KINDS, demo_scene.spheres, demo_scene.planes, demo_scene.lights).tobytes()
