"""The primary-hit pass on the GPU (include/hip_wrap_ext.h: clw_ext_render_gbuffer, clw_ext_pick; csrc/whitted_gbuffer.inc) against the buffers
tests/gbuffer_common.py builds from the oracle's own functions.
strict build: the ids, and the bits of depth, normal, point and albedo, equal the expected on every pixel.
fast build: ids differ on at most 2e-3 of a case's pixels (grazing rays; the share the function tests allow); where they agree depth and point
within rtol 1e-4 / atol 1e-4 and the normal within 1e-5; albedo within 1e-6 on at least 99 % of the pixels (a hit point within 1e-7 of a texel
edge may take the neighbour: the bar of test_find_solid_intersection).

Measured on the MI355X: both builds meet every bound.  strict: 0 ids and 0 bits differ in all cases, depth included.  fast: 0 or 1 id per case
differs, and on the pixels with equal ids depth, point and normal have the expected BITS (largest error 0): the pass decides the winner in the
build's own arithmetic but evaluates the winner's depth, point, normal and a light's colour in the reference's (csrc/whitted_gbuffer.inc,
csrc/ref_tests.h). Evaluated in the fast build's own fused arithmetic the same quantities miss these bounds -- D/4 = b*b - c cancels near a
silhouette and from afar: normals off by up to 7.9e-5 (case A, 21 pixels above 1e-5) and 2.4e-3 (D0, 83 pixels), a light colour of 16.01 off by
an ulp of 1.9e-6 on 2 % of case C1 -- which is why they are not."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_common as gc
from render_common import bits, released, rendering

pytestmark = pytest.mark.gpu

CHANNELS = ("depth", "id", "normal", "point", "albedo")


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


_got = {}


def render_case(name, strict, tex, sky, grid=True, **kw):
    """`with render_case(...) as r:` -- a renderer of the case's scene that looks through the case's camera"""
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    key, w, h, cam, _ = gc.CASES[name]
    return rendering(Renderer, gc.case_scene(name), tex, sky, w, h, setup=None if grid else (lambda wrap: wrap.set_grid(0)), cam=cam, depth=4,
                     strict=strict, **kw)


def gbuffer_of(name, strict, tex, sky):
    """The full-frame buffers of a case in one build, rendered once per module."""
    if (name, strict) not in _got:
        with render_case(name, strict, tex, sky) as r:
            _got[name, strict] = r.gbuffer()
    return _got[name, strict]


def assert_same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def check_against_oracle(g, e, strict, name):
    n = len(e["id"])
    assert g["id"].dtype == np.uint32 and g["id"].shape == (n,) and g["depth"].shape == (n,)
    for k in ("normal", "point", "albedo"):
        assert g[k].shape == (n, 3) and g[k].dtype == np.float32
    differ = g["id"] != e["id"]
    print(f"case {name} {'strict' if strict else 'fast'}: {int(differ.sum())} of {n} ids differ")
    if strict:
        assert not differ.any()
        for k in ("depth", "normal", "point", "albedo"):
            bad = (bits(g[k]) != bits(e[k])).reshape(n, -1).any(1)
            print(f"  {k}: {int(bad.sum())} pixels differ in bits")
            assert not bad.any(), k
        return
    assert differ.mean() <= 2e-3
    same = ~differ
    hit = same & np.isfinite(e["depth"])
    derr = np.abs(g["depth"][hit].astype(np.float64) - e["depth"][hit])
    print(f"  depth: largest error {derr.max():.3g}")
    assert np.allclose(g["depth"][same], e["depth"][same], rtol=1e-4, atol=1e-4)
    alb = np.abs(g["albedo"] - e["albedo"]).max(1) < 1e-6
    lights = ~alb & same & (gc.kind_of(e["id"]) == gc.KIND_LIGHT)
    rel = (np.abs(g["albedo"] - e["albedo"])[lights] / np.maximum(np.abs(e["albedo"][lights]), 1e-30))[e["albedo"][lights] != 0]
    print(f"  albedo within 1e-6 on {alb.mean():.4f} of the pixels; of the {int((~alb).sum())} others {int(lights.sum())} see a light with the expected id "
          f"(largest relative error of its colour {rel.max() if rel.size else 0.0:.3g}, largest value {e['albedo'][lights].max() if lights.any() else 0.0:.4g})")
    assert alb.mean() >= 0.99


def check_fast_geometry(g, e, name):
    """The fast build's point and normal on the pixels whose id is the expected one (the bounds of the module docstring)."""
    same = g["id"] == e["id"]
    perr = np.abs(g["point"][same].astype(np.float64) - e["point"][same])
    pbad = (perr > 1e-4 + 1e-4 * np.abs(e["point"][same])).any(1)
    nerr = np.abs(g["normal"][same] - e["normal"][same]).max(1)
    k = gc.kind_of(e["id"][same])
    print(f"case {name} fast: of the pixels above the normal bound {int(((nerr > 1e-5) & (k == gc.KIND_SPHERE)).sum())} are sphere pixels")
    print(f"case {name} fast: point largest error {perr.max():.3g}, {int(pbad.sum())} of {int(same.sum())} pixels outside rtol 1e-4 / atol 1e-4; "
          f"normal largest error {nerr.max():.3g}, {int((nerr > 1e-5).sum())} pixels above 1e-5")
    assert np.allclose(g["point"][same], e["point"][same], rtol=1e-4, atol=1e-4)
    assert nerr.max() <= 1e-5


@pytest.mark.parametrize("name", list(gc.CASES))
def test_buffers_equal_the_oracle(oracle, tex, sky, strict, name):
    check_against_oracle(gbuffer_of(name, strict, tex, sky), gc.expected_case(oracle, name, tex, sky), strict, name)


@pytest.mark.parametrize("name", list(gc.CASES) + ["D0-nogrid", "D1-nogrid"])
def test_fast_build_point_and_normal(oracle, tex, sky, name):
    import torch  # noqa: F401
    case = name.split("-")[0]
    if case == name:
        g = gbuffer_of(case, False, tex, sky)
    else:
        with render_case(case, False, tex, sky, grid=False) as r:
            g = r.gbuffer()
    check_fast_geometry(g, gc.expected_case(oracle, case, tex, sky), name)


@pytest.mark.parametrize("name", ["D0", "D1"])
def test_linear_scan_of_a_big_scene_equals_the_oracle(oracle, tex, sky, strict, name):
    """324 spheres with the uniform grid switched off: the scene read from global memory, every sphere tested."""
    with render_case(name, strict, tex, sky, grid=False) as r:
        g = r.gbuffer()
    check_against_oracle(g, gc.expected_case(oracle, name, tex, sky), strict, name + " (no grid)")
    if strict:
        assert_same_bits(g, gbuffer_of(name, strict, tex, sky))


def test_channel_mask(tex, sky, strict):
    from example_gui_opencl_raytracer_amd import api
    full = gbuffer_of("A", strict, tex, sky)
    with render_case("A", strict, tex, sky) as r:
        g = r.gbuffer(api.GB_DEPTH | api.GB_ID)
        assert set(g) == {"depth", "id"}
        assert_same_bits(g, {k: full[k] for k in g})
        assert r.w.read_gbuffer(api.GB_NORMAL).size == 0
        assert r.w.L.clw_ext_read_gbuffer(C.byref(r.w.w), api.GB_NORMAL, None, 0) == 0
        assert not r.w.gbuffer_device_ptr(api.GB_NORMAL)
        assert r.w.gbuffer_device_ptr(api.GB_DEPTH) and r.w.gbuffer_device_ptr(api.GB_ID)
        assert r.w.L.clw_ext_read_gbuffer(C.byref(r.w.w), api.GB_DEPTH, None, 0) == 4 * r.pixels
        assert r.w.read_gbuffer(api.GB_ID).shape == (r.pixels,)
        assert r.w.L.clw_ext_read_gbuffer(C.byref(r.w.w), api.GB_DEPTH | api.GB_ID, None, 0) == 0      # one bit at a time
        assert r.w.render_gbuffer(0) == 0 and r.w.render_gbuffer(1 << 7) == 0          # no known bit: no pass, the last one stands
        assert r.w.read_gbuffer(api.GB_DEPTH).shape == (r.pixels,)
        # a later pass with more channels allocates the missing ones
        assert_same_bits(r.gbuffer(), full)


def test_strips_compose(tex, sky, strict):
    """Three strips of the 37-row frame (16, 16 and 5 rows: the last is not tile-aligned) are the full frame's rows, bit for bit."""
    from example_gui_opencl_raytracer_amd.renderer import strip_rows
    full = gbuffer_of("A", strict, tex, sky)
    parts, rows = [], 0
    for rank in range(3):
        r0, n = strip_rows(gc.H, 3, rank)
        assert r0 == rows and n > 0
        rows += n
        with render_case("A", strict, tex, sky, first_row=r0, rows=n) as r:
            parts.append(r.gbuffer())
    assert rows == gc.H and strip_rows(gc.H, 3, 2)[1] % 8 != 0
    assert_same_bits({k: np.concatenate([p[k] for p in parts]) for k in CHANNELS}, full)


def test_row_bands_compose(tex, sky, strict):
    """Two renderers that own every second 8-row band of a 70x32 frame."""
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    w, h = gc.W, 32
    cam = gc.CASES["A"][3]
    def one(**kw):
        with rendering(Renderer, gc.case_scene("A"), tex, sky, w, h, cam=cam, depth=4, strict=strict, **kw) as r:
            return r.gbuffer()
    full = one()
    built = {k: np.zeros_like(full[k]) for k in CHANNELS}
    for phase in range(2):
        g = one(bands=(2, phase))
        local = np.arange(h // 2)
        rows = ((local // 8) * 2 + phase) * 8 + local % 8
        for k in CHANNELS:
            per = full[k].shape[1:]
            built[k].reshape((h, w) + per)[rows] = g[k].reshape((h // 2, w) + per)
    assert_same_bits(built, full)


def pick_equals(p, g, i):
    assert p is not None
    assert p["id"] == int(g["id"][i]) and p["kind"] == p["id"] >> 30 and p["index"] == p["id"] & 0x3FFFFFFF
    assert bits(p["depth"]).item() == bits(g["depth"][i]).item()
    for k in ("point", "normal", "albedo"):
        assert np.array_equal(bits(p[k]), bits(g[k][i])), k


def test_pick_is_the_buffers_entry(oracle, tex, sky, strict):
    from example_gui_opencl_raytracer_amd import api
    W, H = gc.W, gc.H
    full = gbuffer_of("A", strict, tex, sky)
    e = gc.expected_case(oracle, "A", tex, sky)
    kind, miss = gc.kind_of(e["id"]), e["id"] == gc.ID_NONE
    sphere_px = int(np.flatnonzero(~miss & (kind == gc.KIND_SPHERE))[0])
    light_px = int(np.flatnonzero(~miss & (kind == gc.KIND_LIGHT))[0])
    pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (66, 10), (20, 34), (sphere_px % W, sphere_px // W), (light_px % W, light_px // W)]
    with render_case("A", strict, tex, sky) as r:
        for x, y in pixels:
            pick_equals(r.pick(x, y), full, y * W + x)
        if strict:
            assert r.pick(sphere_px % W, sphere_px // W)["kind"] == gc.KIND_SPHERE and r.pick(light_px % W, light_px // W)["kind"] == gc.KIND_LIGHT
        assert r.pick(W, 0) is None and r.pick(0, H) is None                  # outside the frame
        # a pick leaves the last pass's buffers alone
        g = r.gbuffer()
        r.pick(3, 3)
        assert_same_bits({k: r.w.read_gbuffer(bit) for k, (bit, _, _) in api.GB_CHANNELS.items()}, g)
    # a sky pixel of case B
    eb = gc.expected_case(oracle, "B", tex, sky)
    sky_px = int(np.flatnonzero(eb["id"] == gc.ID_NONE)[0])
    fb = gbuffer_of("B", strict, tex, sky)
    with render_case("B", strict, tex, sky) as r:
        p = r.pick(sky_px % W, sky_px // W)
        pick_equals(p, fb, sky_px)
        if strict:
            assert p["id"] == gc.ID_NONE and np.isposinf(p["depth"]) and not p["point"].any() and not p["albedo"].any()


def test_pick_in_a_strip_and_in_a_band(tex, sky, strict):
    from example_gui_opencl_raytracer_amd.renderer import Renderer, strip_rows
    W, H = gc.W, gc.H
    full = gbuffer_of("A", strict, tex, sky)
    r0, n = strip_rows(H, 3, 1)                                           # rows 16..31
    with render_case("A", strict, tex, sky, first_row=r0, rows=n) as r:
        assert r.pick(5, r0 - 1) is None and r.pick(5, r0 + n) is None and r.pick(5, 0) is None
        pick_equals(r.pick(5, r0), full, r0 * W + 5)
        pick_equals(r.pick(W - 1, r0 + n - 1), full, (r0 + n - 1) * W + W - 1)
    cam = gc.CASES["A"][3]
    with Renderer(gc.case_scene("A"), tex, sky, W, 32, depth=4, strict=strict) as a, \
         Renderer(gc.case_scene("A"), tex, sky, W, 32, depth=4, strict=strict, bands=(2, 1)) as b:
        a.look(**cam); b.look(**cam)
        ga = a.gbuffer()
        assert b.pick(7, 3) is None and b.pick(7, 16) is None                 # bands 0 and 2 belong to phase 0
        for y in (8, 15, 24, 31):
            pick_equals(b.pick(7, y), ga, y * W + 7)


def test_nothing_latched_returns_zero_and_the_process_lives_on(tex, sky, strict):
    from example_gui_opencl_raytracer_amd import api
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    with released(api.ClWrap()) as w:
        w.set_strict(strict)
        assert w.pick(0, 0) is None and w.render_gbuffer(api.GB_ALL) == 0
        assert w.read_gbuffer(api.GB_DEPTH).size == 0 and not w.gbuffer_device_ptr(api.GB_DEPTH)
    with Renderer(gc.case_scene("A"), tex, sky, gc.W, gc.H, depth=4, strict=strict) as r:      # a scene, but no raygen launch yet
        assert r.pick(1, 1) is None and r.w.render_gbuffer(api.GB_ALL) == 0
        with pytest.raises(RuntimeError):
            r.gbuffer()
        r.look(**gc.CASES["A"][3])
        assert_same_bits(r.gbuffer(), gbuffer_of("A", strict, tex, sky))


def test_sampling_modes_do_not_change_the_buffers(tex, sky, strict):
    full = gbuffer_of("A", strict, tex, sky)
    disp = np.array([[0.5, 0.0, 0.0], [0.0, 0.3, 0.0], [0.0, 0.0, -0.4], [0.2, 0.2, 0.2]], np.float32)
    for kw in (dict(supersample=4, lens=(0.1, 8.0)), dict(supersample=2, motion=disp)):
        with render_case("A", strict, tex, sky, **kw) as r:
            assert_same_bits(r.gbuffer(), full)
            r.render()                                                        # ... and with the mode's tables on the device
            assert_same_bits(r.gbuffer(), full)
            pick_equals(r.pick(40, 20), full, 20 * gc.W + 40)


def test_an_accumulating_view_keeps_counting(tex, sky, strict):
    full = gbuffer_of("A", strict, tex, sky)
    with render_case("A", strict, tex, sky, accumulate=8) as plain:
        for _ in range(7):
            plain.render()
        want = plain.render_rgb()
        assert plain.accumulated == 8
    with render_case("A", strict, tex, sky, accumulate=8) as r:
        for f in range(7):
            r.render()
            assert r.accumulated == f + 1
            assert_same_bits(r.gbuffer(), full)
            pick_equals(r.pick(33, 12), full, 12 * gc.W + 33)
            assert r.accumulated == f + 1
        got = r.render_rgb()
        assert r.accumulated == 8
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def test_the_frame_is_unchanged(tex, sky, strict):
    with render_case("A", strict, tex, sky) as r:
        before = r.render()
        r.gbuffer()
        r.pick(10, 10)
        after = r.render()
        assert np.array_equal(before, after)
