"""The selection overlay on the GPU (include/hip_wrap_ext.h: clw_ext_render_overlay, clw_ext_unit_overlay; csrc/whitted_overlay.inc) against the
numpy restatement of its rules in tests/overlay_common.py -- bit for bit, in both builds: the pass is integer work.
The unit test feeds the kernel synthetic frames and id fields; the scene tests compose the overlay of rendered frames and hold it to the model of
`render()`'s frame and `gbuffer(GB_ID)`'s ids, and hold that nothing else of the wrapper moved.

Measured on the MI355X: 0 pixels differ from the model in every case of both builds (2 x 2352 unit cases, every scene test); the two strips of
the 61 x 43 frame (seam at row 32) differ from the full frame in 9 pixels, all within 3 rows of the seam, as the header says they may."""
import numpy as np
import pytest

import gbuffer_common as gc
import overlay_common as oc
from conftest import CAM
from render_common import R, api, bits, released, rendering  # noqa: F401  (R, api: the fixtures)

pytestmark = pytest.mark.gpu

OUTLINE, FILL, EDGE = oc.OUTLINE_RGB, oc.FILL_RGB, oc.EDGE_RGB


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


def model_of(frame, ids, width, rows, flags, radius, alpha, sel):
    return oc.model(frame, ids, width, rows, flags, radius, OUTLINE, FILL, alpha, EDGE, sel)


def highlighted(r, sel, flags=7, radius=2, alpha=96):
    """`highlight` with the colours of overlay_common and the flags as a word"""
    return r.highlight(sel, outline=OUTLINE if flags & oc.OV_OUTLINE else None, radius=radius, fill=FILL if flags & oc.OV_FILL else None, alpha=alpha,
                       edges=EDGE if flags & oc.OV_EDGES else None)


def read_framebuffer(r):
    """the framebuffer as it lies, without tracing: the read-back rides on the raygen launch, which in fused mode only latches the camera"""
    out = np.empty(r.pixels, np.uint32)
    r.w.output(r.pixels, out.nbytes, 0, 1, 10, out)
    return out


# ------------------------------------------------------------------ 1. the kernel on synthetic fields
_expected, _unit = {}, {}


def expected_unit(size):
    """[(case, frame, ids, expected, census) ...] of one size: computed once, shared by both builds, never written to"""
    if size not in _expected:
        frame = oc.frame_of(*size)
        frame.setflags(write=False)
        fields, rows = {}, []
        for case in oc.unit_cases([size]):
            w, h, radius, flags, name, sel, alpha = case
            ids = fields.setdefault((name, len(sel)), oc.field(name, w, h, sel))
            want, census = model_of(frame, ids, w, h, flags, radius, alpha, sel)
            want.setflags(write=False)
            rows.append((case, frame, ids, want, census))
        _expected[size] = rows
    return _expected[size]


def run_unit(api, strict, size):
    """every case of one size through clw_ext_unit_overlay -> the census of the cases that equalled the model (all of them, or the test fails)"""
    if (strict, size) not in _unit:
        total, bad = {}, []
        with released(api.ClWrap()) as w:
            w.set_strict(strict)
            for (width, rows, radius, flags, name, sel, alpha), frame, ids, want, census in expected_unit(size):
                got = w.unit_overlay(frame, ids, width, rows, api.overlay_style(flags, radius, OUTLINE, FILL, alpha, EDGE), sel)
                assert got is not None and got.shape == want.shape
                if not np.array_equal(got, want):
                    bad.append((width, rows, radius, flags, name, len(sel), alpha, int((got != want).sum())))
                oc.add_census(total, census)
        print(f"{size[0]} x {size[1]} {'strict' if strict else 'fast'}: {len(expected_unit(size))} cases, {len(bad)} differ from the model {bad[:8]}")
        assert not bad
        _unit[strict, size] = total
    return _unit[strict, size]


@pytest.mark.parametrize("size", oc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unit_overlay_equals_the_model(api, strict, size):
    run_unit(api, strict, size)


def test_unit_run_asks_every_rule_both_ways(api, strict):
    total = {}
    for size in oc.SIZES:
        oc.add_census(total, run_unit(api, strict, size))
    oc.assert_every_rule_fired_and_was_skipped(total)


def test_unit_overlay_refusals(api, strict):
    frame, ids = oc.frame_of(5, 3), oc.field("checker", 5, 3, oc.selection(1))
    S = lambda flags, radius=2, alpha=96: api.overlay_style(flags, radius, OUTLINE, FILL, alpha, EDGE)
    with released(api.ClWrap()) as w:
        w.set_strict(strict)
        for style, sel in ((S(0), [7]), (S(8), [7]), (S(1, 0), [7]), (S(1, 5), [7]), (S(2, 2, 257), [7]), (S(7), np.arange(65))):
            assert w.unit_overlay(frame, ids, 5, 3, style, sel) is None
        assert w.read_overlay().size == 0 and not w.overlay_device_ptr() and w.render_overlay(S(7), [7]) == 0      # no kernels, nothing latched
        got = w.unit_overlay(frame, ids, 5, 3, S(7), None)                                                        # no ids: legal
        assert np.array_equal(got, model_of(frame, ids, 5, 3, 7, 2, 96, np.zeros(0, np.uint32))[0])


# ------------------------------------------------------------------ 2. a rendered scene
def sphere_pixel(ids, width):
    """a pixel in the middle of the run of sphere pixels -> (x, y)"""
    on = np.flatnonzero(gc.kind_of(ids) == gc.KIND_SPHERE)
    assert on.size
    px = int(on[on.size // 2])
    return px % width, px // width


@pytest.mark.parametrize("W,H", [(61, 43), (160, 120)])
def test_scene_highlight_equals_the_model(R, api, demo_scene, tex, sky, strict, W, H):
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:
        frame = r.render()
        g = r.gbuffer(api.GB_ID | api.GB_DEPTH)
        ids, depth = g["id"], g["depth"]
        x, y = sphere_pixel(ids, W)
        sel = r.pick(x, y)["id"]
        assert sel == ids[y * W + x] and sel >> 30 == gc.KIND_SPHERE
        got = highlighted(r, sel)
        want, census = model_of(frame, ids, W, H, 7, 2, 96, [sel])
        print(f"{W} x {H} {'strict' if strict else 'fast'}: {int((got != want).sum())} pixels differ; {census}")
        assert got.dtype == np.uint32 and got.shape == (W * H,) and np.array_equal(got, want)
        assert census["fill_drawn"] > 0 and census["outline_drawn"] > 0 and census["edge_drawn"] > 0
        # nothing else moved: the traced frame, the channels of the earlier pass, the overlay's own read-back and device buffer
        assert np.array_equal(read_framebuffer(r), frame)
        assert np.array_equal(bits(r.w.read_gbuffer(api.GB_DEPTH)), bits(depth)) and np.array_equal(r.w.read_gbuffer(api.GB_ID), ids)
        assert np.array_equal(r.w.read_overlay(), got) and r.w.overlay_device_ptr()
        assert r.w.overlay_device_ptr() != r.w.device_ptr(1, 10) and r.w.overlay_device_ptr() != r.w.gbuffer_device_ptr(api.GB_ID)
        # every radius and OUTLINE alone, on the same frame
        for radius in oc.RADII:
            assert np.array_equal(highlighted(r, sel, oc.OV_OUTLINE, radius), model_of(frame, ids, W, H, oc.OV_OUTLINE, radius, 0, [sel])[0]), radius
        # a pixel is filled iff the object under it is the selected one
        paint = 0x010203
        assert not (frame == paint).any()
        filled = r.highlight(sel, outline=None, fill=paint, alpha=256)
        rng = np.random.default_rng(5)
        sample = [(x, y)] + [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(24)]
        hits = 0
        for sx, sy in sample:
            is_selected = r.pick(sx, sy)["id"] == sel
            hits += is_selected
            assert (filled[sy * W + sx] == paint) == is_selected, (sx, sy)
        assert 0 < hits < len(sample)
        assert np.array_equal(r.render(), frame)


# ------------------------------------------------------------------ 3. what can be selected
@pytest.mark.parametrize("kind", ["plane", "light", "sky"])
def test_selections_by_kind(R, api, tex, sky, strict, kind):
    name = "B" if kind == "sky" else "A"
    _, W, H, cam, _ = gc.CASES[name]
    with rendering(R, gc.case_scene(name), tex, sky, W, H, cam=cam, depth=4, strict=strict) as r:
        frame = r.render()
        ids = r.gbuffer(api.GB_ID)["id"]
        kinds = gc.kind_of(ids)
        if kind == "sky":
            sel = api.ID_NONE
        else:
            sel = int(ids[np.flatnonzero((kinds == (gc.KIND_PLANE if kind == "plane" else gc.KIND_LIGHT)) & (ids != api.ID_NONE))[0]])
        assert (ids == sel).any() and (ids != sel).any()
        want, census = model_of(frame, ids, W, H, 7, 3, 128, [sel])
        got = highlighted(r, sel, 7, 3, 128)
        print(f"{kind} {'strict' if strict else 'fast'}: id {sel:#x}, {int((got != want).sum())} pixels differ; {census}")
        assert np.array_equal(got, want)
        assert census["fill_drawn"] > 0 and census["outline_drawn"] > 0


# ------------------------------------------------------------------ 4. a scene on the uniform grid, 64 ids
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "linear"])
def test_grid_scene_with_64_ids(R, api, tex, sky, strict, grid):
    _, W, H, cam, _ = gc.CASES["D1"]
    with rendering(R, gc.case_scene("D1"), tex, sky, W, H, cam=cam, depth=4, strict=strict, setup=None if grid else (lambda w: w.set_grid(0))) as r:
        frame = r.render()
        assert bool(r.w.last_trace_flags() & 16) == grid          # WT_F_GRID: the trace launch walked the uniform grid, or scanned all 324 spheres
        ids = r.gbuffer(api.GB_ID)["id"]
        seen = np.unique(ids[gc.kind_of(ids) == gc.KIND_SPHERE])
        assert seen.size > 128
        sel = seen[::2][:64]                        # every second sphere in sight: 64 ids, with unselected spheres between them
        assert sel.size == 64
        want, census = model_of(frame, ids, W, H, 7, 1, 200, sel)
        got = highlighted(r, sel, 7, 1, 200)
        print(f"grid {grid} {'strict' if strict else 'fast'}: {int((got != want).sum())} pixels differ; {census}")
        assert np.array_equal(got, want)
        assert census["fill_drawn"] > 0 and census["outline_drawn"] > 0 and census["fill_unselected"] > 0


# ------------------------------------------------------------------ 5. row strips
def test_strips_are_composed_on_their_own_rows(R, api, demo_scene, tex, sky, strict):
    W, H, radius = 61, 43, 3
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:
        frame = r.render()
        ids = r.gbuffer(api.GB_ID)["id"]
        # the seam between the two strips: the first row (a multiple of 8 if there is one) that a sphere crosses; that sphere is selected
        grid = ids.reshape(H, W)
        spheres_across = lambda s: [int(i) for i in np.intersect1d(grid[s - 1], grid[s]) if i >> 30 == gc.KIND_SPHERE]
        seams = [s for s in list(range(8, H - radius, 8)) + list(range(radius + 1, H - radius)) if spheres_across(s)]
        assert seams
        seam = seams[0]
        sel = spheres_across(seam)[0]
        assert r.pick(int(np.flatnonzero(grid[seam] == sel)[0]), seam)["id"] == sel
        full = highlighted(r, sel, 7, radius)
        assert np.array_equal(full, model_of(frame, ids, W, H, 7, radius, 96, [sel])[0])
    differ_near_the_seam = 0
    for r0, n in ((0, seam), (seam, H - seam)):
        with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, first_row=r0, rows=n) as r:
            part = r.render()
            assert np.array_equal(part, frame[r0 * W:(r0 + n) * W])
            got = highlighted(r, sel, 7, radius)
            own = model_of(part, ids[r0 * W:(r0 + n) * W], W, n, 7, radius, 96, [sel])[0]
            assert got.shape == (n * W,) and np.array_equal(got, own)
            # rows at least `radius` from the seam are the full frame's
            keep = slice(0, (seam - radius) * W) if r0 == 0 else slice(radius * W, None)
            assert np.array_equal(got[keep], full[r0 * W:(r0 + n) * W][keep])
            near = slice((seam - radius) * W, None) if r0 == 0 else slice(0, radius * W)
            differ_near_the_seam += int((got[near] != full[r0 * W:(r0 + n) * W][near]).sum())
    print(f"seam at row {seam}, {'strict' if strict else 'fast'}: {differ_near_the_seam} pixels within {radius} rows of it differ from the full frame's")


# ------------------------------------------------------------------ 6. sampling modes
def test_supersampled_frame(R, api, demo_scene, tex, sky, strict):
    W, H = 61, 43
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, supersample=2) as r:
        frame = r.render()
        ids = r.gbuffer(api.GB_ID)["id"]
        sel = r.pick(*sphere_pixel(ids, W))["id"]
        got = highlighted(r, sel)
        assert got.shape == (W * H,) and np.array_equal(got, model_of(frame, ids, W, H, 7, 2, 96, [sel])[0])
        assert np.array_equal(read_framebuffer(r), frame)


def test_an_accumulating_view_keeps_counting(R, api, demo_scene, tex, sky, strict):
    W, H = 61, 43
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as plain:
        for _ in range(3):
            plain.render()
        want = plain.render_rgb()
        assert plain.accumulated == 4
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as r:
        ids = r.gbuffer(api.GB_ID)["id"]
        sel = r.pick(*sphere_pixel(ids, W))["id"]
        for f in range(3):
            frame = r.render()
            assert r.accumulated == f + 1
            assert np.array_equal(highlighted(r, sel), model_of(frame, ids, W, H, 7, 2, 96, [sel])[0])
            assert r.accumulated == f + 1
        got = r.render_rgb()
        assert r.accumulated == 4
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


# ------------------------------------------------------------------ 7. refusals: 0, and the process goes on
def test_refusals_return_zero_and_the_process_renders_on(R, api, demo_scene, tex, sky, strict):
    W, H = 70, 32
    S = lambda flags=7, radius=2, alpha=96: api.overlay_style(flags, radius, OUTLINE, FILL, alpha, EDGE)
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as ref:
        want = ref.render()
        ids = ref.gbuffer(api.GB_ID)["id"]
    with R(demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:          # a scene, but no camera latched yet
        assert r.w.render_overlay(S(), [0]) == 0
        with pytest.raises(RuntimeError):
            r.highlight(0)
        assert r.w.read_overlay().size == 0 and not r.w.overlay_device_ptr()
        r.look(**CAM)
        frame = r.render()
        assert np.array_equal(frame, want)
        for what, style, sel in (("65 ids", S(), np.arange(65)), ("radius 0", S(1, 0), [0]), ("radius 5", S(7, 5), [0]), ("alpha 257", S(2, 2, 257), [0]),
                                 ("unknown flag", S(8), [0]), ("unknown flag beside known ones", S(7 | 32), [0]), ("no flag", S(0), [0])):
            assert r.w.render_overlay(style, sel) == 0, what
        assert r.w.read_overlay().size == 0                                    # no refused call composed anything
        with pytest.raises(RuntimeError):
            r.highlight(0, radius=5)
        assert np.array_equal(r.render(), want)
        got = highlighted(r, 0)                                                # ... and the overlay works behind them
        assert np.array_equal(got, model_of(want, ids, W, H, 7, 2, 96, [0])[0])
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, bands=(2, 1)) as b:      # row bands
        banded = b.render()
        assert b.w.render_overlay(S(), [0]) == 0
        with pytest.raises(RuntimeError):
            b.highlight(0)
        assert np.array_equal(b.render(), banded)
