"""The visible-object table on the GPU (include/hip_wrap_ext.h: clw_ext_object_stats, clw_ext_unit_object_stats; csrc/whitted_objects.inc)
against the numpy restatement of its rules in tests/objects_common.py -- the raw 48-byte records bit for bit, in both builds: the pass is
integer work.  The unit test feeds the kernels synthetic id and depth fields; the scene tests hold `objects()` to the model of `gbuffer(GB_ID |
GB_DEPTH)` from the same renderer, the strips' tables to their merge, and hold that nothing else of the wrapper moved.

Measured on the MI355X: 0 records differ from the model in every case of both builds (2 x 1008 unit cases, the two large-coordinate cases, the eight cases of
561 tiles, every scene test).  The census of the unit run, the same in both builds: foreign ids present in 114 cases and absent in 894, the rectangle clipped
in 378 and not in 630, an empty table in 168, a table of one record in 408 and of several in 432, of more than 1024 records (more than one
round of the compact kernel) in 30.  The demo scene shows 9 objects at 61 x 43 and at 160 x 120; its strips at the seam of row 32 hold 9 and 2
records, which merge into the frame's 9; the grid scene lists 161 of its 324 spheres, through the grid and through the linear scan alike."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_common as gc
import objects_common as oc
import overlay_common as ovc
from conftest import CAM
from render_common import R, api, bits, released, rendering  # noqa: F401  (R, api: the fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[True, False], ids=["strict", "fast"])
def strict(request):
    import torch  # noqa: F401
    return request.param


def read_framebuffer(r):
    """the framebuffer as it lies, without tracing: the read-back rides on the raygen launch, which in fused mode only latches the camera"""
    out = np.empty(r.pixels, np.uint32)
    r.w.output(r.pixels, out.nbytes, 0, 1, 10, out)
    return out


# ------------------------------------------------------------------ 1. the kernels on synthetic fields
_expected, _unit = {}, {}


def expected_unit(api, size):
    """[(case, ids, depth, counts, rect, records, summary, census) ...] of one size: computed once, shared by both builds, never written to; the C
    model is held to the numpy model on the way"""
    if size not in _expected:
        fields, rows = {}, []
        for case in oc.unit_cases([size]):
            w, h, first_row, rname, fname, with_depth = case
            if fname not in fields:
                ids, counts = oc.field(fname, w, h)
                depth = oc.depth_field(w, h)
                ids.setflags(write=False)
                depth.setflags(write=False)
                fields[fname] = (ids, counts, depth)
            ids, counts, depth = fields[fname]
            depth = depth if with_depth else None
            rect = oc.rect_of(rname, w, h, first_row)
            want, summary, census = oc.model(ids, depth, w, h, counts, first_row, rect)
            host, host_summary = api.object_stats(ids, depth, w, h, counts, first_row, rect)
            assert oc.same_records(host, want) and host_summary == summary, case
            rows.append((case, ids, depth, counts, rect, want, summary, census))
        _expected[size] = rows
    return _expected[size]


def run_unit(api, strict, size):
    """every case of one size through clw_ext_unit_object_stats -> the census of the cases that equalled the model (all of them, or the test fails)"""
    if (strict, size) not in _unit:
        total, bad = {}, []
        with released(api.ClWrap()) as w:
            w.set_strict(strict)
            for case, ids, depth, counts, rect, want, summary, census in expected_unit(api, size):
                got = w.unit_object_stats(ids, depth, case[0], case[1], counts, case[2], rect)
                assert got is not None, case
                if not (oc.same_records(got[0], want) and got[1] == summary):
                    bad.append((case, got[1], summary))
                oc.add_census(total, census)
        print(f"{size[0]} x {size[1]} {'strict' if strict else 'fast'}: {len(expected_unit(api, size))} cases, {len(bad)} differ from the model {bad[:6]}")
        assert not bad
        _unit[strict, size] = total
    return _unit[strict, size]


@pytest.mark.parametrize("size", oc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unit_table_equals_the_model(api, strict, size):
    run_unit(api, strict, size)


def test_unit_run_asks_every_rule_both_ways(api, strict):
    total = {}
    for size in oc.SIZES:
        oc.add_census(total, run_unit(api, strict, size))
    oc.assert_every_rule_fired_and_was_skipped(total)


@pytest.mark.parametrize("width,rows,first_row", oc.LARGE, ids=lambda v: str(v))
def test_unit_large_coordinates_need_64_bit_sums(api, strict, width, rows, first_row):
    ids = np.full((rows, width), 5, np.uint32)
    depth = None if first_row == 0 else np.full((rows, width), 2.5, np.float32)
    want, summary, _ = oc.model(ids, depth, width, rows, oc.COUNTS, first_row)
    with released(api.ClWrap()) as w:
        w.set_strict(strict)
        got = w.unit_object_stats(ids, depth, width, rows, oc.COUNTS, first_row)
    assert got is not None and got[1] == summary and oc.same_records(got[0], want)
    assert int(got[0]["sum_x" if first_row == 0 else "sum_y"][0]) >= 1 << 32


_run_expected = []


def test_unit_workgroups_that_walk_a_run_of_tiles(api, strict):
    """561 tiles: more than the launch has workgroups, so each walks consecutive tiles and keeps its LDS table across them"""
    (width, rows), first_row = oc.RUN_SIZE, oc.RUN_FIRST_ROW
    assert -(-width // 32) * -(-rows // 8) > 512
    if not _run_expected:
        depth = oc.depth_field(width, rows)
        for fname, rname in oc.RUN_CASES:
            ids, counts = oc.field(fname, width, rows)
            rect = oc.rect_of(rname, width, rows, first_row)
            _run_expected.append((fname, rname, ids, depth, counts, rect) + oc.model(ids, depth, width, rows, counts, first_row, rect)[:2])
    with released(api.ClWrap()) as w:
        w.set_strict(strict)
        for fname, rname, ids, depth, counts, rect, want, summary in _run_expected:
            got = w.unit_object_stats(ids, depth, width, rows, counts, first_row, rect)
            assert got is not None and got[1] == summary and oc.same_records(got[0], want), (fname, rname)


def test_unit_refusals_and_a_small_capacity(api, strict):
    ids, counts = oc.field("kinds", 33, 9)
    counts = np.array(counts, np.uint32)
    full, summary, _ = oc.model(ids, None, 33, 9, counts)
    with released(api.ClWrap()) as w:
        w.set_strict(strict)
        assert w.object_stats() is None                                           # no kernels, nothing latched
        assert w.unit_object_stats(ids, None, 33, 9, counts, 0, (1, 1, 0, 2)) is None
        assert w.unit_object_stats(ids, None, 33, 9, counts, 0, (1, 1, 2, 0)) is None
        assert w.unit_object_stats(ids, None, 33, 9, (1 << 24, 0, 0)) is None
        out = np.zeros(20, api.OBJECT_STAT)
        out["id"] = 0xA5A5A5A5
        s = api.clw_object_summary(7, 7, 7, 7)
        call = lambda capacity, sp: w.L.clw_ext_unit_object_stats(C.byref(w.w), api._ptr(ids), None, 33, 9, 0, None, api._ptr(counts), api._ptr(out), capacity, sp)
        assert call(20, None) == 0 and (out["id"] == 0xA5A5A5A5).all()            # a NULL summary
        assert call(5, C.byref(s)) == 1
        assert s.objects == len(full) == summary["objects"] and s.pixels == 33 * 9 and s.foreign == 0
        assert oc.same_records(out[:5], full[:5]) and (out["id"][5:] == 0xA5A5A5A5).all()


# ------------------------------------------------------------------ 2. a rendered scene
def model_of_gbuffer(g, W, rows, counts, first_row=0, rect=None):
    return oc.model(g["id"], g["depth"], W, rows, counts, first_row, rect)


@pytest.mark.parametrize("W,H", [(61, 43), (160, 120)])
def test_scene_table_equals_the_model(R, api, demo_scene, tex, sky, strict, W, H):
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:
        frame = r.render()
        g = r.gbuffer(api.GB_ID | api.GB_DEPTH)
        ids, depth = g["id"], g["depth"]
        before = highlighted = r.highlight(int(ids[0]))
        r.w.timing_reset()
        got = r.objects()
        want, summary, _ = model_of_gbuffer(g, W, H, demo_scene.counts)
        assert got.dtype == api.OBJECT_STAT and got.shape == want.shape
        print(f"{W} x {H} {'strict' if strict else 'fast'}: {len(got)} records, {int((got != want).sum())} differ from the model")
        assert oc.same_records(got, want)
        assert summary["foreign"] == 0 and int(got["pixels"].sum()) == W * H
        assert r.w.timing_get(api.TIMING_OBJECTS)[0] == 1 and r.w.timing_get(api.TIMING_GBUFFER)[0] == 1
        # each record's box contains a pixel that `pick` reports for that id
        for rec in got:
            px = int(np.flatnonzero(ids == rec["id"])[len(np.flatnonzero(ids == rec["id"])) // 2])
            x, y = px % W, px // W
            assert r.pick(x, y)["id"] == rec["id"]
            assert rec["x0"] <= x <= rec["x1"] and rec["y0"] <= y <= rec["y1"]
        # a rectangle around a picked sphere returns it
        on = np.flatnonzero(gc.kind_of(ids) == gc.KIND_SPHERE)
        px = int(on[on.size // 2])
        x, y = px % W, px // W
        sel = r.pick(x, y)["id"]
        rect = (max(x - 2, 0), max(y - 2, 0), 5, 5)
        around = r.objects(rect)
        assert oc.same_records(around, model_of_gbuffer(g, W, H, demo_scene.counts, 0, rect)[0]) and sel in around["id"]
        # rubber-band selection, fed to the overlay
        mine = got[got["id"] == sel][0]
        chosen = r.select_rect(int(mine["x1"]), int(mine["y1"]), int(mine["x0"]), int(mine["y0"]))
        inside = model_of_gbuffer(g, W, H, demo_scene.counts, 0, (int(mine["x0"]), int(mine["y0"]), int(mine["x1"] - mine["x0"]) + 1, int(mine["y1"] - mine["y0"]) + 1))[0]
        inside = inside[gc.kind_of(inside["id"]) <= gc.KIND_PLANE]
        order = sorted(range(len(inside)), key=lambda k: (-int(inside["pixels"][k]), int(inside["id"][k])))
        assert chosen.dtype == np.uint32 and list(chosen) == [int(inside["id"][k]) for k in order][:64] and sel in chosen
        assert list(r.select_rect(0, 0, W - 1, H - 1, min_pixels=W * H + 1)) == []
        assert (gc.kind_of(r.select_rect(0, 0, W - 1, H - 1, kinds=(api.ID_SPHERE,))) == gc.KIND_SPHERE).all()
        shown = r.highlight(chosen, outline=ovc.OUTLINE_RGB, radius=2, fill=ovc.FILL_RGB, alpha=96, edges=ovc.EDGE_RGB)
        assert np.array_equal(shown, ovc.model(frame, ids, W, H, 7, 2, ovc.OUTLINE_RGB, ovc.FILL_RGB, 96, ovc.EDGE_RGB, chosen)[0])
        # nothing else moved: the traced frame, the channels of the earlier pass, the overlay's read-back
        highlighted = r.highlight(int(ids[0]))
        assert np.array_equal(highlighted, before)
        r.objects()
        assert np.array_equal(r.w.read_overlay(), highlighted)
        assert np.array_equal(read_framebuffer(r), frame)
        assert np.array_equal(bits(r.w.read_gbuffer(api.GB_DEPTH)), bits(depth)) and np.array_equal(r.w.read_gbuffer(api.GB_ID), ids)
        assert np.array_equal(r.render(), frame)


def test_an_accumulating_view_keeps_counting(R, api, demo_scene, tex, sky, strict):
    W, H = 61, 43
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as plain:
        for _ in range(3):
            plain.render()
        want = plain.render_rgb()
        assert plain.accumulated == 4
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, accumulate=4) as r:
        g = r.gbuffer(api.GB_ID | api.GB_DEPTH)
        table = model_of_gbuffer(g, W, H, demo_scene.counts)[0]
        for f in range(3):
            r.render()
            assert r.accumulated == f + 1
            assert oc.same_records(r.objects(), table)
            assert r.accumulated == f + 1
        got = r.render_rgb()
        assert r.accumulated == 4
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


# ------------------------------------------------------------------ 3. row strips
def test_strips_merge_into_the_frame(R, api, demo_scene, tex, sky, strict):
    W, H = 61, 43
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:
        g = r.gbuffer(api.GB_ID | api.GB_DEPTH)
        full = r.objects()
        assert oc.same_records(full, model_of_gbuffer(g, W, H, demo_scene.counts)[0])
    # the seam between the two strips: the first row (a multiple of 8 if there is one) that a sphere crosses
    grid = g["id"].reshape(H, W)
    spheres_across = lambda s: [int(i) for i in np.intersect1d(grid[s - 1], grid[s]) if i >> 30 == gc.KIND_SPHERE]
    seams = [s for s in list(range(8, H, 8)) + list(range(1, H)) if spheres_across(s)]
    assert seams
    seam = seams[0]
    crossing = spheres_across(seam)[0]
    parts = []
    for r0, n in ((0, seam), (seam, H - seam)):
        with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, first_row=r0, rows=n) as r:
            got = r.objects()
            own = {k: v[r0 * W:(r0 + n) * W] for k, v in g.items()}
            assert oc.same_records(got, model_of_gbuffer(own, W, n, demo_scene.counts, r0)[0])          # boxes in frame coordinates
            assert crossing in got["id"] and int(got["y0"].min()) >= r0 and int(got["y1"].max()) < r0 + n
            rect = (5, max(seam - 3, 0), 40, 6)                                                                 # a rectangle across the seam
            assert oc.same_records(r.objects(rect), model_of_gbuffer(own, W, n, demo_scene.counts, r0, rect)[0])
            parts.append(got)
    merged = api.merge_object_stats(*parts)
    print(f"seam at row {seam}, {'strict' if strict else 'fast'}: {len(parts[0])} + {len(parts[1])} records merge into {len(merged)}")
    assert oc.same_records(merged, full)
    rec = merged[merged["id"] == crossing][0]
    assert rec["y0"] < seam <= rec["y1"]


# ------------------------------------------------------------------ 4. a scene on the uniform grid
def test_grid_scene_lists_every_sphere_in_sight(R, api, tex, sky, strict):
    _, W, H, cam, _ = gc.CASES["D1"]
    sc = gc.case_scene("D1")
    tables = []
    for grid in (True, False):
        with rendering(R, sc, tex, sky, W, H, cam=cam, depth=4, strict=strict, setup=None if grid else (lambda w: w.set_grid(0))) as r:
            r.render()
            assert bool(r.w.last_trace_flags() & 16) == grid          # WT_F_GRID
            g = r.gbuffer(api.GB_ID | api.GB_DEPTH)
            got = r.objects()
            assert oc.same_records(got, model_of_gbuffer(g, W, H, sc.counts)[0])
            tables.append(got)
    assert oc.same_records(*tables)
    spheres = tables[0]["id"][gc.kind_of(tables[0]["id"]) == gc.KIND_SPHERE]
    seen = np.unique(g["id"][gc.kind_of(g["id"]) == gc.KIND_SPHERE])
    print(f"grid scene {'strict' if strict else 'fast'}: {spheres.size} sphere records of {len(tables[0])}")
    assert spheres.size > 128 and np.array_equal(spheres, seen)


# ------------------------------------------------------------------ 5. refusals: 0, and the process goes on
def test_refusals_return_zero_and_the_process_renders_on(R, api, demo_scene, tex, sky, strict):
    W, H = 70, 32
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict) as ref:
        want = ref.render()
        g = ref.gbuffer(api.GB_ID | api.GB_DEPTH)
    table = model_of_gbuffer(g, W, H, demo_scene.counts)[0]
    with R(demo_scene, tex, sky, W, H, depth=4, strict=strict) as r:          # a scene, but no camera latched yet
        assert r.w.object_stats() is None
        with pytest.raises(RuntimeError):
            r.objects()
        r.look(**CAM)
        assert np.array_equal(r.render(), want)
        out = np.zeros(4, api.OBJECT_STAT)
        out["id"] = 0xA5A5A5A5
        s = api.clw_object_summary(7, 7, 7, 7)
        for what, rect, sp in (("a rectangle of zero width", api.clw_rect(3, 3, 0, 5), C.byref(s)), ("a rectangle of zero height", api.clw_rect(3, 3, 5, 0), C.byref(s)),
                               ("a NULL summary", None, None)):
            assert r.w.L.clw_ext_object_stats(C.byref(r.w.w), C.byref(rect) if rect is not None else None, api._ptr(out), 4, sp) == 0, what
            assert (out["id"] == 0xA5A5A5A5).all() and (s.objects, s.pixels, s.foreign, s.reserved) == (7, 7, 7, 7), what
        with pytest.raises(RuntimeError):
            r.objects((3, 3, 0, 5))
        with pytest.raises(RuntimeError):
            r.select_rect(-1, 0, 5, 5)
        assert np.array_equal(r.render(), want)
        assert oc.same_records(r.objects(), table)                            # ... and the table works behind them
        assert len(r.objects((0, H, W, 9))) == 0                              # below the frame: empty, not refused
    with rendering(R, demo_scene, tex, sky, W, H, depth=4, strict=strict, bands=(2, 1)) as b:      # row bands
        banded = b.render()
        assert b.w.object_stats() is None
        with pytest.raises(RuntimeError):
            b.objects()
        assert np.array_equal(b.render(), banded)
