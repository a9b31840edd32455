"""The visible-object table without a GPU: the C model clw_host_object_stats (csrc/objects_host.c) against the numpy restatement of
objects_common.py on every case of the GPU unit test, the merge of strips, its refusals, the capacity rule and the ABI."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import objects_common as oc
from render_common import api, declared_symbols, header_text  # noqa: F401  (api: the fixture)

NEW = ["clw_host_object_stats", "clw_host_merge_object_stats", "clw_ext_object_stats", "clw_ext_unit_object_stats"]


# ------------------------------------------------------------------ 1. the ABI
def test_header_library_and_mirror_agree_on_the_new_symbols(api):
    declared = declared_symbols()
    L = api.load_library()
    for name in NEW:
        assert name in declared and name in api.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None
    assert (C.sizeof(api.clw_rect), C.sizeof(api.clw_object_stat), C.sizeof(api.clw_object_summary)) == (16, 48, 16)
    assert [f[0] for f in api.clw_rect._fields_] == ["x", "y", "width", "height"]
    assert [f[0] for f in api.clw_object_stat._fields_] == oc.FIELD_ORDER
    assert [f[0] for f in api.clw_object_summary._fields_] == ["objects", "pixels", "foreign", "reserved"]
    assert api.OBJECT_STAT.itemsize == 48 and list(api.OBJECT_STAT.names) == oc.FIELD_ORDER and api.OBJECT_STAT == oc.OBJECT_STAT
    for name in oc.FIELD_ORDER:                     # the dtype and the structure lay every field at the same place
        assert api.OBJECT_STAT.fields[name][1] == getattr(api.clw_object_stat, name).offset, name
    # the header declares the three structures with their fields in that order
    text = header_text(comments=False)
    stat = re.search(r"typedef struct clw_object_stat \{(.*?)\} clw_object_stat;", text, re.S).group(1)
    assert re.findall(r"\b(id|pixels|x0|y0|x1|y1|depth_min|depth_max|sum_x|sum_y)\b", stat) == oc.FIELD_ORDER
    assert re.search(r"typedef struct clw_rect \{ uint32_t x, y, width, height; \} clw_rect;", text)
    assert re.search(r"typedef struct clw_object_summary \{ uint32_t objects, pixels, foreign, reserved; \} clw_object_summary;", text)
    defs = dict(re.findall(r"#define\s+(CLW_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", header_text()))
    assert int(defs["CLW_TIMING_OBJECTS"], 0) == api.TIMING_OBJECTS == 0x4F424A53
    assert api.ID_NONE == oc.ID_NONE
    assert "per-frame automatic table" in header_text()          # the header says what is not built


def test_renderer_and_wrapper_have_the_table():
    from example_gui_opencl_raytracer_amd import api
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    p = inspect.signature(Renderer.objects).parameters
    assert list(p) == ["self", "rect"] and p["rect"].default is None
    p = inspect.signature(Renderer.select_rect).parameters
    assert list(p) == ["self", "x0", "y0", "x1", "y1", "min_pixels", "kinds"]
    assert p["min_pixels"].default == 1 and tuple(p["kinds"].default) == (api.ID_SPHERE, api.ID_PLANE)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("min_pixels", "kinds"))
    for name in ("object_stats", "unit_object_stats"):
        assert callable(getattr(api.ClWrap, name))
    assert callable(api.object_stats) and callable(api.merge_object_stats)


# ------------------------------------------------------------------ 2. the C model is the numpy model
_fields = {}


def case_inputs(width, rows, fname, with_depth):
    key = (width, rows, fname)
    if key not in _fields:
        ids, counts = oc.field(fname, width, rows)
        ids.setflags(write=False)
        _fields[key] = (ids, counts, oc.depth_field(width, rows))
    ids, counts, depth = _fields[key]
    return ids, counts, depth if with_depth else None


@pytest.mark.parametrize("width,rows", oc.SIZES)
def test_c_model_equals_the_numpy_model(api, width, rows):
    total = {}
    for w, h, first_row, rname, fname, with_depth in oc.unit_cases([(width, rows)]):
        ids, counts, depth = case_inputs(w, h, fname, with_depth)
        rect = oc.rect_of(rname, w, h, first_row)
        want, summary, census = oc.model(ids, depth, w, h, counts, first_row, rect)
        got, got_summary = api.object_stats(ids, depth, w, h, counts, first_row, rect)
        assert got.dtype == api.OBJECT_STAT and oc.same_records(got, want), (w, h, first_row, rname, fname)
        assert got_summary == summary, (w, h, first_row, rname, fname)
        assert int(want["pixels"].sum()) + summary["foreign"] == summary["pixels"]
        oc.add_census(total, census)
    if (width, rows) == (61, 43):
        oc.assert_every_rule_fired_and_was_skipped(total)


def test_c_model_equals_the_numpy_model_on_the_run_cases(api):
    (width, rows), first_row = oc.RUN_SIZE, oc.RUN_FIRST_ROW
    depth = oc.depth_field(width, rows)
    for fname, rname in oc.RUN_CASES:
        ids, counts = oc.field(fname, width, rows)
        rect = oc.rect_of(rname, width, rows, first_row)
        want, summary, _ = oc.model(ids, depth, width, rows, counts, first_row, rect)
        got, got_summary = api.object_stats(ids, depth, width, rows, counts, first_row, rect)
        assert oc.same_records(got, want) and got_summary == summary, (fname, rname)


@pytest.mark.parametrize("width,rows,first_row", oc.LARGE)
def test_large_coordinates_need_64_bit_sums(api, width, rows, first_row):
    ids = np.full((rows, width), 5, np.uint32)
    got, summary = api.object_stats(ids, None, width, rows, oc.COUNTS, first_row)
    want, want_summary, _ = oc.model(ids, None, width, rows, oc.COUNTS, first_row)
    assert oc.same_records(got, want) and summary == want_summary and len(got) == 1
    xs, ys = rows * (width * (width - 1) // 2), width * sum(range(first_row, first_row + rows))
    assert (int(got["sum_x"][0]), int(got["sum_y"][0])) == (xs, ys) and max(xs, ys) >= 1 << 32
    assert (xs if first_row == 0 else ys) >= 1 << 32


def test_depth_extremes_are_ordered_by_bit_pattern(api):
    """a NaN and negative values need no rule: as uint32 the negative ones are the largest"""
    ids = np.zeros((1, 6), np.uint32)
    depth = np.array([[2.0, -1.0, np.inf, 0.5, -0.0, np.nan]], np.float32)
    got, _ = api.object_stats(ids, depth, 6, 1, (1, 0, 0))
    assert oc.same_records(got, oc.model(ids, depth, 6, 1, (1, 0, 0))[0])
    assert got["depth_min"].view(np.uint32)[0] == np.float32(0.5).view(np.uint32) and got["depth_max"].view(np.uint32)[0] == np.float32(-1.0).view(np.uint32)
    none, _ = api.object_stats(ids, None, 6, 1, (1, 0, 0))
    assert none["depth_min"].view(np.uint32)[0] == 0 and none["depth_max"].view(np.uint32)[0] == 0


# ------------------------------------------------------------------ 3. merging strips
@pytest.mark.parametrize("width,rows", [(33, 9), (61, 43)])
def test_split_at_every_row_and_merged_is_the_whole(api, width, rows):
    first_row = 13
    for fname in oc.FIELDS:
        ids, counts, depth = case_inputs(width, rows, fname, True)
        for rect in (None, oc.rect_of("inside", width, rows, first_row), oc.rect_of("beyond", width, rows, first_row)):
            whole, _ = api.object_stats(ids, depth, width, rows, counts, first_row, rect)
            for r in range(1, rows):
                a, _ = api.object_stats(ids[:r], depth[:r], width, r, counts, first_row, rect)
                b, _ = api.object_stats(ids[r:], depth[r:], width, rows - r, counts, first_row + r, rect)
                merged = api.merge_object_stats(a, b)
                assert oc.same_records(merged, whole), (fname, rect, r)
                assert oc.same_records(api.merge_object_stats(b, a), merged)                    # commutative
            empty = np.zeros(0, api.OBJECT_STAT)
            assert oc.same_records(api.merge_object_stats(whole, empty), whole) and oc.same_records(api.merge_object_stats(empty, whole), whole)
    assert len(api.merge_object_stats(np.zeros(0, api.OBJECT_STAT), np.zeros(0, api.OBJECT_STAT))) == 0


def test_merge_capacity_and_count(api):
    L = api.load_library()
    ids, counts = oc.field("kinds", 33, 9)
    a, _ = api.object_stats(ids[:4], None, 33, 4, counts, 0)
    b, _ = api.object_stats(ids[4:], None, 33, 5, counts, 4)
    full = api.merge_object_stats(a, b)
    out = np.zeros(len(full), api.OBJECT_STAT)
    out["id"] = 0xA5A5A5A5
    n = L.clw_host_merge_object_stats(api._ptr(a), len(a), api._ptr(b), len(b), api._ptr(out), 3)
    assert n == len(full) and oc.same_records(out[:3], full[:3]) and (out["id"][3:] == 0xA5A5A5A5).all()


# ------------------------------------------------------------------ 4. refusals: 0, and `out` and `summary` untouched
def test_refusals_return_zero_and_write_nothing(api):
    L = api.load_library()
    w, h = 5, 3
    ids, counts = oc.field("kinds", w, h)
    counts = np.array(counts, np.uint32)
    sentinel = 0xA5A5A5A5

    def call(ids=ids, depth=None, width=w, rows=h, first_row=0, rect=None, counts=counts, with_out=True, with_summary=True):
        out = np.zeros(16, api.OBJECT_STAT)
        out["id"] = sentinel
        s = api.clw_object_summary(sentinel, sentinel, sentinel, sentinel)
        ret = L.clw_host_object_stats(api._ptr(ids), api._ptr(depth), width, rows, first_row, C.byref(api.clw_rect(*rect)) if rect else None,
                                      api._ptr(counts), api._ptr(out) if with_out else None, 16, C.byref(s) if with_summary else None)
        return ret, bool((out["id"] == sentinel).all()) and s.objects == sentinel and s.reserved == sentinel

    assert call() == (1, False)                                   # the call itself is fine
    refused = {
        "NULL ids": dict(ids=None), "NULL counts": dict(counts=None), "NULL summary": dict(with_summary=False),
        "zero width": dict(width=0), "zero rows": dict(rows=0),
        "a rectangle of zero width": dict(rect=(1, 1, 0, 2)), "a rectangle of zero height": dict(rect=(1, 1, 2, 0)),
        "2^24 slots + 1": dict(counts=np.array([(1 << 24) - 2, 1, 1], np.uint32)), "counts that overflow 32 bits": dict(counts=np.array([0xFFFFFFFF, 1, 0], np.uint32)),
        "2^30 pixels": dict(width=1 << 15, rows=1 << 15), "2^31 x 2 pixels": dict(width=1 << 31, rows=2),
    }
    for what, kw in refused.items():
        assert call(**kw) == (0, True), what
    # what is NOT refused: 2^24 slots exactly, a rectangle that misses the range (an empty table), no `out`
    ret, untouched = call(counts=np.array([(1 << 24) - 3, 1, 1], np.uint32))
    assert ret == 1 and not untouched
    for rect in ((0, h, w, 4), (w, 0, 1, 1), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        got, summary = api.object_stats(ids, None, w, h, counts, 0, rect)
        assert len(got) == 0 and summary == dict(objects=0, pixels=0, foreign=0), rect
    assert call(with_out=False)[0] == 1
    with pytest.raises(ValueError):
        api.object_stats(ids, None, w, h, counts, 0, (0, 0, 0, 1))
    with pytest.raises(ValueError):
        api.object_stats(ids, None, w, h + 1, counts)


def test_a_small_capacity_gets_the_prefix_and_the_full_count(api):
    L = api.load_library()
    w, h = 33, 9
    ids, counts = oc.field("kinds", w, h)
    counts = np.array(counts, np.uint32)
    full, summary = api.object_stats(ids, None, w, h, counts)
    assert summary["objects"] == len(full) == 14
    for capacity in (0, 1, 5, 14, 20):
        out = np.zeros(20, api.OBJECT_STAT)
        out["id"] = 0xA5A5A5A5
        s = api.clw_object_summary()
        assert L.clw_host_object_stats(api._ptr(ids), None, w, h, 0, None, api._ptr(counts), api._ptr(out), capacity, C.byref(s)) == 1
        n = min(capacity, 14)
        assert s.objects == 14 and s.pixels == w * h and oc.same_records(out[:n], full[:n]) and (out["id"][n:] == 0xA5A5A5A5).all(), capacity
