"""The selection overlay without a GPU: the C model clw_host_overlay (csrc/overlay_host.c) against the numpy restatement of overlay_common.py on
every case of the GPU unit test, its refusals, its properties, the corruptions the comparison must reject, and the ABI."""
import ctypes as C
import re

import numpy as np
import pytest

import overlay_common as oc
from render_common import api, declared_symbols, header_text  # noqa: F401  (api: the fixture)

NEW = ["clw_host_overlay", "clw_ext_render_overlay", "clw_ext_read_overlay", "clw_ext_overlay_device_ptr", "clw_ext_unit_overlay"]


def style_of(api, flags, radius, alpha):
    return api.overlay_style(flags, radius, oc.OUTLINE_RGB, oc.FILL_RGB, alpha, oc.EDGE_RGB)


def model_of(frame, ids, width, rows, flags, radius, alpha, sel, corrupt=None):
    return oc.model(frame, ids, width, rows, flags, radius, oc.OUTLINE_RGB, oc.FILL_RGB, alpha, oc.EDGE_RGB, sel, corrupt)


# ------------------------------------------------------------------ 1. the ABI
def test_header_library_and_mirror_agree_on_the_new_symbols(api):
    declared = declared_symbols()
    L = api.load_library()
    for name in NEW:
        assert name in declared and name in api.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None
    assert C.sizeof(api.clw_overlay) == 24
    assert [f[0] for f in api.clw_overlay._fields_] == ["flags", "radius", "outline_rgb", "fill_rgb", "fill_alpha", "edge_rgb"]
    defs = dict(re.findall(r"#define\s+(CLW_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", header_text()))
    want = dict(CLW_OV_OUTLINE=api.OV_OUTLINE, CLW_OV_FILL=api.OV_FILL, CLW_OV_EDGES=api.OV_EDGES, CLW_TIMING_OVERLAY=api.TIMING_OVERLAY)
    for name, value in want.items():
        assert int(defs[name], 0) == value, name
    assert (api.OV_OUTLINE, api.OV_FILL, api.OV_EDGES) == (oc.OV_OUTLINE, oc.OV_FILL, oc.OV_EDGES) and api.ID_NONE == oc.ID_NONE
    assert "latched mode" in header_text()          # the header says what is not built


def test_renderer_and_wrapper_have_the_overlay():
    import inspect
    from example_gui_opencl_raytracer_amd import api
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    p = inspect.signature(Renderer.highlight).parameters
    assert list(p) == ["self", "ids", "outline", "radius", "fill", "alpha", "edges"]
    assert (p["outline"].default, p["radius"].default, p["fill"].default, p["alpha"].default, p["edges"].default) == (0xFFFF00, 2, None, 96, None)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    for name in ("render_overlay", "read_overlay", "overlay_device_ptr", "unit_overlay"):
        assert callable(getattr(api.ClWrap, name))


# ------------------------------------------------------------------ 2. the C model is the numpy model
@pytest.mark.parametrize("width,rows", oc.SIZES)
def test_c_model_equals_the_numpy_model(api, width, rows):
    frame = oc.frame_of(width, rows)
    fields = {}
    for w, h, radius, flags, name, sel, alpha in oc.unit_cases([(width, rows)]):
        ids = fields.setdefault((name, len(sel)), oc.field(name, w, h, sel))
        want, _ = model_of(frame, ids, w, h, flags, radius, alpha, sel)
        got = api.overlay(frame, ids, w, h, style_of(api, flags, radius, alpha), sel)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (w, h, radius, flags, name, len(sel), alpha)
        assert not (got >> np.uint32(24)).any()


def test_the_unit_cases_ask_every_rule_both_ways():
    """what the GPU unit test asserts of its run holds of the model alone, for the seeds chosen"""
    total = {}
    for w, h, radius, flags, name, sel, alpha in oc.unit_cases():
        _, census = model_of(oc.frame_of(w, h), oc.field(name, w, h, sel), w, h, flags, radius, alpha, sel)
        oc.add_census(total, census)
    oc.assert_every_rule_fired_and_was_skipped(total)


def test_an_empty_selection_draws_edges_only(api):
    w, h = 9, 9
    frame, ids = oc.frame_of(w, h), oc.field("noise3", w, h, oc.selection(1))
    none = np.zeros(0, np.uint32)
    got = api.overlay(frame, ids, w, h, style_of(api, 7, 2, 96), None)
    assert np.array_equal(got, model_of(frame, ids, w, h, 7, 2, 96, none)[0])
    assert np.array_equal(got, model_of(frame, ids, w, h, oc.OV_EDGES, 2, 96, none)[0])
    assert np.array_equal(api.overlay(frame, ids, w, h, style_of(api, 3, 2, 96), None), frame & np.uint32(0xFFFFFF))


def test_the_sky_can_be_selected(api):
    w, h = 8, 8
    ids = np.full((h, w), 5, np.uint32)
    ids[2:5, 3:6] = oc.ID_NONE
    frame = oc.frame_of(w, h)
    got = api.overlay(frame, ids, w, h, style_of(api, 3, 1, 256), [oc.ID_NONE]).reshape(h, w)
    assert (got[2:5, 3:6] == oc.FILL_RGB).all() and (got[1:6, 2:7][ids[1:6, 2:7] == 5] == oc.OUTLINE_RGB).all()
    assert np.array_equal(got[0], frame.reshape(h, w)[0] & np.uint32(0xFFFFFF))


# ------------------------------------------------------------------ 3. refusals: 0, and `out` untouched
def test_refusals_return_zero_and_write_nothing(api):
    L = api.load_library()
    w, h = 5, 3
    frame, ids = oc.frame_of(w, h), oc.field("checker", w, h, oc.selection(1))
    sel = oc.selection(64)
    big = np.arange(65, dtype=np.uint32)
    S = lambda flags, radius=2, alpha=96: api.overlay_style(flags, radius, 1, 2, alpha, 3)
    sentinel = np.uint32(0xA5A5A5A5)

    def call(frame=frame, ids=ids, width=w, rows=h, style=S(7), sel=sel, count=64):
        out = np.full(w * h, sentinel, np.uint32)
        ret = L.clw_host_overlay(api._ptr(frame), api._ptr(ids), width, rows, C.byref(style) if style is not None else None,
                                 api._ptr(sel) if sel is not None else None, count, api._ptr(out))
        return ret, bool((out == sentinel).all())

    assert call() == (1, False)                                   # the call itself is fine
    refused = {
        "unknown flag bit": dict(style=S(8)), "unknown flag bit beside known ones": dict(style=S(7 | 16)), "top flag bit": dict(style=S(1 << 31)),
        "no flag": dict(style=S(0)),
        "OUTLINE radius 0": dict(style=S(1, 0)), "OUTLINE radius 5": dict(style=S(3, 5)), "OUTLINE radius 2^32 - 1": dict(style=S(7, 0xFFFFFFFF)),
        "FILL alpha 257": dict(style=S(2, 2, 257)), "FILL alpha 2^32 - 1": dict(style=S(6, 2, 0xFFFFFFFF)),
        "65 ids": dict(sel=big, count=65), "ids without their array": dict(sel=None, count=1),
        "zero width": dict(width=0), "zero rows": dict(rows=0),
    }
    for what, kw in refused.items():
        assert call(**kw) == (0, True), what
    # what is read only with its flag is not checked without it; count == 0 needs no array
    assert call(style=S(6, 0))[0] == 1 and call(style=S(4, 77))[0] == 1 and call(style=S(1, 4, 999))[0] == 1 and call(style=S(5, 1, 257))[0] == 1
    assert call(sel=None, count=0)[0] == 1 and call(count=0)[0] == 1
    with pytest.raises(ValueError):
        api.overlay(frame, ids, w, h, S(0), [7])
    with pytest.raises(ValueError):
        api.overlay(frame, ids, w, h + 1, S(7), [7])


# ------------------------------------------------------------------ 4. properties
SHAPES = [(61, 43), (9, 9), (130, 17)]


@pytest.mark.parametrize("width,rows", SHAPES)
def test_properties(api, width, rows):
    frame = oc.frame_of(width, rows, seed=3)
    for name, count in [(n, c) for n in oc.FIELDS for c in oc.SELECTIONS]:
        sel = oc.selection(count)
        ids = oc.field(name, width, rows, sel, seed=3)
        selected = np.isin(ids.reshape(-1), sel)
        plain = frame & np.uint32(0xFFFFFF)
        # alpha 0 with FILL alone: the frame, less its top byte
        assert np.array_equal(api.overlay(frame, ids, width, rows, style_of(api, oc.OV_FILL, 2, 0), sel), plain)
        # alpha 256 paints fill_rgb exactly, on the selected pixels and no other
        full = api.overlay(frame, ids, width, rows, style_of(api, oc.OV_FILL, 2, 256), sel)
        assert (full[selected] == oc.FILL_RGB).all() and np.array_equal(full[~selected], plain[~selected])
        # no outlined pixel is selected; the outline of radius r lies inside that of r + 1
        previous = None
        for radius in oc.RADII:
            out = api.overlay(frame, ids, width, rows, style_of(api, oc.OV_OUTLINE, radius, 0), sel)
            drawn = out != plain                   # (a frame pixel that already has the outline's colour would hide: the seeds hold none)
            assert not (plain == oc.OUTLINE_RGB).any()
            assert not (drawn & selected).any() and (out[drawn] == oc.OUTLINE_RGB).all()
            if previous is not None:
                assert not (previous & ~drawn).any()
            previous = drawn
        # OUTLINE + FILL at alpha 256: a selected pixel is never covered by its own outline
        both = api.overlay(frame, ids, width, rows, style_of(api, 3, 4, 256), sel)
        assert (both[selected] == oc.FILL_RGB).all()


# ------------------------------------------------------------------ 5. the comparison rejects a wrong model
@pytest.mark.parametrize("corrupt", ["inner", "outline_under_fill", "no_round", "fill_first"])
def test_corruptions_are_rejected(api, corrupt):
    """inner instead of outer band; FILL applied after OUTLINE (the dilated selection painted first, the object filled over it); >> 8 without the
    + 128; FILL before EDGES -- each differs from the C model on the unit cases"""
    rejected = 0
    for w, h, radius, flags, name, sel, alpha in oc.unit_cases([(61, 43), (9, 9)]):
        frame, ids = oc.frame_of(w, h), oc.field(name, w, h, sel)
        got = api.overlay(frame, ids, w, h, style_of(api, flags, radius, alpha), sel)
        rejected += not np.array_equal(got, model_of(frame, ids, w, h, flags, radius, alpha, sel, corrupt)[0])
    print(f"corruption {corrupt}: rejected in {rejected} cases")
    assert rejected > 0
    # and on the plainest case each names: a 3 x 3 block selected in a 9 x 9 frame with a second object beside it, everything drawn, alpha 96
    ids = np.zeros((9, 9), np.uint32)
    ids[3:6, 3:6] = 7
    ids[4:6, 5:8] = 9
    frame = oc.frame_of(9, 9)
    got = api.overlay(frame, ids, 9, 9, style_of(api, 7, 1, 96), [7])
    assert np.array_equal(got, model_of(frame, ids, 9, 9, 7, 1, 96, [7])[0])
    assert not np.array_equal(got, model_of(frame, ids, 9, 9, 7, 1, 96, [7], corrupt)[0])


def test_exchanging_fill_and_outline_as_written_changes_nothing():
    """Rule 3 changes selected pixels only, rule 4 unselected ones only: applied in either order they give the same frame, so "FILL after
    OUTLINE" can only be told from the definition in the form test_corruptions_are_rejected[outline_under_fill] rejects."""
    for w, h, radius, flags, name, sel, alpha in oc.unit_cases([(61, 43), (9, 9)]):
        frame, ids = oc.frame_of(w, h), oc.field(name, w, h, sel)
        assert np.array_equal(model_of(frame, ids, w, h, flags, radius, alpha, sel)[0], model_of(frame, ids, w, h, flags, radius, alpha, sel, "fill_last")[0])
