"""Shared by test_primary_cull_host.py, test_gpu_primary_cull.py and test_gpu_cull_twins.py: the primary-ray cull table (include/hip_wrap_ext.h:
clw_host_primary_cull, clw_ext_read_primary_cull; csrc/primary_cull_host.h states the rule) held to what the trace kernel relies on -- the line
test D >= 0 of the oracle's intersect_sphere in float32 (`check_case`: soundness and the margin) --, and the one driver of the GPU tests
(`on_and_off`): a view rendered with and without its table, compared bit for bit, its device table held to the host definition and its launch
to the flag word of the twin kernel (`wt_trace_cull<FLAGS>`, csrc/whitted_trace.inc) the case names."""
import numpy as np

from oracle.oracle_py import Camera
from example_gui_opencl_raytracer_amd import api

F = np.float32
NO_CULL = 32768                         # clw_ext_set_variant: the launch is given no table (csrc/launch_plan.h: WT_V_NO_CULL)


def oracle_camera(cam):
    return Camera.from_buffer_copy(bytes(cam))


def disc32(o, d, c, r):
    """D of the oracle's intersect_sphere (oracle/whitted_oracle.c; primitives.cl:170-195), float32 operation by operation; d: [n, 3]"""
    dot = lambda a, b: a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    v = (o - c).astype(F)
    a = dot(d, d)
    b = dot(v * F(2), d)
    cc = dot(v, v) - r * r
    return b * b - F(4) * a * cc


def disc64_rel(o, d, c, r):
    """D / 4 over |c - o|^2 for the float32 directions taken as exact, in float64 and with a = 1: sin^2 alpha - sin^2 phi of the header"""
    o, d, c, r = (np.asarray(x, np.float64) for x in (o, d, c, r))
    v = o - c
    L2 = (v * v).sum()
    if not L2 > 0:      # the origin is the centre: every line passes
        return np.full(d.shape[0], np.inf)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    b = (d * v).sum(-1)
    return (b * b - (L2 - r * r)) / L2


def tile_any(flag, W, rows):
    """per-pixel flags [rows * W] -> [tile rows, tiles per row]: any pixel of the tile"""
    trows, tpr = (rows + 7) // 8, (W + 7) // 8
    pad = np.zeros((trows * 8, tpr * 8), bool)
    pad[:rows, :W] = flag.reshape(rows, W)
    return pad.reshape(trows, 8, tpr, 8).any(axis=(1, 3))


def tile_max(val, W, rows):
    trows, tpr = (rows + 7) // 8, (W + 7) // 8
    pad = np.full((trows * 8, tpr * 8), -np.inf)
    pad[:rows, :W] = val.reshape(rows, W)
    return pad.reshape(trows, 8, tpr, 8).max(axis=(1, 3))


def launch_rays(oracle, cam, rows, row_offset, bands):
    """origins and directions of the launch's pixels in local row order, as the trace kernel maps them"""
    W = int(cam.width)
    rays = oracle.raygen(oracle_camera(cam))
    if bands:
        stride, phase = bands
        y = np.arange(rows)
        gy = ((y >> 3) * stride + phase) * 8 + (y & 7)
    else:
        gy = row_offset + np.arange(rows)
    ids = (gy[:, None] * W + np.arange(W)[None, :]).reshape(-1)
    return rays[ids, 0:3], rays[ids, 4:7]


def check_case(oracle, cam, sc, rows=None, row_offset=0, bands=None):
    """-> (table, per-tile 'some pixel passes the line test' for spheres and lights); asserts soundness and the margin"""
    rows = int(cam.height) if rows is None else rows
    W = int(cam.width)
    table = api.host_primary_cull(cam, sc.spheres, sc.lights, rows=rows, row_offset=row_offset, band_stride=bands[0] if bands else 1,
                                  band_phase=bands[1] if bands else 0)
    o, d = launch_rays(oracle, cam, rows, row_offset, bands)
    out = []
    for bit, prims in ((api.CULL_SPHERES, sc.spheres), (api.CULL_LIGHTS, sc.lights)):
        passes = np.zeros((table.shape[0], table.shape[1]), bool)
        worst = np.full(table.shape, -np.inf)
        for p in prims:
            c, r = p["origin"].astype(F), F(p["radius"])
            D = disc32(o[0], d, c, r)
            passes |= tile_any(~(D < 0), W, rows)
            worst = np.maximum(worst, tile_max(disc64_rel(o[0], d, c, r), W, rows))
        set_ = (table & bit) != 0
        assert not (set_ & passes).any(), ("a set bit over a tile with D >= 0", bit, np.argwhere(set_ & passes)[:4])
        if len(prims):
            assert (worst[set_] <= -4e-6).all(), ("margin", bit, worst[set_].max())
        out.append(passes)
    return table, out[0], out[1]


def shares(name, tables):
    t = np.concatenate([x.reshape(-1) for x in tables])
    s0, s1 = float(((t & 1) != 0).mean()), float(((t & 2) != 0).mean())
    print(f"{name}: {t.size} tiles, bit 0 (spheres) set in {100 * s0:.1f} %, bit 1 (lights) set in {100 * s1:.1f} %")
    return s0, s1


# ---- the GPU side
def no_table(w, builds):
    """the last whole-range trace launch had no table, and the builder has run `builds` times"""
    table, n = w.read_primary_cull()
    return table is None and n == builds


def on_and_off(r, what, *, cam=None, flags=None, variant=0, expect_table=True, counting=False, asserted=None, build=None, **host_range):
    """The first frame of a view (no table yet: a view is built for when it comes twice in a row), a frame with the table, a frame without it
    (`variant` | 32768), a frame with it again: all the same bits, packed and float (the first frame packed: the float output is read behind
    a launch of its own, which would be the view's second) -> (the table-off frame, the device table).

    cam (a camera dict): the device table is api.host_primary_cull of that camera over the renderer's frame and scene (`host_range`: the rows,
    row_offset, band_stride, band_phase of a strip or a band share), byte for byte.  flags: the flag word every launch must report
    (clw_ext_last_trace_flags); with `asserted` and `build` the pair (build, flags) is added to that set once the case has passed.  counting:
    the launches' ray counters are the same with and without the table."""
    from render_common import assert_same_frames, take
    w = r.w
    w.set_variant(variant)
    first = r.render().copy()      # (one trace launch; a frame of `take` is two: the float output is read behind a launch of its own)
    assert no_table(w, 0), what
    words = [w.last_trace_flags()]
    counters = []

    def shot(v):
        w.set_variant(v)
        if counting:
            w.read_counters()      # (reading clears them)
        frame = take(r, 1)[0]
        words.append(w.last_trace_flags())
        if counting:
            counters.append(w.read_counters())
        return frame
    on = shot(variant)
    table, builds = w.read_primary_cull()
    assert (table is not None) == expect_table and builds == (1 if expect_table else 0), (what, builds)
    off = shot(variant | NO_CULL)
    assert w.read_primary_cull()[0] is None, what
    again = shot(variant)
    table2, builds = w.read_primary_cull()
    assert builds == (1 if expect_table else 0), (what, builds)      # the table built once serves the view again
    assert (table2 is not None) == expect_table and (table is None or np.array_equal(table, table2)), what
    assert np.array_equal(first, off[0]), what
    assert_same_frames([on, again], off[0], off[1], what)
    if counting:
        assert counters[0] == counters[1] == counters[2] and counters[0]["segments"] > r.pixels, (what, counters)
    if flags is not None:
        assert all(x == flags for x in words), (what, [hex(x) for x in words], hex(flags))
    if cam is not None and expect_table:
        c = api.perspective(cam["origin"], cam["look"], cam["fov"], cam["focal"], r.width, r.height)
        host = api.host_primary_cull(c, r.scene.spheres, r.scene.lights, **host_range).reshape(-1)
        assert table.shape == host.shape and table.tobytes() == host.tobytes(), (what, int((table != host).sum()))
    if asserted is not None and flags is not None and expect_table:
        asserted.add((build, flags))
    return off, table
