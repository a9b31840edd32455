"""The bounce cull table on the CPU (include/hip_wrap_ext.h: clw_host_bounce_cull; csrc/bounce_cull_host.h states the rule): a second byte per 8x8
tile, bits 0-3 = no shadow ray of the tile's first shade passes the line test of a sphere i with i % 4 = the bit, bit 4 / 5 = no ray of the tile's
second loop iteration passes the line test of any sphere / any light.

SOUNDNESS, against the trace kernel's arithmetic restated here in numpy float32 (wt_plane, the shading point, wt_light_sample_dir's sum,
wt_shadow_pre / wt_shadow_disc, wt_reflect, wt_sphere_disc): wherever a byte is not 0 every pixel of the tile meets the SAME plane first; wherever
a shadow bit is set, D < 0 for every pixel, 66 sample points spread over every light sphere and every sphere of the class; wherever a reflected
bit is set, D < 0 (a = 1 and a = d.d) for the reflected ray of every pixel from its offset hit and every primitive of the group.  MARGINS, in
float64 on the float32 points and directions: D / |c - p|^2 <= -8.8e-6 under a shadow bit (WT_BC_SHADOW_HELD: the header derives -8.99997e-6
for the exact line, the float32 direction moves it by < 2e-7), <= -3.5e-5 under a reflected bit (WT_BC_REFL_HELD: -3.59996e-5 for the exact
line, wt_reflect's roundings below 1e-6; every plane that carries bits here has an exactly unit normal).  Both relative to |c - p|^2 with p the
SHADING point, as the kernel computes D -- the families "image" and "under-image" put small spheres and lights next to the mirrored camera,
where |c - p| is many times the distance from the virtual origin.  The worst values seen are printed.
Families (every case is compared, none skipped): floor only, wall only, both (they meet inside tiles), a camera under the floor, primitives
near the camera's mirror images (camera above and under the floor), a normal that is not unit, a transparent plane, lights and spheres touching a footprint, spheres resting on the plane, depth 1; frames from 64x40 to 200x120
with widths that are no multiples of 8, row strips and band shares.

The demo view at 1920x1080 (test_demo_view_premise): the shares the estimate of the gain rests on."""
import numpy as np
import pytest

from conftest import CAM
from cull_common import launch_rays
from example_gui_opencl_raytracer_amd import api, scene

F = np.float32
EPS = F(0.001)
SHADOW_HELD, REFL_HELD = 8.8e-6, 3.5e-5      # csrc/bounce_cull_host.h: WT_BC_SHADOW_HELD, WT_BC_REFL_HELD (test_the_bounds_are_the_headers)
WORST = {"shadow": -np.inf, "reflected": -np.inf}      # the largest D / |c - p|^2 seen under a set bit


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def sphere_points(n=66):
    """n unit vectors spread over the sphere (a Fibonacci spiral and the six axis points)"""
    k = np.arange(n - 6) + 0.5
    z = 1.0 - 2.0 * k / (n - 6)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    fib = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    return np.concatenate([fib, np.eye(3), -np.eye(3)]).astype(F)


UNIT = sphere_points()


def first_planes(o, d, planes):
    """the nearest plane of every ray as the kernel finds it in float32 (wt_plane, strict `t >= tbest` keeps the earlier) -> (index or -1, t)"""
    best = np.full(d.shape[0], -1)
    tbest = np.full(d.shape[0], np.inf, F)
    for i, p in enumerate(planes):
        n, p0 = p["normal"].astype(F), p["point_in_plane"].astype(F)
        num = dot((p0 - o).astype(F), n)
        b = dot(d, n)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (num / b).astype(F)
        hit = (b != 0) & ~(t <= 0) & ~(t >= tbest)
        best[hit] = i
        tbest[hit] = t[hit]
    return best, tbest


def check_bounce(oracle, cam, sc, depth=4, rows=None, row_offset=0, bands=None):
    """-> (primary table, bounce table); asserts the soundness and the margins of every bit that is set"""
    rows = int(cam.height) if rows is None else rows
    W = int(cam.width)
    rng_ = dict(rows=rows, row_offset=row_offset, band_stride=bands[0] if bands else 1, band_phase=bands[1] if bands else 0)
    prim = api.host_primary_cull(cam, sc.spheres, sc.lights, **rng_)
    table = api.host_bounce_cull(cam, sc.spheres, sc.planes, sc.lights, depth=depth, **rng_)
    assert not (table[(prim & 1) == 0]).any(), "a bounce bit without the primary sphere bit"
    if depth < 2:
        assert not (table & 48).any()
    if not table.any():
        return prim, table
    o, d = launch_rays(oracle, cam, rows, row_offset, bands)
    o = o[0].astype(F)
    tpr = (W + 7) // 8
    y, x = np.divmod(np.arange(rows * W), W)
    tile = (y // 8) * tpr + x // 8
    byte = table.reshape(-1)[tile]                       # the byte of every pixel's tile
    sel = np.nonzero(byte)[0]
    d, tile, byte = d[sel], tile[sel], byte[sel]
    best, t = first_planes(o, d, sc.planes)
    assert (best >= 0).all(), "a tile with bits has a pixel that meets no plane"
    lo, hi = np.full(table.size, 99), np.full(table.size, -1)
    np.minimum.at(lo, tile, best); np.maximum.at(hi, tile, best)
    assert (lo[np.unique(tile)] == hi[np.unique(tile)]).all(), "a tile with bits meets two planes"
    nrm = np.stack([sc.planes[j]["normal"].astype(F) for j in best])
    for j in np.unique(best):
        assert abs(float(np.linalg.norm(sc.planes[j]["normal"].astype(np.float64))) - 1.0) <= 1.1e-6
        if (byte[best == j] & 48).any():
            assert sc.planes[j]["material"]["transperent"] == 0 and depth >= 2
    ip = ((d * t[:, None] + o).astype(F) + nrm * EPS).astype(F)      # (two roundings where the kernel's fma has one: below the slack by far)
    # ---- bits 0-3: every shadow line of the first shade
    for i, s in enumerate(sc.spheres):
        m = (byte >> (i & 3)) & 1 == 1
        if not m.any():
            continue
        c, r = s["origin"].astype(F), F(abs(s["radius"]))
        v = (ip[m] - c).astype(F)
        cc = (dot(v, v) - r * r).astype(F)
        v64 = v.astype(np.float64)
        L2 = (v64 * v64).sum(-1)
        for l in sc.lights:
            lf = (l["origin"].astype(F) - ip[m]).astype(F)
            to = (lf[:, None, :] + UNIT[None, :, :] * F(l["radius"])).astype(F)      # [pixels, samples, 3]
            rd = (to / np.sqrt(dot(to, to))[..., None]).astype(F)
            b = dot(v[:, None, :], rd)
            D = (b * b - cc[:, None]).astype(F)
            assert (D < 0).all(), ("a shadow bit over a line with D >= 0", i, float(D.max()))
            rd64 = rd.astype(np.float64)
            rd64 /= np.sqrt((rd64 * rd64).sum(-1, keepdims=True))
            b64 = (v64[:, None, :] * rd64).sum(-1)
            rel = (b64 * b64 - (L2 - float(r) ** 2)[:, None]) / L2[:, None]
            WORST["shadow"] = max(WORST["shadow"], float(rel.max()))
            assert rel.max() <= -SHADOW_HELD, ("shadow margin", i, rel.max())
    # ---- bits 4-5: the reflected ray of every pixel
    cosI = -dot(nrm, d)
    dr = (nrm * (F(2) * cosI)[:, None] + d).astype(F)
    for bit, prims in ((16, sc.spheres), (32, sc.lights)):
        m = (byte & bit) != 0
        if not m.any():
            continue
        a = dot(dr[m], dr[m])
        dr64 = dr[m].astype(np.float64)
        dr64 /= np.sqrt((dr64 * dr64).sum(-1, keepdims=True))
        for p in prims:
            c, r = p["origin"].astype(F), F(abs(p["radius"]))
            v = (ip[m] - c).astype(F)
            cc = (dot(v, v) - r * r).astype(F)
            b = dot(v, dr[m])
            assert (b * b - cc < 0).all() and (b * b - a * cc < 0).all(), ("a reflected bit over a ray with D >= 0", bit)
            v64 = v.astype(np.float64)
            L2 = (v64 * v64).sum(-1)
            b64 = (v64 * dr64).sum(-1)
            rel = (b64 * b64 - (L2 - float(r) ** 2)) / L2
            WORST["reflected"] = max(WORST["reflected"], float(rel.max()))
            assert rel.max() <= -REFL_HELD, ("reflected margin", bit, rel.max())
    return prim, table


FRAMES = [(64, 40), (77, 45), (100, 60), (67, 51)]
KINDS = ["floor", "wall", "both", "under", "nonunit", "transparent", "touch", "resting", "depth1", "image", "under-image"]


def make_case(rng, k):
    """case k of the fuzz: (camera, scene, depth, kind)"""
    kind = KINDS[k % len(KINDS)]
    W, H = (200, 120) if k % 40 == 7 else FRAMES[k % 4]
    o = np.array([rng.uniform(-3, 3), rng.uniform(0.6, 4.0), rng.uniform(-9, -4)])
    look = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.9, 0.05), 1.0])
    base = scene.render_map_scene()
    planes = base.planes.copy()
    if kind == "floor":
        planes = planes[:1]
    elif kind == "wall":
        planes = planes[1:]
    elif kind == "under":
        o[1] = -rng.uniform(0.5, 3.0)
    elif kind == "under-image":      # the floor seen from below: the reflected rays leave the camera's image ABOVE the floor
        o[1] = -rng.uniform(0.5, 3.0)
        look[1] = rng.uniform(0.1, 0.9)
    elif kind == "nonunit":
        planes[k % 2]["normal"] = planes[k % 2]["normal"] * F(rng.choice([1.00001, 0.99, 2.0]))
    elif kind == "transparent":
        planes[k % 2]["material"] = scene.glass()
    ns = 1 + k % 5
    s = np.zeros(ns, scene.SPHERE)
    for i in range(ns):
        r = rng.uniform(0.2, 1.0)
        s[i]["origin"] = (rng.uniform(-5, 5), r if kind == "resting" else rng.uniform(0.2, 3.0), rng.uniform(-3, 6.5))
        s[i]["radius"] = r
        s[i]["material"] = scene.glass() if i % 2 else scene.plastic()
    l = base.lights.copy()
    for i in range(3):
        l[i]["origin"] = (rng.uniform(-4, 4), rng.uniform(0.5, 4.5), rng.uniform(-3, 6.5))
        l[i]["radius"] = rng.choice([0.1, 0.3])
    if kind == "touch":      # a light and a sphere whose surfaces touch the floor inside the view
        l[0]["origin"][1] = l[0]["radius"] * F(rng.choice([1.0, 1.001, 1.02]))
        s[0]["origin"][1] = s[0]["radius"] * F(rng.choice([1.0, 0.999, 1.02]))
    if kind in ("image", "under-image"):      # small primitives next to the camera's mirror image in the floor, and in the wall
        images = [o * (1, -1, 1), np.array([o[0], o[1], 14.0 - o[2]])]
        for i in range(min(ns, 2)):
            s[i]["radius"] = rng.choice([5e-4, 0.01, 0.05])
            s[i]["origin"] = images[(k + i) % 2] + rng.normal(size=3) * rng.choice([0.01, 0.2, 1.0])
        l[0]["origin"] = images[k % 2] + rng.normal(size=3) * rng.choice([0.2, 1.0])
        l[1]["origin"] = images[(k + 1) % 2] + rng.normal(size=3) * rng.choice([0.05, 0.5])
    cam = api.perspective(tuple(o), tuple(look), float(rng.choice([40.0, 60.0, 90.0])), 1.0, W, H)
    return cam, scene.Scene(s, planes, l), (1 if kind == "depth1" else int(rng.choice([2, 4]))), kind


def test_fuzz_soundness(oracle):
    rng = np.random.default_rng(23)
    set_bits = {kind: np.zeros(6, int) for kind in KINDS}
    tiles = {kind: 0 for kind in KINDS}
    for k in range(396):
        cam, sc, depth, kind = make_case(rng, k)
        W, H = int(cam.width), int(cam.height)
        if k % 6 == 1:        # a row strip from any row
            row_offset = int(rng.integers(1, H - 17))
            rng_ = dict(rows=int(rng.integers(9, H - row_offset + 1)), row_offset=row_offset)
        elif k % 6 == 4:      # one share of interleaved 8-row bands
            stride = 2 + k % 2
            rng_ = dict(rows=(H // 8 // stride) * 8, bands=(stride, int(rng.integers(0, stride))))
        else:
            rng_ = {}
        _, table = check_bounce(oracle, cam, sc, depth=depth, **rng_)
        tiles[kind] += table.size
        for b in range(6):
            set_bits[kind][b] += int(((table >> b) & 1).sum())
    for kind in KINDS:
        print(f"{kind:12s} {tiles[kind]:6d} tiles; bits 0-5 set in", " ".join(f"{100.0 * c / tiles[kind]:5.1f}%" for c in set_bits[kind]))
    print(f"worst D / |c - p|^2 under a set bit: shadow {WORST['shadow']:.4e} (held {-SHADOW_HELD}), reflected {WORST['reflected']:.4e} (held {-REFL_HELD})")
    for kind in KINDS:
        sh = set_bits[kind] / tiles[kind]
        assert (sh[:4] > 0.02).all() and (sh[:4] < 0.98).all(), kind      # every family shows set and clear shadow bits
        if kind == "depth1":
            assert not set_bits[kind][4:].any()
        else:
            assert (sh[4:] > 0.02).all() and (sh[4:] < 0.98).all(), kind


def test_the_bounds_are_the_headers():
    import os
    import re
    h = open(os.path.join(os.path.dirname(api.__file__), "csrc", "bounce_cull_host.h")).read()
    held = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define WT_BC_(SHADOW|REFL)_HELD (\S+)", h)}
    assert held == {"SHADOW": SHADOW_HELD, "REFL": REFL_HELD}


def test_a_small_sphere_next_to_the_mirrored_camera(oracle, demo_scene):
    """a footprint far from a primitive that sits next to the virtual origin: the kernel's D is relative to |c - ip|^2, many times |c - o'|^2"""
    cam = api.perspective((0.0, 2.5, -8.0), (0.0, -0.25, 1.0), 60.0, 1.0, 640, 360)
    for c, r in (((0.004, -2.475, -7.82), 5e-4), ((0.5, -2.0, -7.5), 0.01)):
        s = np.zeros(1, scene.SPHERE)
        s[0]["origin"], s[0]["radius"], s[0]["material"] = c, r, scene.plastic()
        sc = scene.Scene(s, demo_scene.planes[:1].copy(), demo_scene.lights)
        _, t = check_bounce(oracle, cam, sc)
        print(f"sphere r = {r} at {c}: bit 4 set in {int(((t >> 4) & 1).sum())} of {t.size} tiles")
        assert (t & 15).any()


def test_the_cases_the_rule_refuses(oracle, demo_scene):
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], 200, 120)
    good = check_bounce(oracle, cam, demo_scene)[1]
    assert (good & 15).any() and (good & 48).any()
    both = api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights)
    # a tile in which the floor meets the wall carries nothing
    o, d = launch_rays(oracle, cam, 120, 0, None)
    best = first_planes(o[0].astype(F), d, demo_scene.planes)[0].reshape(120, 200)
    pad = best.reshape(15, 8, 25, 8)
    mixed = pad.min(axis=(1, 3)) != pad.max(axis=(1, 3))
    assert mixed.any() and not good[mixed].any()
    # a normal that is not unit: its tiles carry nothing; a transparent plane: no reflected bit over it; depth 1: none at all
    for j in (0, 1):
        sc = scene.Scene(demo_scene.spheres, demo_scene.planes.copy(), demo_scene.lights)
        sc.planes[j]["normal"] = sc.planes[j]["normal"] * F(1.00001)
        t = check_bounce(oracle, cam, sc)[1]
        first = (pad == j).all(axis=(1, 3))
        assert not t[first].any() and np.array_equal(t[~first & ~mixed], good[~first & ~mixed])
        sc = scene.Scene(demo_scene.spheres, demo_scene.planes.copy(), demo_scene.lights)
        sc.planes[j]["material"]["transperent"] = 1
        t = check_bounce(oracle, cam, sc)[1]
        assert not (t[first] & 48).any() and np.array_equal(t & 15, good & 15) and np.array_equal(t[~first], good[~first])
    t = check_bounce(oracle, cam, demo_scene, depth=1)[1]
    assert not (t & 48).any() and np.array_equal(t & 15, good & 15)
    # the parts
    kw = dict(depth=4)
    assert np.array_equal(api.host_bounce_cull(cam, demo_scene.spheres, demo_scene.planes, demo_scene.lights, parts=1, **kw), good & 15)
    assert np.array_equal(api.host_bounce_cull(cam, demo_scene.spheres, demo_scene.planes, demo_scene.lights, parts=2, **kw), good & 48)
    assert not api.host_bounce_cull(cam, demo_scene.spheres, demo_scene.planes, demo_scene.lights, parts=0, **kw).any()
    # terms that are not finite
    for field in ("im_corner", "origin", "up", "right"):
        c = api.clw_camera.from_buffer_copy(bytes(cam))
        getattr(c, field)[1] = np.nan
        assert not api.host_bounce_cull(c, demo_scene.spheres, demo_scene.planes, demo_scene.lights).any(), field
    for what in ("normal", "point_in_plane"):
        for bad in (np.nan, np.inf):
            sc = scene.Scene(demo_scene.spheres, demo_scene.planes.copy(), demo_scene.lights)
            sc.planes[1][what][2] = bad
            assert not api.host_bounce_cull(cam, sc.spheres, sc.planes, sc.lights).any(), (what, bad)
    sc = scene.Scene(demo_scene.spheres.copy(), demo_scene.planes, demo_scene.lights.copy())
    sc.spheres[1]["origin"][0] = np.nan
    t = api.host_bounce_cull(cam, sc.spheres, sc.planes, sc.lights)
    assert not t.any()                                      # (the primary sphere bit is gone)
    sc.spheres[1]["origin"][0] = demo_scene.spheres[1]["origin"][0]
    sc.lights[2]["radius"] = np.inf
    t = api.host_bounce_cull(cam, sc.spheres, sc.planes, sc.lights)
    assert not (t & (15 | 32)).any() and np.array_equal(t & 16, good & 16)
    # no planes: nothing; no lights: no shadow ray exists, every class is clear wherever a plane is the first hit
    assert not api.host_bounce_cull(cam, demo_scene.spheres, None, demo_scene.lights).any()
    t = api.host_bounce_cull(cam, demo_scene.spheres, demo_scene.planes, None)
    assert ((t & 15) == 15)[good != 0].all() and not (t[(both & 1) == 0]).any() and ((t & 15) == 15).sum() > ((good & 15) == 15).sum()
    with pytest.raises(ValueError):
        api.host_bounce_cull(cam, demo_scene.spheres, demo_scene.planes, demo_scene.lights, rows=16, band_stride=2, band_phase=2)


def test_demo_view_premise(demo_scene):
    """the flagship frame: the shares of skipped tests the estimate of the gain rests on (numpy model: 76 % and 92 %)"""
    cam = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], 1920, 1080)
    prim = api.host_primary_cull(cam, demo_scene.spheres, demo_scene.lights)
    t = api.host_bounce_cull(cam, demo_scene.spheres, demo_scene.planes, demo_scene.lights, depth=4)
    plane_tiles = (prim & 1) != 0
    n = int(plane_tiles.sum())
    shadow = sum(int(((t[plane_tiles] >> b) & 1).sum()) for b in range(4)) / (4.0 * n)
    refl = (4.0 * int(((t[plane_tiles] >> 4) & 1).sum()) + 3.0 * int(((t[plane_tiles] >> 5) & 1).sum())) / (7.0 * n)
    print(f"demo view 1920x1080: {t.size} tiles, {n} whose primary rays miss every sphere, {int((t != 0).sum())} with bounce bits")
    print(f"  first-hit shadow sphere tests skipped: {100 * shadow:.1f} %; per class:",
          " ".join(f"{100.0 * ((t[plane_tiles] >> b) & 1).mean():.1f}" for b in range(4)))
    print(f"  second-iteration group tests skipped: {100 * refl:.1f} % (spheres {100.0 * ((t[plane_tiles] >> 4) & 1).mean():.1f} %, "
          f"lights {100.0 * ((t[plane_tiles] >> 5) & 1).mean():.1f} %)")
    assert shadow >= 0.5, "fewer than half of the first-hit shadow sphere tests are skipped: the estimate does not hold"
    assert refl >= 0.8, "fewer than 80 % of the second iteration's group tests are skipped: the estimate does not hold"


def test_the_definition_under_the_sanitizers(tmp_path):
    """tools/bounce_cull_sanitize.c: csrc/bounce_cull_host.c built with -fsanitize=address,undefined as a stand-alone program, run as a child
    process on degenerate inputs (host code only)"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc_ = shutil.which(os.environ.get("CC") or "gcc")
    assert cc_, "no C compiler"
    csrc = os.path.join(root, "example_gui_opencl_raytracer_amd", "csrc")
    exe = str(tmp_path / "bounce_cull_sanitize")
    cmd = [cc_, "-O1", "-g", "-std=c99", "-ffp-contract=off", "-D_DEFAULT_SOURCE", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I", csrc, os.path.join(root, "tools", "bounce_cull_sanitize.c")] + \
          [os.path.join(csrc, f) for f in ("bounce_cull_host.c", "primary_cull_host.c", "host_camera.c", "scene_prep.c")] + ["-lm", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-1500:], p.stderr[-2000:])
    assert p.returncode == 0 and "0 failures" in p.stdout
