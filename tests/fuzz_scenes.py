"""Seeded random scenes shared by the CPU (oracle vs reference kernels) and GPU (HIP vs oracle) fuzz tests."""
import numpy as np

from example_gui_opencl_raytracer_amd import scene as S


def random_scene(seed: int):
    rng = np.random.default_rng(seed)
    ns, npl, nl = int(rng.integers(0, 9)), int(rng.integers(0, 4)), int(rng.integers(0, 5))
    presets = [S.stone, S.plastic, S.mirror, S.glass]
    sph = np.zeros(ns, S.SPHERE)
    for i in range(ns):
        sph[i]["origin"] = rng.uniform([-4, 0.2, -2], [5, 3, 7])
        sph[i]["radius"] = rng.uniform(0.2, 1.2)
        m = presets[int(rng.integers(0, 4))]()
        m["rgb"] = rng.uniform(0, 1, 3)
        m["shininess"] = int(rng.integers(0, 200))
        m["reflectivity"] = rng.choice([0.0, 0.04, 0.1, 0.5, 1.0])
        m["n"] = rng.choice([1.0, 1.33, 1.52, 2.4])
        m["texture_id"] = -1
        sph[i]["material"] = m
    pln = np.zeros(npl, S.PLANE)
    for i in range(npl):
        n = rng.normal(size=3) if i else np.array([0.0, 1.0, 0.0])
        n = (n / np.linalg.norm(n)).astype(np.float32)
        pln[i]["normal"] = n
        pln[i]["point_in_plane"] = (0, 0, 0) if i == 0 else (n * -rng.uniform(4, 9)).astype(np.float32)
        m = presets[int(rng.integers(0, 3))]()
        m["rgb"] = rng.uniform(0, 1, 3)
        m["texture_id"] = int(rng.integers(-1, 4))
        m["texture_scale"] = rng.choice([1.0, 17.5, 100.0])
        pln[i]["material"] = m
    lgt = np.zeros(nl, S.LIGHT)
    for i in range(nl):
        lgt[i]["origin"] = rng.uniform([-4, 1.5, -3], [4, 6, 6])
        lgt[i]["radius"] = rng.uniform(0.05, 0.4)
        lgt[i]["intensity"] = rng.uniform(3, 40)
        lgt[i]["rgb"] = rng.uniform(0, 1, 3)
    cam = dict(origin=tuple(rng.uniform([-3, 0.5, -9], [3, 4, -4]).astype(np.float32).tolist()),
               look=tuple(rng.uniform([-0.4, -0.4, 0.8], [0.4, 0.2, 1.0]).astype(np.float32).tolist()),
               fov=float(rng.choice([60.0, 90.0, 110.0])), focal=1.0)
    depth = int(rng.choice([1, 2, 3, 4, 8, 15]))
    return S.Scene(sph, pln, lgt), cam, depth


# ---- one scene per count pair the shaped trace kernel is compiled for (wt_shape in csrc/whitted_trace.inc: 1..4 spheres, 0..2 planes, 3 lights)
SHAPED_CAM_BOX = ([-1.5, 1.0, -5.5], [1.5, 3.0, -3.5])        # closer than random_scene's camera: a sphere covers a few per cent of a 72 x 48 frame
SHAPED_SPHERE_BOX = ([-2.5, 0.3, -1.0], [2.5, 2.2, 3.0])
# (spheres, planes) -> seed.  tests/test_shape_scenes_host.py holds every one of these scenes to the conditions the GPU tests of
# tests/test_gpu_shape_modes.py rely on (defined reference, visible motion, a refine mask with both kinds of block, a frame that is not flat).
SHAPED_SEEDS = {
    (1, 0): 2, (1, 1): 1, (1, 2): 3,
    (2, 0): 4, (2, 1): 0, (2, 2): 0,
    (3, 0): 4, (3, 1): 0, (3, 2): 0,
    (4, 0): 1, (4, 1): 0, (4, 2): 1,
}


def sphere_displacement(rng, ns, first=0):
    """float32 [ns, 3]: sphere `first mod ns` moves by a few tenths of a unit, the next one (ns >= 2) stands still, the others by the coin"""
    disp = np.zeros((ns, 3), np.float32)
    for i in range(ns):
        k = (i - first) % ns
        d = rng.uniform(-0.6, 0.6, 3)
        coin = rng.random() < 0.5
        if k == 0 or (k > 1 and coin):
            disp[i] = d
    return disp


def shaped_scene(ns: int, npl: int, seed: int):
    """-> (scene, camera, displacement): exactly `ns` spheres, `npl` planes and 3 lights, with a stream of its own (random_scene's is untouched).
    Materials, radii and lights are drawn as random_scene draws them, but sphere i starts from preset (i + shape number) mod 4, so that stone,
    plastic, mirror and glass sit on other sphere indices in every shape; with planes and an even sphere count, light 0 is put onto the last
    plane, which it then straddles (entry 0 of the light / plane side table), while the floor keeps every other light on one side."""
    assert 1 <= ns and 0 <= npl
    rng = np.random.default_rng([ns, npl, seed])
    shape = (ns - 1) * 3 + npl
    presets = [S.stone, S.plastic, S.mirror, S.glass]
    sph = np.zeros(ns, S.SPHERE)
    for i in range(ns):
        sph[i]["origin"] = rng.uniform(*SHAPED_SPHERE_BOX)
        sph[i]["radius"] = rng.uniform(0.2, 1.2)
        m = presets[(i + shape) % 4]()
        m["rgb"] = rng.uniform(0, 1, 3)
        m["shininess"] = int(rng.integers(0, 200))
        m["reflectivity"] = rng.choice([0.0, 0.04, 0.1, 0.5, 1.0])
        m["n"] = rng.choice([1.0, 1.33, 1.52, 2.4])
        m["texture_id"] = -1
        sph[i]["material"] = m
    pln = np.zeros(npl, S.PLANE)
    for i in range(npl):
        n = rng.normal(size=3) if i else np.array([0.0, 1.0, 0.0])
        n = (n / np.linalg.norm(n)).astype(np.float32)
        pln[i]["normal"] = n
        pln[i]["point_in_plane"] = (0, 0, 0) if i == 0 else (n * -rng.uniform(4, 9)).astype(np.float32)
        m = presets[int(rng.integers(0, 3))]()
        m["rgb"] = rng.uniform(0, 1, 3)
        m["texture_id"] = int(rng.integers(-1, 4))
        m["texture_scale"] = rng.choice([1.0, 17.5, 100.0])
        pln[i]["material"] = m
    lgt = np.zeros(3, S.LIGHT)
    for i in range(3):
        lgt[i]["origin"] = rng.uniform([-4, 1.5, -3], [4, 6, 6])
        lgt[i]["radius"] = rng.uniform(0.05, 0.4)
        lgt[i]["intensity"] = rng.uniform(3, 40)
        lgt[i]["rgb"] = rng.uniform(0, 1, 3)
    if npl and ns % 2 == 0:
        n, p, o = pln[npl - 1]["normal"].astype(np.float64), pln[npl - 1]["point_in_plane"].astype(np.float64), lgt[0]["origin"].astype(np.float64)
        lgt[0]["origin"] = o - (np.dot(n, o - p) - 0.5 * float(lgt[0]["radius"])) * n        # the centre half a radius above the plane
    cam = dict(origin=tuple(rng.uniform(*SHAPED_CAM_BOX).astype(np.float32).tolist()),
               look=tuple(rng.uniform([-0.2, -0.3, 0.9], [0.2, 0.0, 1.0]).astype(np.float32).tolist()),
               fov=float(rng.choice([60.0, 90.0])), focal=1.0)
    return S.Scene(sph, pln, lgt), cam, sphere_displacement(rng, ns, first=shape)


# ---- deep scenes: refraction trees that fill the DFS stack, with every light count the tail's node layout distinguishes
DEEP_LIGHT_COUNTS = (0, 1, 2, 3, 4, 7)
DEEP_W, DEEP_H = 64, 48
DEEP_RAY_CAP = 10_000_000
# seed -> {depth: the deepest DFS stack the CPU oracle reaches at DEEP_W x DEEP_H (the current ray counts)}.  The depths of a seed are the ones its
# GPU test runs: 5, both sides of the two flavour switches (8 | 9, 16 | 17), and 32 where that stays under DEEP_RAY_CAP rays.  Seeds 12, 1 and 2
# fill the stack of every depth to the last entry.  tests/test_deep_scenes_host.py re-derives the table and
# holds every frame to: no undefined float -> int cast or read in the reference, at most DEEP_RAY_CAP rays.
DEEP_SEEDS = {
    12: {5: 5, 8: 8, 9: 9, 16: 16, 17: 17},              # 0 lights
    1: {5: 5, 8: 8, 9: 9, 16: 16, 17: 17},               # 1
    2: {5: 5, 8: 8, 9: 9, 16: 16, 17: 17},               # 2
    15: {5: 5, 8: 8, 9: 9, 16: 15, 17: 16},              # 3
    16: {5: 5, 8: 8, 9: 8, 16: 13, 17: 14, 32: 25},      # 4
    17: {5: 5, 8: 8, 9: 9, 16: 14, 17: 15},              # 7
    24: {5: 5, 8: 7, 9: 8, 16: 14, 17: 15},              # 0
}
# the deepest stack at depth 32 under the ray cap among seeds 0..33: 28 of the 32 entries, 1.6 M rays -- 660 000 of them one pixel's, a serial chain
# that took an MI355X 2.5 s per launch in every mode, so this seed runs at depth 32 in one test of its own and not in the five modes of the others
# (of the listed seeds only 16 and 24 stay under the ray cap at depth 32)
DEEP_TOP_SEED, DEEP_TOP_STACK = 24, 28


def deep_scene(seed: int):
    """-> (scene, camera): a g x g field (g = 3..5) of touching spheres on the floor level in front of a close camera, with a stream of its own
    (random_scene's is untouched).  About 70 % of the spheres are dielectric, their n and reflectivity drawn from random_scene's choices, the
    rest stone, plastic or mirror; 0 to 2 planes; DEEP_LIGHT_COUNTS[seed mod 6] lights."""
    rng = np.random.default_rng([0xDEE9, seed])
    g = int(rng.integers(3, 6))
    pitch = float(rng.uniform(0.8, 1.2))
    sph = np.zeros(g * g, S.SPHERE)
    others = [S.stone, S.plastic, S.mirror]
    for i in range(g * g):
        ix, iz = i % g, i // g
        sph[i]["origin"] = ((ix - (g - 1) / 2) * pitch, pitch / 2, iz * pitch)
        sph[i]["radius"] = pitch / 2
        if rng.random() < 0.7:
            m = S.glass()
            m["n"] = rng.choice([1.0, 1.33, 1.52, 2.4])
            m["reflectivity"] = rng.choice([0.0, 0.04, 0.1, 0.5, 1.0])
        else:
            m = others[int(rng.integers(0, 3))]()
            m["shininess"] = int(rng.integers(0, 200))
        m["rgb"] = rng.uniform(0, 1, 3)
        m["texture_id"] = -1
        sph[i]["material"] = m
    npl = int(rng.integers(0, 3))
    pln = np.zeros(npl, S.PLANE)
    for i in range(npl):
        n = np.array([0.0, 1.0, 0.0]) if i == 0 else np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), -1.0])
        n = (n / np.linalg.norm(n)).astype(np.float32)
        pln[i]["normal"] = n
        pln[i]["point_in_plane"] = (0, 0, 0) if i == 0 else (0, 0, g * pitch + rng.uniform(0.5, 2.0))
        m = [S.stone, S.plastic, S.mirror][int(rng.integers(0, 3))]()
        m["rgb"] = rng.uniform(0, 1, 3)
        m["texture_id"] = int(rng.integers(-1, 4))
        m["texture_scale"] = rng.choice([1.0, 17.5, 100.0])
        pln[i]["material"] = m
    nl = DEEP_LIGHT_COUNTS[seed % len(DEEP_LIGHT_COUNTS)]
    lgt = np.zeros(nl, S.LIGHT)
    for i in range(nl):
        lgt[i]["origin"] = rng.uniform([-3, 1.5, -2], [3, 5, g * pitch])
        lgt[i]["radius"] = rng.uniform(0.05, 0.3)
        lgt[i]["intensity"] = rng.uniform(3, 40)
        lgt[i]["rgb"] = rng.uniform(0, 1, 3)
    cam = dict(origin=(float(np.float32(rng.uniform(-0.5, 0.5))), float(np.float32(rng.uniform(0.4, 1.4) * pitch)), float(np.float32(-rng.uniform(1.2, 2.2) * pitch))),
               look=(float(np.float32(rng.uniform(-0.1, 0.1))), float(np.float32(rng.uniform(-0.35, -0.05))), 1.0), fov=90.0, focal=1.0)
    return S.Scene(sph, pln, lgt), cam


# ---- grid layouts: scenes of more than 256 spheres whose uniform grid (csrc/scene_prep.c) and both of its shadow walks decide something
GRID_LAYOUTS = ("cloud", "giants", "coincident", "touching", "tower", "offset")
GRID_3D = ("cloud", "giants", "tower", "offset")          # layouts whose grid has more than one cell on every axis
GRID_OFFSET = (4000.0, 4000.0, 4000.0)
GLASS_FIELDS = ("ambient", "diffuse", "specular", "shininess", "transperent", "dielectric", "n", "reflectivity")


def _plastic_spheres(n):
    return S.sphere_grid_scene(n, 1).spheres.copy()          # n plastic spheres with hashed colours: the geometry is overwritten


def _glass(sp, sel):
    g = S.glass()
    for name in GLASS_FIELDS:
        sp["material"][name][sel] = g[name]


def _cam(origin, look, fov):
    return dict(origin=tuple(float(np.float32(x)) for x in origin), look=tuple(float(x) for x in look), fov=float(fov), focal=1.0)


def grid_layout(name: str, lights: str = "small"):
    """-> (scene, [camera outside the sphere set, camera inside it]).  Every layout keeps the demo floor plane and three lights.
    lights "small": radii <= 0.1, a fraction of a cell (the grid pairs the two samples of a light in one walk); "large": light 0 has radius
    1.5 and sits INSIDE the sphere set (more than 0.3 of a cell: every shadow ray walks on its own).  Every sphere lies within 40 units of
    every camera and light, the cameras see the floor beyond 300 units in at most one pixel row, and radii are >= 0.05: inside the domain where the float sphere test still decides.
      cloud       600 spheres scattered in a box, radii 0.12 .. 1.2, a third glass (test_gpu_parity's cloud, seed 1)
      giants      400 spheres of r 0.05 .. 0.15 in a box and three of r 6, 8 and 10 (opaque, glass, glass) around its middle: listed in
                  (nearly) every cell, a glass one crossed over a dozen consecutive cells; the inside camera sits in both glass giants
      coincident  300 spheres on ONE centre, radii 0.5 .. 0.9 in steps of 1 / 64 (equal-t ties), even indices opaque (r <= 0.7) and odd ones
                  glass, and 10 elsewhere: long cell lists, every glass shell counted once; the inside camera sits between the shells
      touching    r 0.5 at pitch 1, 14 x 2 x 14: tangent spheres; the inside camera sits in a void of the lattice
      tower       a column 3 x 66 x 3 of r 0.3 at pitch 1 (the tallest that keeps its ends within 40 units of a camera and light at
                  mid-height): res[1] far above res[0] and res[2]; the inside camera looks up the column
      offset      cloud moved by GRID_OFFSET -- cameras, lights and the floor with it
    The floor matters: a shadow ray starts at its hit point, and a floor point thousands of units from the spheres is as far outside that
    domain as a camera there (the linear scan then "hits" spheres whose padded boxes the ray misses, by rounding alone).  So the floor
    moves with `offset`, and the tower's outside camera looks down at the column instead of at the horizon behind it."""
    assert name in GRID_LAYOUTS and lights in ("small", "large")
    base = S.render_map_scene()
    planes, li = base.planes[:1].copy(), base.lights.copy()
    li["radius"] = (0.1, 0.08, 0.1)
    shift = np.zeros(3, np.float32)
    if name in ("cloud", "offset"):
        rng = np.random.default_rng(1)
        sp = S.sphere_grid_scene(25, 24).spheres.copy()
        n = len(sp)
        sp["origin"][:, 0] = rng.uniform(-9.0, 9.0, n).astype(np.float32)
        sp["origin"][:, 1] = rng.uniform(0.2, 7.0, n).astype(np.float32)
        sp["origin"][:, 2] = rng.uniform(2.0, 20.0, n).astype(np.float32)
        sp["radius"] = (0.12 * 10.0 ** rng.uniform(0.0, 1.0, n)).astype(np.float32)
        _glass(sp, rng.random(n) < 0.33)
        li["origin"] = [(0.0, 3.5, 11.0), (-4.0, 1.5, 6.0), (3.0, 9.0, 4.0)]
        big = (-3.0, 4.0, 14.0)
        cams = [_cam((0.0, 4.0, -6.0), (0.0, -0.1, 1.0), 80.0), _cam((1.0, 3.0, 10.0), (-0.3, 0.1, 1.0), 100.0)]
        if name == "offset":
            shift = np.asarray(GRID_OFFSET, np.float32)
    elif name == "giants":
        rng = np.random.default_rng(0x61A27)
        n = 400
        sp = _plastic_spheres(n + 3)
        sp["origin"][:n] = rng.uniform([-8.0, 0.3, 2.0], [8.0, 12.0, 18.0], (n, 3)).astype(np.float32)
        sp["radius"][:n] = rng.uniform(0.05, 0.15, n).astype(np.float32)
        sel = np.zeros(n + 3, bool)
        sel[:n] = rng.random(n) < 0.33
        sp["origin"][n:] = [(0.0, 6.0, 10.0), (1.5, 6.0, 9.0), (-1.0, 7.0, 11.0)]
        sp["radius"][n:] = (6.0, 8.0, 10.0)
        sel[n + 1:] = True
        _glass(sp, sel)
        li["origin"] = [(0.5, 6.5, 2.5), (-6.0, 9.0, 5.0), (7.5, 3.0, 16.0)]      # in both glass giants; in the r 10 one; in none
        big = (-3.0, 5.0, 4.0)
        cams = [_cam((0.0, 6.0, -16.0), (0.0, 0.0, 1.0), 80.0), _cam((0.0, 6.0, 3.0), (0.6, -0.1, 1.0), 100.0)]
    elif name == "coincident":
        rng = np.random.default_rng(0xC01C)
        n = 300
        sp = _plastic_spheres(n + 10)
        sp["origin"][:n] = (0.0, 2.0, 8.0)
        r = np.where(np.arange(n) % 2 == 0, rng.uniform(0.5, 0.7, n), rng.uniform(0.5, 0.9, n))
        sp["radius"][:n] = (np.round(r * 64.0) / 64.0).astype(np.float32)
        sp["origin"][n:] = rng.uniform([-6.0, 0.5, 3.0], [6.0, 5.0, 14.0], (10, 3)).astype(np.float32)
        sp["radius"][n:] = rng.uniform(0.3, 0.6, 10).astype(np.float32)
        sel = np.zeros(n + 10, bool)
        sel[1:n:2] = True
        _glass(sp, sel)
        li["origin"] = [(-2.5, 4.5, 6.0), (2.0, 1.0, 5.0), (0.5, 5.0, 11.0)]
        big = (-2.0, 2.5, 9.5)
        cams = [_cam((0.0, 2.5, 4.5), (0.0, -0.1, 1.0), 70.0), _cam((0.8, 2.0, 8.0), (-1.0, 0.05, 0.3), 100.0)]
    elif name == "touching":
        rng = np.random.default_rng(0x70C4)
        n = 14 * 2 * 14
        sp = _plastic_spheres(n)
        k = np.arange(n)
        sp["origin"][:, 0] = (k % 14).astype(np.float32) - np.float32(6.5)
        sp["origin"][:, 1] = ((k // 14) % 2).astype(np.float32) + np.float32(0.5)
        sp["origin"][:, 2] = (k // 28).astype(np.float32) + np.float32(2.0)
        sp["radius"] = 0.5
        _glass(sp, rng.random(n) < 0.33)
        li["origin"] = [(0.0, 4.0, 8.0), (-3.0, 3.0, 5.0), (2.0, 1.0, 6.5)]         # the last one in a void of the lattice
        big = (3.0, 1.0, 10.5)
        cams = [_cam((0.0, 5.0, -4.0), (0.0, -0.4, 1.0), 80.0), _cam((0.0, 1.0, 8.5), (1.0, 0.1, 0.3), 100.0)]
    else:
        rng = np.random.default_rng(0x703E)
        n = 3 * 66 * 3
        sp = _plastic_spheres(n)
        k = np.arange(n)
        sp["origin"][:, 0] = (k % 3).astype(np.float32) - np.float32(1.0)
        sp["origin"][:, 1] = (k // 9).astype(np.float32) + np.float32(0.5)
        sp["origin"][:, 2] = ((k // 3) % 3).astype(np.float32) + np.float32(5.0)
        sp["radius"] = 0.3
        _glass(sp, rng.random(n) < 0.33)
        li["origin"] = [(-0.5, 30.0, 6.5), (3.0, 36.0, 3.0), (0.5, 34.0, 5.5)]
        big = (0.5, 38.0, 6.5)
        cams = [_cam((-9.0, 38.0, 6.0), (1.0, -1.0, 0.0), 60.0), _cam((-0.5, 33.0, 5.5), (0.2, 1.0, 0.3), 100.0)]
    if lights == "large":
        li["origin"][0] = big
        li["radius"][0] = 1.5
    sp["origin"] += shift
    li["origin"] += shift
    planes["point_in_plane"] += shift
    cams = [dict(c, origin=tuple(float(x) for x in (np.asarray(c["origin"], np.float32) + shift))) for c in cams]
    return S.Scene(sp, planes, li), cams
