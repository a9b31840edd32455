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
