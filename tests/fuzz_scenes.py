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
