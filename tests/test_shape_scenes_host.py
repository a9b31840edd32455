"""The twelve scenes of fuzz_scenes.SHAPED_SEEDS -- one per count pair of the shaped trace kernel -- held to what the GPU tests of
test_gpu_shape_modes.py rely on, with the CPU oracle alone and at the frame sizes, depths, factor and threshold those tests use.  With these
conditions met, no GPU case needs a skip or an exception for a scene: the reference is defined on every frame that is compared with it, the
moving frame differs from the static one, the refine mask has blocks of both kinds and the frames are not flat."""
import numpy as np
import pytest

from adaptive_common import refine_mask_np
from fuzz_scenes import SHAPED_SEEDS, random_scene, shaped_scene
from render_common import api  # noqa: F401  (the fixture)
from shape_common import ADAPTIVE, DEPTHS, FRAME, RAGGED, SHAPES, scene_of
from sphere_motion_common import moved_scene


SEED = 0x9E3779B1      # the seed offset of the GPU tests: it must show (soft shadows draw random points on the lights)


def oracle_frame(oracle, sc, cam, tex, sky, W, H, depth):
    return oracle.render(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H), sc, tex, sky, depth)


def conditions(oracle, api, sc, cam, disp, tex, sky):
    """-> the list of conditions this scene misses (empty = fit for the GPU tests)"""
    missed = []
    W, H = FRAME
    n, T = ADAPTIVE
    for depth in DEPTHS:
        for w, h in (FRAME, RAGGED):
            _, _, cnt = oracle_frame(oracle, sc, cam, tex, sky, w, h, depth)
            if cnt.int_cast_oor or cnt.oob_reads:
                missed.append(f"depth {depth} {w}x{h}: {cnt.int_cast_oor} casts out of range, {cnt.oob_reads} reads out of bounds")
        ends = []
        for t in (0.0, 1.0):
            p, _, cnt = oracle_frame(oracle, moved_scene(api, sc, disp, t), cam, tex, sky, W, H, depth)
            if cnt.int_cast_oor or cnt.oob_reads:
                missed.append(f"depth {depth} S({t}): undefined in the reference")
            ends.append(p)
        moved = float((ends[0] != ends[1]).mean())
        if moved < 0.01:
            missed.append(f"depth {depth}: the motion changes {100 * moved:.2f} % of the pixels")
        refined = float(refine_mask_np(ends[0], W, H, n, T).mean())
        if not 0.05 < refined < 0.95:
            missed.append(f"depth {depth}: {100 * refined:.1f} % of the blocks are refined")
        if len(np.unique(ends[0])) <= 100:
            missed.append(f"depth {depth}: {len(np.unique(ends[0]))} distinct pixel values")
        ocam = oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H)
        seeded, _ = oracle.trace_rays(oracle.raygen(ocam), sc, tex, sky, depth, id_begin=SEED)
        if np.array_equal(seeded, ends[0]):
            missed.append(f"depth {depth}: the seed offset changes no pixel")
    return missed


def test_the_table_names_every_compiled_shape():
    assert sorted(SHAPED_SEEDS) == SHAPES and len(SHAPES) == 12


@pytest.mark.parametrize("ns,npl", SHAPES)
def test_scene_meets_the_conditions_of_the_gpu_tests(oracle, api, tex, sky, ns, npl):
    sc, cam, disp = scene_of(ns, npl)
    assert sc.counts == (ns, npl, 3)
    assert disp.dtype == np.float32 and disp.shape == (ns, 3) and np.isfinite(disp).all()
    moves = (disp != 0).any(1)
    assert moves.any() and (ns < 2 or not moves.all())
    assert conditions(oracle, api, sc, cam, disp, tex, sky) == []


def test_presets_sit_on_other_sphere_indices_in_other_shapes():
    """what tells the presets apart after the draw: (transperent, dielectric, ambient) -- stone, plastic, mirror, glass"""
    kinds = {(0, 1, 0.4): "stone", (0, 0, 0.3): "plastic", (0, 1, 0.3): "mirror", (1, 1, 0.1): "glass"}
    seen = {}
    for ns, npl in SHAPES:
        m = scene_of(ns, npl)[0].spheres["material"]
        for i in range(ns):
            seen.setdefault(i, set()).add(kinds[int(m["transperent"][i]), int(m["dielectric"][i]), round(float(m["ambient"][i]), 3)])
    # every preset on every index in some shape (index 3 exists in three shapes only: three presets)
    assert all(seen[i] == set(kinds.values()) for i in range(3)) and len(seen[3]) == 3, seen


def test_lights_straddle_a_plane_in_some_scene_and_lie_on_one_side_in_another():
    """entry (light, plane) of the side table (csrc/scene_prep.c) is 0 iff the light sphere touches or straddles the plane"""
    straddling, one_side = 0, 0
    for ns, npl in SHAPES:
        sc = scene_of(ns, npl)[0]
        for p in sc.planes:
            n = p["normal"].astype(np.float64)
            d = (sc.lights["origin"].astype(np.float64) - p["point_in_plane"].astype(np.float64)) @ n / np.linalg.norm(n)
            r = sc.lights["radius"].astype(np.float64)
            straddling += int((np.abs(d) < 0.9 * r).sum())
            one_side += int((np.abs(d) > r + 1e-2).sum())
    assert straddling >= 1 and one_side >= 1, (straddling, one_side)


def test_random_scene_keeps_its_stream():
    """shaped_scene draws from a generator of its own: the seeds the existing tests name still give their counts"""
    before = [random_scene(s)[0].counts for s in (1, 11, 24, 37, 14, 16, 43, 42, 7)]
    shaped_scene(2, 1, 5)
    assert before == [(4, 2, 3), (1, 0, 3), (3, 1, 3), (1, 2, 3), (1, 3, 3), (4, 2, 4), (4, 2, 2), (0, 3, 3), (8, 2, 3)]
    assert [random_scene(s)[0].counts for s in (1, 11, 24, 37, 14, 16, 43, 42, 7)] == before
