"""CPU conditions of the deep scenes of tests/fuzz_scenes.py (deep_scene, DEEP_SEEDS), held with the oracle alone, so that their GPU tests in
tests/test_gpu_dispatch.py skip nothing and stay quick."""
import pytest

import fuzz_scenes as F


def test_the_seed_list_covers_every_light_count_and_both_flavour_switches():
    counts = {len(F.deep_scene(seed)[0].lights) for seed in F.DEEP_SEEDS}
    assert counts == set(F.DEEP_LIGHT_COUNTS)
    for seed, table in F.DEEP_SEEDS.items():
        assert set(table) - {32} == {5, 8, 9, 16, 17}, seed
    # stacks exactly as deep as WT_F_D8 / WT_F_D16 allow (7 / 15 parents and the current ray), and one deeper under the next flavour
    assert any(t[8] == 8 and t[9] == 9 and t[16] == 16 and t[17] == 17 for t in F.DEEP_SEEDS.values())
    assert F.DEEP_TOP_STACK >= max(t.get(32, 0) for t in F.DEEP_SEEDS.values()) and F.DEEP_TOP_STACK >= 28


def test_deep_scene_has_a_stream_of_its_own():
    a, cam_a = F.deep_scene(3)
    b, cam_b = F.deep_scene(3)
    assert a.spheres.tobytes() == b.spheres.tobytes() and a.planes.tobytes() == b.planes.tobytes() and a.lights.tobytes() == b.lights.tobytes() and cam_a == cam_b
    assert 9 <= len(a.spheres) <= 25 and len(a.planes) <= 2
    glassy = sum(int(len(F.deep_scene(s)[0].spheres["material"]["transperent"].nonzero()[0])) for s in range(40))
    total = sum(len(F.deep_scene(s)[0].spheres) for s in range(40))
    assert 0.6 < glassy / total < 0.8, glassy / total


@pytest.mark.parametrize("seed", list(F.DEEP_SEEDS))
def test_deep_scene_conditions(oracle, tex, sky, seed):
    sc, cam = F.deep_scene(seed)
    for depth, want_stack in F.DEEP_SEEDS[seed].items():
        img, _, cnt = oracle.render(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], F.DEEP_W, F.DEEP_H), sc, tex, sky, depth)
        what = (seed, depth, cnt.as_dict())
        assert cnt.int_cast_oor == 0 and cnt.oob_reads == 0, what           # the reference is defined on every pixel: the GPU test skips nothing
        assert cnt.rays <= F.DEEP_RAY_CAP, what
        assert cnt.max_stack == want_stack, what
        assert len(set(img.tolist())) > 1000, what                          # a frame, not a flat colour


def test_the_top_seed_at_depth_32(oracle, tex, sky):
    sc, cam = F.deep_scene(F.DEEP_TOP_SEED)
    _, _, cnt = oracle.render(oracle.camera(cam["origin"], cam["look"], cam["fov"], cam["focal"], F.DEEP_W, F.DEEP_H), sc, tex, sky, 32)
    assert cnt.int_cast_oor == 0 and cnt.oob_reads == 0 and cnt.rays <= F.DEEP_RAY_CAP, cnt.as_dict()
    assert cnt.max_stack == F.DEEP_TOP_STACK
