"""Moving spheres without a GPU: the C ABI, the two host helpers that ARE the definition (sample times, the moved scene) and -- with the
oracle alone -- that the definition the GPU tests hold the kernels to is not a trivial one."""
import ctypes as C

import numpy as np
import pytest

from conftest import CAM
from example_gui_opencl_raytracer_amd import api, scene
from render_common import declared_symbols, resolve
from sample_cameras_common import composed, slot
from sphere_motion_common import DISP, field_disp, fma32, moved_scene

NEW = ["clw_ext_set_sphere_motion", "clw_ext_get_sample_times", "clw_host_sample_times", "clw_host_spheres_at"]


# ------------------------------------------------------------------ 1. the ABI
def test_header_library_and_mirror_agree_on_the_new_symbols():
    declared = declared_symbols()
    L = api.load_library()
    for name in NEW:
        assert name in declared and name in api.SYMBOLS and hasattr(L, name), name
    for name in declared:          # (tests/test_host_logic.py holds the whole header to api.SYMBOLS)
        assert hasattr(L, name), name


def test_renderer_and_wrapper_take_a_motion():
    import inspect
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    assert "motion" in inspect.signature(Renderer.__init__).parameters
    assert callable(Renderer.set_sphere_motion) and callable(api.ClWrap.set_sphere_motion) and callable(api.ClWrap.get_sample_times)
    assert callable(api.sample_times) and callable(api.spheres_at)


# ------------------------------------------------------------------ 2. the sample times
@pytest.mark.parametrize("n", [2, 4, 8])
def test_sample_times_are_the_shutters(n):
    t = api.sample_times(n)
    assert t.shape == (n * n,) and t.dtype == np.float32
    want = np.array([(slot(k, n) + 0.5) / (n * n) for k in range(n * n)], np.float32)       # exact in float32
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32))
    assert sorted(t.tolist()) == [(j + 0.5) / (n * n) for j in range(n * n)]
    # the times clw_host_shutter_cameras uses, read from the table it builds: a shutter from x = 0 to x = 1 stores a + (b - a) t = t
    W, H = 320, 240
    cam0 = api.perspective(**dict(CAM, origin=(0.0, 2.5, -8.0)), width=W, height=H)
    cam1 = api.perspective(**dict(CAM, origin=(1.0, 2.5, -8.0)), width=W, height=H)
    table = api.shutter_cameras(cam0, cam1, n)
    assert np.array_equal(table[:, 3].view(np.uint32), t.view(np.uint32))


def test_sample_times_reject_other_factors():
    out = np.zeros(256, np.float32)
    L = api.load_library()
    for n in (0, 1, 3, 5, 16):
        assert L.clw_host_sample_times(n, out.ctypes.data_as(C.c_void_p)) == 0
        with pytest.raises(ValueError):
            api.sample_times(n)
    assert L.clw_host_sample_times(2, None) == 0


# ------------------------------------------------------------------ 3. the moved scene
@pytest.mark.parametrize("which", ["demo", "field"])
def test_spheres_at_is_one_fma_per_component_and_touches_nothing_else(which, demo_scene):
    rng = np.random.default_rng(11)
    if which == "demo":
        sc, disp = demo_scene, DISP
    else:
        sc = scene.dielectric_field_scene()
        disp = (field_disp(len(sc.spheres)) + rng.normal(0, 0.3, (len(sc.spheres), 3))).astype(np.float32)
    raw = sc.spheres.copy()
    pad = raw.view(np.uint8).reshape(len(raw), 96)
    pad[:, 12:16] = rng.integers(0, 256, (len(raw), 4))          # padding bytes that are NOT zero: they must travel as they are
    pad[:, 20:32] = rng.integers(0, 256, (len(raw), 12))
    before = pad.tobytes()                                          # (byte views throughout: numpy does not keep padding when it copies records)
    times = list(api.sample_times(8)) + [0.0, 1.0, -0.75, 3.1415927, 1e-3, 0.3333333]
    for t in times:
        got = api.spheres_at(raw, disp, float(t))
        assert pad.tobytes() == before                              # the input is not written
        assert got.dtype == raw.dtype and got.shape == raw.shape
        g = got.view(np.uint8).reshape(len(raw), 96)
        want = pad.copy()
        want[:, :12] = fma32(np.float32(t), disp, raw["origin"]).view(np.uint8)
        assert g.tobytes() == want.tobytes(), t
        assert np.array_equal(g[:, 12:], pad[:, 12:])               # radius, material, padding: every byte
    # ... a centre really moves by t * d (to rounding), and only where d is not zero
    got = api.spheres_at(raw, disp, 0.5)
    assert np.abs(got["origin"].astype(np.float64) - (raw["origin"].astype(np.float64) + 0.5 * disp.astype(np.float64))).max() <= 1e-6
    still = ~disp.any(1)
    assert np.array_equal(got["origin"][still].view(np.uint32), raw["origin"][still].view(np.uint32))
    assert (got["origin"][~still] != raw["origin"][~still]).any(1).all()


def test_fma_restatement_rounds_once():
    """the numpy restatement against cases where a * b + c with two roundings differs from the fused result"""
    a = np.float32(1 + 2.0 ** -12)
    assert fma32(a, a, np.float32(-1.0)) == np.float32(2.0 ** -11 + 2.0 ** -24)          # the product's low bits survive
    assert np.float32(a * a) + np.float32(-1.0) != fma32(a, a, np.float32(-1.0))
    rng = np.random.default_rng(5)
    t, d, c = (rng.normal(0, 1, 100000).astype(np.float32) for _ in range(3))
    import fractions
    got = fma32(t, d, c)
    for i in range(0, 100000, 997):                                  # exact rational arithmetic, rounded once through float64 only when it is safe
        exact = fractions.Fraction(float(t[i])) * fractions.Fraction(float(d[i])) + fractions.Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(exact - fractions.Fraction(float(got[i]))) <= min(abs(exact - fractions.Fraction(float(lo))), abs(exact - fractions.Fraction(float(hi))))


def test_spheres_at_with_no_displacement_or_time_zero_is_the_input(demo_scene):
    raw = demo_scene.spheres
    for t in (0.0, 0.5, 1.0, -2.0):
        assert api.spheres_at(raw, np.zeros_like(DISP), t).tobytes() == raw.tobytes()
    assert api.spheres_at(raw, DISP, 0.0).tobytes() == raw.tobytes()
    # in place, and the empty scene
    L = api.load_library()
    buf = raw.copy()
    assert L.clw_host_spheres_at(buf.ctypes.data_as(C.c_void_p), len(buf), DISP.ctypes.data_as(C.c_void_p), C.c_float(0.25), buf.ctypes.data_as(C.c_void_p)) == 1
    assert buf.tobytes() == api.spheres_at(raw, DISP, 0.25).tobytes()
    assert L.clw_host_spheres_at(None, 0, None, C.c_float(0.25), None) == 1
    assert L.clw_host_spheres_at(None, 4, DISP.ctypes.data_as(C.c_void_p), C.c_float(0.25), buf.ctypes.data_as(C.c_void_p)) == 0
    assert L.clw_host_spheres_at(buf.ctypes.data_as(C.c_void_p), 4, None, C.c_float(0.25), buf.ctypes.data_as(C.c_void_p)) == 0


# ------------------------------------------------------------------ 4. the definition, with the oracle alone
def test_the_definition_is_not_trivial_oracle_only(oracle, demo_scene, tex, sky):
    """A zero displacement composes to the plain supersampled oracle frame exactly; the tests' displacement changes the frame, where the moving
    spheres are and nowhere far from them."""
    W, H, n, depth = 160, 120, 2, 4
    virt = oracle.camera(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], n * W, n * H)
    plain_p, plain_f = resolve(oracle.render(virt, demo_scene, tex, sky, depth, want_rgb=True)[1], W, H, n)
    times = api.sample_times(n)

    def through(disp):
        return composed(lambda k: oracle.render(virt, moved_scene(api, demo_scene, disp, float(times[k])), tex, sky, depth, want_rgb=True)[1], times, W, H, n)

    p0, f0 = through(np.zeros_like(DISP))
    assert np.array_equal(p0, plain_p) and np.array_equal(f0.view(np.uint32), plain_f.view(np.uint32))
    p1, _ = through(DISP)
    changed = (p1 != plain_p).reshape(H, W)
    print(f"displacement of the tests, {W}x{H} n={n} depth {depth}: {100 * float(changed.mean()):.1f} % of the packed pixels differ from the static supersampled frame")
    assert 0.01 < changed.mean() < 0.6
    assert not changed[:H // 8].any()              # the sky at the top of the frame stands still
