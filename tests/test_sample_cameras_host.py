"""Per-sample cameras without a GPU: the C ABI, the two host helpers that build tables (thin lens, open shutter), and -- with the
oracle alone -- that the definition the GPU tests hold the kernels to is not a trivial one."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import CAM
from example_gui_opencl_raytracer_amd import api
from render_common import declared_symbols, header_text, resolve
from sample_cameras_common import composed, rows_of, slot, virtual_camera

NEW = ["clw_ext_set_sample_cameras", "clw_ext_get_sample_cameras", "clw_ext_set_lens", "clw_host_lens_cameras", "clw_host_shutter_cameras"]
SIZES = [(320, 240), (1920, 1080), (101, 75)]
LENSES = [(0.2, 8.0), (0.05, 8.0), (0.5, 3.0), (0.01, 40.0)]


def cam_of(W, H, **over):
    return api.perspective(**dict(CAM, **over), width=W, height=H)


def f64(v):
    return np.asarray(list(v), np.float32).astype(np.float64)


# ------------------------------------------------------------------ 1. the ABI
def test_header_library_and_mirror_agree_on_the_new_symbols():
    declared = declared_symbols()
    L = api.load_library()
    for name in NEW:
        assert name in declared and name in api.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(api.clw_sample_camera) == 48
    assert re.search(r"typedef struct clw_sample_camera \{ float im_corner\[3\], origin\[3\], up\[3\], right\[3\]; \} clw_sample_camera;",
                     header_text(comments=False))
    for env in ("CLWRAP_APERTURE", "CLWRAP_FOCUS"):
        assert env in header_text()


def test_renderer_takes_a_lens_and_a_table():
    import inspect
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    assert "lens" in inspect.signature(Renderer.__init__).parameters
    assert callable(Renderer.set_sample_cameras) and callable(api.ClWrap.set_lens) and callable(api.ClWrap.get_sample_cameras)


# ------------------------------------------------------------------ 2. the lens table
@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_aperture_zero_is_the_base_camera_bit_for_bit(W, H, n):
    cam = cam_of(W, H)
    t = api.lens_cameras(cam, 0.0, 8.0, n)
    assert t.shape == (n * n, 12) and t.dtype == np.float32
    assert np.array_equal(t.view(np.uint32), np.tile(rows_of(cam).view(np.uint32), (n * n, 1)))


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("W,H", SIZES)
def test_lens_geometry(W, H, n):
    rng = np.random.default_rng(7 * n + W)
    for cam in (cam_of(W, H), cam_of(W, H, origin=(-3.0, 1.0, 2.0), look=(0.5, -0.3, -1.0), fov=60.0, focal=2.5)):
        base = rows_of(cam)
        right, up, origin = f64(cam.right), f64(cam.up), f64(cam.origin)
        centre = f64(cam.im_corner) + right * (np.float64(cam.w_factor) * W / 2) - up * (np.float64(cam.h_factor) * H / 2)
        focal = np.linalg.norm(centre)
        for aperture, focus in LENSES:
            t = api.lens_cameras(cam, aperture, focus, n)
            assert t.shape == (n * n, 12)
            assert np.array_equal(t[:, 6:].view(np.uint32), np.tile(base[6:].view(np.uint32), (n * n, 1)))       # up, right unchanged
            off = t[:, 3:6].astype(np.float64) - origin
            # in the span of right and up (an orthogonal pair), no longer than the aperture
            a, b = off @ right / (right @ right), off @ up / (up @ up)
            resid = off - np.outer(a, right) - np.outer(b, up)
            assert np.abs(resid).max() <= 1e-6 * max(1.0, np.abs(origin).max())
            assert np.linalg.norm(off, axis=1).max() <= aperture * (1 + 1e-5) + 1e-6 * np.abs(origin).max()
            assert abs(right @ up) <= 1e-6
            # every lens cell is used once: lens coordinates -> the inverse concentric map -> cell indices
            lx, ly = a / aperture, b / aperture
            r, phi = np.hypot(lx, ly), np.arctan2(ly, lx)
            phi = np.where(phi < -np.pi / 4, phi + 2 * np.pi, phi)
            sq = np.empty((n * n, 2))
            for i, (rr, ph) in enumerate(zip(r, phi)):
                if ph < np.pi / 4: sq[i] = (rr, rr * ph / (np.pi / 4))
                elif ph < 3 * np.pi / 4: sq[i] = (-rr * (ph - np.pi / 2) / (np.pi / 4), rr)
                elif ph < 5 * np.pi / 4: sq[i] = (-rr, -rr * (ph - np.pi) / (np.pi / 4))
                else: sq[i] = (rr * (ph - 3 * np.pi / 2) / (np.pi / 4), -rr)
            cells = np.floor((sq + 1) / 2 * n).astype(int)
            assert cells.min() >= 0 and cells.max() < n
            assert sorted(cells[:, 1] * n + cells[:, 0]) == list(range(n * n))
            assert [int(c[1] * n + c[0]) for c in cells] == [slot(k, n) for k in range(n * n)]
            # centred
            assert np.abs(off.mean(0)).max() <= 1e-6 * max(1.0, np.abs(origin).max())
            # focus invariance: every camera sees the points of the focal plane at the same virtual pixel position
            vx, vy = rng.integers(0, n * W, 64), rng.integers(0, n * H, 64)
            wf, hf = np.float64(np.float32(cam.w_factor) / np.float32(n)), np.float64(np.float32(cam.h_factor) / np.float32(n))
            pts = np.stack([t[k, 3:6].astype(np.float64) + (focus / focal) *
                            (t[k, 0:3].astype(np.float64) + np.outer(vx * wf, right) - np.outer(vy * hf, up)) for k in range(n * n)])
            spread = np.abs(pts - pts[0]).max()
            print(f"{W}x{H} n={n} aperture {aperture} focus {focus}: focal-plane spread {spread / focus:.2e} x focus")
            assert spread <= 1e-5 * focus
            # ... and the points of another plane at positions spread in proportion to the aperture (the table is not n*n copies)
            near = np.stack([t[k, 3:6].astype(np.float64) + (0.5 * focus / focal) * (t[k, 0:3].astype(np.float64)) for k in range(n * n)])
            assert np.abs(near - near[0]).max() >= 0.2 * aperture


def test_lens_rejects_bad_arguments():
    cam = cam_of(320, 240)
    out = np.zeros((64, 12), np.float32)
    L = api.load_library()
    call = lambda c, a, f, n: L.clw_host_lens_cameras(C.byref(c), C.c_float(a), C.c_float(f), n, out.ctypes.data_as(C.c_void_p))
    assert call(cam, 0.1, 8.0, 2) == 1
    for a, f, n in ((-0.1, 8.0, 2), (float("nan"), 8.0, 2), (float("inf"), 8.0, 2), (0.1, 0.0, 2), (0.1, -1.0, 2), (0.1, float("nan"), 2),
                    (0.1, float("inf"), 2), (0.1, 8.0, 1), (0.1, 8.0, 3), (0.1, 8.0, 16), (0.1, 8.0, 0)):
        assert call(cam, a, f, n) == 0, (a, f, n)
    assert L.clw_host_lens_cameras(None, C.c_float(0.1), C.c_float(8.0), 2, out.ctypes.data_as(C.c_void_p)) == 0
    assert L.clw_host_lens_cameras(C.byref(cam), C.c_float(0.1), C.c_float(8.0), 2, None) == 0
    with pytest.raises(ValueError):
        api.lens_cameras(cam, -1.0, 8.0, 2)


# ------------------------------------------------------------------ 3. the shutter table
@pytest.mark.parametrize("n", [2, 4, 8])
def test_shutter_table(n):
    W, H = 320, 240
    cam0 = cam_of(W, H)
    cam1 = cam_of(W, H, origin=(1.4, 2.9, -7.0), look=(0.0, -0.1, 1.0))
    same = api.shutter_cameras(cam0, cam0, n)
    assert np.array_equal(same.view(np.uint32), np.tile(rows_of(cam0).view(np.uint32), (n * n, 1)))
    t = api.shutter_cameras(cam0, cam1, n)
    a, b = rows_of(cam0), rows_of(cam1)
    assert t.shape == (n * n, 12)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert (t >= lo).all() and (t <= hi).all()
    times = np.array([(slot(k, n) + 0.5) / (n * n) for k in range(n * n)], np.float32)
    assert len(set(times.tolist())) == n * n
    want = np.where(a == b, a, a + (b - a) * times[:, None])          # float32 throughout, one rounding per operation
    assert want.dtype == np.float32 and np.array_equal(t.view(np.uint32), want.view(np.uint32))
    # the times read back from a component that moves
    moving = int(np.argmax(np.abs(b - a)))
    got = (t[:, moving].astype(np.float64) - a[moving]) / (np.float64(b[moving]) - a[moving])
    assert np.abs(got - times).max() <= 1e-5


def test_shutter_rejects_mismatched_cameras():
    cam0 = cam_of(320, 240)
    for other in (cam_of(324, 240), cam_of(320, 248), cam_of(320, 240, fov=60.0)):
        with pytest.raises(ValueError):
            api.shutter_cameras(cam0, other, 2)
    for n in (0, 1, 3, 16):
        with pytest.raises(ValueError):
            api.shutter_cameras(cam0, cam0, n)


# ------------------------------------------------------------------ 4. the definition, with the oracle alone
def test_the_definition_is_not_trivial_oracle_only(oracle, demo_scene, tex, sky):
    """aperture 0 composes to the plain supersampled oracle frame exactly; aperture 0.2 at focus 8 changes more than 10 % of the pixels."""
    from oracle.oracle_py import Camera
    W, H, n, depth = 160, 120, 2, 4
    base = cam_of(W, H)
    virt = oracle.camera(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], n * W, n * H)
    plain_p, plain_f = resolve(oracle.render(virt, demo_scene, tex, sky, depth, want_rgb=True)[1], W, H, n)

    def through(table):
        return composed(lambda k: oracle.render(virtual_camera(Camera, table[k], base, n), demo_scene, tex, sky, depth, want_rgb=True)[1], table, W, H, n)

    p0, f0 = through(api.lens_cameras(base, 0.0, 8.0, n))
    assert np.array_equal(p0, plain_p) and np.array_equal(f0.view(np.uint32), plain_f.view(np.uint32))
    p1, _ = through(api.lens_cameras(base, 0.2, 8.0, n))
    changed = float((p1 != plain_p).mean())
    print(f"aperture 0.2 focus 8, {W}x{H} n={n} depth {depth}: {100 * changed:.1f} % of the packed pixels differ from the plain supersampled frame")
    assert changed > 0.10
