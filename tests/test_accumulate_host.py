"""Progressive frame accumulation, the host side (no GPU): clw_host_frame_seed and clw_host_jitter_camera against the numpy restatement of
accumulate_common.py, the fold itself, and the new symbols."""
import ctypes as C

import numpy as np
import pytest

from accumulate_common import F32, camera_bytes, camera_rows, fold, frame_seed, halton, jittered, pack
from conftest import CAM
from render_common import api, header_text  # noqa: F401  (api: the fixture)

NEW_SYMBOLS = ["clw_ext_set_seed_offset", "clw_ext_get_seed_offset", "clw_ext_set_accumulate", "clw_ext_get_accumulated",
               "clw_ext_reset_accumulation", "clw_host_frame_seed", "clw_host_jitter_camera"]


@pytest.fixture(scope="module")
def cam(api):
    return api.perspective(CAM["origin"], CAM["look"], 90.0, 1.0, 101, 75)


def test_frame_seed(api):
    assert api.frame_seed(0) == 0
    seeds = np.array([api.frame_seed(f) for f in range(65536)], np.uint64)
    assert len(np.unique(seeds)) == 65536
    want = (np.arange(65536, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    assert np.array_equal(seeds, want)
    assert all(api.frame_seed(f) == frame_seed(f) for f in (1, 2, 65535, 65536, 0xFFFFFFFF))


def test_jitter_frame_0_is_the_base_camera(api, cam):
    for n in (1, 2, 4, 8):
        assert bytes(api.jitter_camera(cam, 0, n)) == bytes(cam)


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_jitter_equals_the_numpy_restatement(api, cam, n):
    for f in range(1, 65):
        got, want = api.jitter_camera(cam, f, n), jittered(cam, f, n)
        assert camera_bytes(got) == camera_bytes(want), (f, n)
        assert bytes(got)[12:] == bytes(cam)[12:]                   # everything but im_corner is copied
        assert bytes(got)[:12] != bytes(cam)[:12]


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_every_offset_is_within_half_a_cell(api, cam, n):
    corner, _, up, right = (v.astype(np.float64) for v in camera_rows(cam))
    for f in range(1, 65):
        jx, jy = halton(f)
        assert -0.5 <= jx < 0.5 and -0.5 <= jy < 0.5
        d = np.array(list(api.jitter_camera(cam, f, n).im_corner), np.float64) - corner
        # right and up are orthogonal: the offset's components along them, in cells of a sample
        cx = d @ right / (right @ right) / (cam.w_factor / n)
        cy = -(d @ up) / (up @ up) / (cam.h_factor / n)
        assert abs(cx) <= 0.5 + 1e-3 and abs(cy) <= 0.5 + 1e-3, (f, n, cx, cy)
        assert abs(cx - float(jx)) < 1e-3 and abs(cy - float(jy)) < 1e-3      # (float32 rounding of a corner of magnitude ~1 in cells of ~0.01)


def test_halton_points(api):
    assert [float(halton(f)[0]) for f in (1, 2, 3, 4)] == [0.0, -0.25, 0.25, -0.375]
    assert np.allclose([float(halton(f)[1]) for f in (1, 2, 3)], [1 / 3 - 0.5, 2 / 3 - 0.5, 1 / 9 - 0.5], atol=1e-7)


def test_jitter_rejects_bad_arguments(api, cam):
    L = api.load_library()
    out = api.clw_camera()
    for n in (0, 3, 5, 16):
        assert L.clw_host_jitter_camera(C.byref(cam), 1, n, C.byref(out)) == 0
        with pytest.raises(ValueError):
            api.jitter_camera(cam, 1, n)
    assert L.clw_host_jitter_camera(None, 1, 1, C.byref(out)) == 0
    assert L.clw_host_jitter_camera(C.byref(cam), 1, 1, None) == 0
    assert L.clw_host_jitter_camera(C.byref(cam), 1, 1, C.byref(out)) == 1


def test_fold_of_one_frame_is_the_plain_pack():
    rng = np.random.default_rng(7)
    c = rng.uniform(-0.2, 1.3, (4096, 3)).astype(F32)
    p, mean = fold([c])
    clamped = np.clip(c, F32(0), F32(1))
    assert np.array_equal(mean, clamped) and np.array_equal(p, pack(clamped))
    # and of several: sequential float32 sums, one multiplication by the rounded reciprocal
    cs = [rng.uniform(0, 1, (257, 3)).astype(F32) for _ in range(3)]
    p3, m3 = fold(cs)
    want = np.minimum(((cs[0] + cs[1]) + cs[2]) * (F32(1) / F32(3)), F32(1))
    assert m3.dtype == np.float32 and np.array_equal(m3, want) and np.array_equal(p3, pack(want))


def test_new_symbols_are_exported_and_listed(api):
    L = api.load_library()
    header = header_text()
    for name in NEW_SYMBOLS:
        assert name in api.SYMBOLS, name
        assert hasattr(L, name), name
        assert name + "(" in header, name
