"""Supersampling (clw_ext_set_supersample), the parts that need no GPU: the two symbols, the camera identity the shim relies on
(the n*W x n*H frame of the same camera is the W x H one with w_factor / n, h_factor / n), and the resolve order as a numpy spec.

(Reading the factor back through clw_ext_get_supersample needs an initialised cl_wrap, i.e. a device: tests/test_gpu_supersample.py.)"""
import re

import numpy as np
import pytest

from conftest import CAM
from render_common import header_text, resolve

from example_gui_opencl_raytracer_amd import api


def resolve_y_first(rgb, W, H, n):
    s = np.clip(rgb.reshape(H * n, W * n, 3), np.float32(0), np.float32(1))
    k = n
    while k > 1: s = s[0::2] + s[1::2]; k //= 2
    k = n
    while k > 1: s = s[:, 0::2] + s[:, 1::2]; k //= 2
    return (s * np.float32(1.0 / (n * n))).reshape(-1, 3)


def pack1(rgb):
    """the 1-sample pack (raytracing.cl:193-194)"""
    c = (np.clip(rgb, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint32)
    return (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]


def test_header_library_and_symbol_list_agree_on_the_supersample_symbols():
    text = header_text(comments=False)
    assert re.search(r"\bvoid\s+clw_ext_set_supersample\s*\(\s*cl_wrap\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+clw_ext_get_supersample\s*\(\s*const\s+cl_wrap\s*\*\s*\w+\s*\)\s*;", text)
    L = api.load_library()
    for name in ("clw_ext_set_supersample", "clw_ext_get_supersample"):
        assert name in api.SYMBOLS and hasattr(L, name)
    assert L.clw_ext_get_supersample.restype is api.C.c_int and len(L.clw_ext_set_supersample.argtypes) == 2
    assert callable(api.ClWrap.set_supersample) and callable(api.ClWrap.get_supersample)


def test_renderer_takes_a_supersample_argument():
    import inspect
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    p = inspect.signature(Renderer.__init__).parameters["supersample"]
    assert p.default == 1 and p.kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("size", [(320, 240), (101, 75), (800, 600), (1920, 1080), (200, 152), (96, 64)])
def test_virtual_frame_camera_is_the_same_camera_with_scaled_factors(size, n):
    """rgen_perspective for n*W x n*H gives bit for bit: the same corner, origin, up, right; w_factor / n, h_factor / n."""
    W, H = size
    c1 = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], W, H)
    cn = api.perspective(CAM["origin"], CAM["look"], CAM["fov"], CAM["focal"], n * W, n * H)
    for f in ("im_corner", "origin", "up", "right"):
        assert np.array_equal(np.array(getattr(c1, f)[:], np.float32).view(np.uint32), np.array(getattr(cn, f)[:], np.float32).view(np.uint32)), f
    assert np.float32(c1.w_factor) / np.float32(n) == np.float32(cn.w_factor)
    assert np.float32(c1.h_factor) / np.float32(n) == np.float32(cn.h_factor)
    assert (cn.width, cn.height) == (n * W, n * H)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_resolve_keeps_flat_groups(n):
    """A pixel whose n x n samples are equal keeps exactly its 1-sample value (power-of-two sums are exact), clamp included."""
    rng = np.random.default_rng(n)
    W, H = 37, 21
    px = rng.uniform(-0.2, 1.3, (H, W, 3)).astype(np.float32)
    px[0, 0] = (0.0, 1.0, np.float32(1.0) - np.float32(2.0) ** -24)
    virt = np.repeat(np.repeat(px, n, 0), n, 1).reshape(-1, 3)
    packed, mean = resolve(virt, W, H, n)
    assert np.array_equal(mean, np.clip(px, np.float32(0), np.float32(1)).reshape(-1, 3))
    assert np.array_equal(packed, pack1(px).reshape(-1))


@pytest.mark.parametrize("n", [2, 4, 8])
def test_resolve_is_within_rounding_of_the_float64_mean(n):
    """Pairwise summation of N = n^2 non-negative terms: |error| <= log2(N) u S to first order, u = 2^-24, S the sum, and u S < ulp(S); the
    scaling by 1 / n^2 is exact.  So |float32 mean - float64 mean| <= log2(n^2) ulp(mean)."""
    rng = np.random.default_rng(100 + n)
    W, H = 64, 48
    virt = rng.uniform(-0.1, 1.1, (H * n * W * n, 3)).astype(np.float32)
    _, mean = resolve(virt, W, H, n)
    exact = np.clip(virt.astype(np.float64), 0, 1).reshape(H, n, W, n, 3).mean((1, 3)).reshape(-1, 3)
    ulp = np.spacing(np.maximum(mean, exact.astype(np.float32)))
    err = np.abs(mean.astype(np.float64) - exact)
    rounds = 2 * int(np.log2(n))
    print(f"n={n}: max error {float((err / ulp).max()):.3f} ulp, bound {rounds}")
    assert (err <= rounds * ulp.astype(np.float64)).all()


def test_resolve_order_is_visible():
    """x-first and y-first pair sums round differently on a constructed group: the order is part of the definition."""
    e = np.float32(2.0) ** -24      # half an ulp of 1.0
    # one 2x2 group [[a, b], [c, d]]: x first (1 + e) + (0 + e) = 1 + e -> 1 (both ties to even); y first (1 + 0) + (e + e) = 1 + 2e, exact
    a, b, c, d = np.float32(1.0), e, np.float32(0.0), e
    virt = np.array([[a] * 3, [b] * 3, [c] * 3, [d] * 3], np.float32)
    _, xf = resolve(virt, 1, 1, 2)
    yf = resolve_y_first(virt, 1, 1, 2)
    assert xf.dtype == np.float32 and yf.dtype == np.float32
    assert not np.array_equal(xf, yf), (xf, yf)
    # and on random data a fair share of the groups
    rng = np.random.default_rng(7)
    virt = rng.uniform(0, 1, (32 * 2 * 32 * 2, 3)).astype(np.float32)
    assert (resolve(virt, 32, 32, 2)[1] != resolve_y_first(virt, 32, 32, 2)).any(-1).mean() > 0.05
