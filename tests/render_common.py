"""Shared by every test module that renders on the GPU, and by the host tests of the same features: the `R` and `api` fixtures, the one
render driver (`rendering` + `take`), the definition of a supersampled pixel (`resolve`), the bit-for-bit comparisons, the child-process
runner of the refusal tests and the reader of the declarations of include/*.h.

A test module takes the fixtures with `from render_common import R, api  # noqa: F401`."""
import contextlib
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import CAM, ROOT


@pytest.fixture(scope="module")
def R():
    import torch  # noqa: F401  (before the shim is loaded: both then share the ROCm runtime torch ships)
    from example_gui_opencl_raytracer_amd.renderer import Renderer
    return Renderer


@pytest.fixture(scope="module")
def api():
    import torch  # noqa: F401  (before the shim is loaded: both then share the ROCm runtime torch ships)
    from example_gui_opencl_raytracer_amd import api
    return api


# ---- the render driver
@contextlib.contextmanager
def rendering(R, sc, tex, sky, W, H, *, setup=None, cam=CAM, **renderer_kw):
    """A renderer with `setup(r.w)` applied (knobs set on the wrapper), then the camera set -- a dict through `look`, a camera structure through
    `set_camera`, None = none -- and released on the way out, whatever happens inside."""
    with R(sc, tex, sky, W, H, **renderer_kw) as r:
        if setup:
            setup(r.w)
        if isinstance(cam, dict):
            r.look(**cam)
        elif cam is not None:
            r.set_camera(cam)
        yield r


@contextlib.contextmanager
def released(w):
    """`with released(api.ClWrap()) as w:` -- a bare wrapper, released on the way out"""
    try:
        yield w
    finally:
        w.release()


def queued_on(stream):
    """-> a `setup` that puts the wrapper's launches on the caller's torch stream and makes them asynchronous"""
    def setup(w):
        w.set_stream(stream.cuda_stream)
        w.set_async(True)
    return setup


def take(r, count=1, rgb=True, extra=None):
    """`count` frames in a row -> [(packed, float or None[, extra(r)]) ...]; `extra` reads what a test wants next to each frame"""
    out = []
    for _ in range(count):
        if rgb:
            p, f = r.render_rgb()
            shot = (p.copy(), f.copy())
        else:
            shot = (r.render().copy(), None)
        out.append(shot + (extra(r),) if extra else shot)
    return out


def frames(R, sc, tex, sky, W, H, depth, strict, n=1, count=1, setup=None, rgb=True, cam=CAM, **kw):
    """`count` frames in a row from one renderer -> ([(packed, float) ...], flags of the last trace launch); **kw goes to the Renderer"""
    with rendering(R, sc, tex, sky, W, H, setup=setup, cam=cam, depth=depth, strict=strict, supersample=n, **kw) as r:
        return take(r, count, rgb), r.w.last_trace_flags()


# ---- the definition of a supersampled pixel and the comparisons
def resolve(rgb, W, H, n):                      # rgb: float32 [n*H * n*W, 3], virtual-frame order
    s = np.clip(rgb.reshape(H * n, W * n, 3), np.float32(0), np.float32(1))
    k = n
    while k > 1: s = s[:, 0::2] + s[:, 1::2]; k //= 2
    k = n
    while k > 1: s = s[0::2] + s[1::2]; k //= 2
    s = s * np.float32(1.0 / (n * n))
    c = (s * np.float32(255.0)).astype(np.uint32)
    return ((c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).reshape(-1), s.reshape(-1, 3)


def same_floats(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_frames(got, want_p, want_f, what):
    """every (packed, float, ...) frame of `got` is (want_p, want_f), bit for bit; `what` names the configuration in the printed counts"""
    for k, (p, f, *_) in enumerate(got):
        bad = int((p != want_p).sum())
        print(f"{what} frame {k}: {bad} packed pixels differ, {int((f.view(np.uint32) != want_f.view(np.uint32)).any(1).sum())} float pixels differ")
        assert np.array_equal(p, want_p), (what, k, bad)
        assert same_floats(f, want_f), (what, k)


# ---- child processes (the refusal tests: message + exit(1))
def run_child(snippet, env=None, timeout=300):
    """`snippet` in a fresh interpreter, behind the imports, CAM and the demo scene `sc`, `tex`, `sky` -> the CompletedProcess"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "import torch\n"
            "from example_gui_opencl_raytracer_amd import api, scene, textures\n"
            "from example_gui_opencl_raytracer_amd.renderer import Renderer\n"
            "CAM = %r\n"
            "sc, tex, sky = scene.render_map_scene(), textures.texture_layers(), textures.skybox_cross(64)\n" % (ROOT, ROOT + "/tests", CAM)) + snippet
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- the headers
def header_text(name="hip_wrap_ext.h", comments=True):
    text = open(os.path.join(ROOT, "include", name)).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared_symbols(*headers, prefixes=("clw_ext", "clw_host")):
    """the functions the headers (default hip_wrap_ext.h) declare outside their comments"""
    pattern = r"\b((?:%s)_\w+)\s*\(" % "|".join(prefixes)
    return set().union(*(re.findall(pattern, header_text(h, comments=False)) for h in headers or ("hip_wrap_ext.h",)))
