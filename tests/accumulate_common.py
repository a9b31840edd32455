"""Shared by test_accumulate_host.py and test_gpu_accumulate.py: the numpy restatement of progressive frame accumulation
(include/hip_wrap_ext.h, clw_ext_set_accumulate).

Frame K-1 of an accumulated view is `fold` of K constituent frames c_0 .. c_{K-1}: per output pixel and channel the values the plain launch
would pack (clamped to [0, 1]), added one after the other in float32, times float32(1 / K), capped at 1, packed with (unsigned)(v * 255).
Constituent frame f is the plain frame with seed offset `frame_seed(f)` through the camera `jittered(cam, f, n)`."""
import numpy as np

from conftest import CAM
from render_common import rendering, take

F32 = np.float32
GOLDEN_RATIO_ODD = 0x9E3779B1


def frame_seed(f):
    return (int(f) * GOLDEN_RATIO_ODD) & 0xFFFFFFFF


def pack(v):
    c = (np.asarray(v, F32) * F32(255.0)).astype(np.uint32)
    return ((c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).reshape(-1)


def fold(cs):
    """cs: K float32 [pixels, 3] frames (radiance or resolved means; clamped here) -> (packed uint32 [pixels], float32 mean [pixels, 3])"""
    cs = [np.clip(np.asarray(c, F32), F32(0), F32(1)) for c in cs]
    s = cs[0].copy()
    for c in cs[1:]:
        s = s + c                                          # float32, one rounding
    r = F32(1.0) / F32(len(cs))                            # correctly rounded
    mean = np.minimum(s * r, F32(1.0))
    return pack(mean), mean


def radical_inverse(f, base):
    inv = 1.0 / base                                       # Python floats are doubles: the C digit loop, operation for operation
    w, r = inv, 0.0
    while f:
        r += float(f % base) * w
        f //= base
        w *= inv
    return r


def halton(f):
    """-> (jx, jy) float32: the Halton (2, 3) point of frame f, centred on 0"""
    return F32(radical_inverse(f, 2) - 0.5), F32(radical_inverse(f, 3) - 0.5)


def camera_rows(cam):
    """clw_camera / oracle Camera -> (im_corner, origin, up, right) float32 [3] each"""
    return tuple(np.array(list(v), F32) for v in (cam.im_corner, cam.origin, cam.up, cam.right))


def jittered(cam, f, n, cls=None):
    """The camera of frame f (a `cls` structure, default type(cam)): im_corner = (im_corner + right ax) - up ay in float32, the rest copied."""
    out = (cls or type(cam))()
    corner, origin, up, right = camera_rows(cam)
    if f:
        jx, jy = halton(f)
        ax = (F32(cam.w_factor) / F32(n)) * jx
        ay = (F32(cam.h_factor) / F32(n)) * jy
        corner = (corner + right * ax) - up * ay
    for name, v in (("im_corner", corner), ("origin", origin), ("up", up), ("right", right)):
        for i in range(3):
            getattr(out, name)[i] = float(v[i])
    out.w_factor, out.h_factor = float(F32(cam.w_factor)), float(F32(cam.h_factor))
    out.width, out.height = cam.width, cam.height
    return out


def camera_bytes(cam):
    corner, origin, up, right = camera_rows(cam)
    return np.concatenate([corner, origin, up, right, np.array([cam.w_factor, cam.h_factor], F32)]).tobytes() + \
        np.array([cam.width, cam.height], np.uint32).tobytes()


# ---- the GPU side (R = renderer.Renderer, api = the api module; `cam`: the view, conftest.CAM unless given; `setup(w)`: knobs set on the wrapper)
def base_camera(api, W, H, cam=CAM):
    return api.perspective(cam["origin"], cam["look"], cam["fov"], cam["focal"], W, H)


def plain(R, sc, tex, sky, W, H, depth, strict, cam, n=1, seed=0, setup=None, **kw):
    """one frame of a fresh renderer with the mode off -> (packed, float)"""
    with rendering(R, sc, tex, sky, W, H, setup=setup, cam=cam, depth=depth, strict=strict, supersample=n, seed_offset=seed, **kw) as r:
        return take(r)[0]


_own = {}


def own_frames(R, api, sc, tex, sky, W, H, n, depth, strict, jitter, count, cam=CAM, name=None, setup=None):
    """the constituent frames 0 .. count-1 of a view, each from a fresh renderer, rendered once per process (`name` tells scenes, cameras and
    set-ups apart)"""
    key = (W, H, n, depth, strict, jitter, name)
    have = _own.setdefault(key, [])
    cam = base_camera(api, W, H, cam)
    while len(have) < count:
        f = len(have)
        p, c = plain(R, sc, tex, sky, W, H, depth, strict, api.jitter_camera(cam, f, n) if jitter else cam, n=n, seed=api.frame_seed(f), setup=setup)
        p.setflags(write=False); c.setflags(write=False)
        have.append((p, c))
    return have[:count]


def accumulated(R, api, sc, tex, sky, W, H, n, depth, strict, jitter, count, max_frames=64, cam=CAM, setup=None, flags=None, **kw):
    """`count` frames in a row of one accumulating renderer -> [(packed, float, K) ...]; the flags of the last trace launch are appended to `flags`"""
    with rendering(R, sc, tex, sky, W, H, setup=setup, cam=base_camera(api, W, H, cam), depth=depth, strict=strict, supersample=n,
                   accumulate=max_frames, jitter=jitter, **kw) as r:
        out = take(r, count, extra=lambda r: r.accumulated)
        if flags is not None:
            flags.append(r.w.last_trace_flags())
        return out
