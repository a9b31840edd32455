"""Shared by test_sample_cameras_host.py and test_gpu_sample_cameras.py: the numpy reference of the definition of per-sample cameras.

With factor n and a table cams[0 .. n*n), the sample at virtual pixel (vx, vy) is pixel (vx, vy) of a 1-sample render of the n*W x n*H
frame through cams[(vy mod n) * n + (vx mod n)] with w_factor / n, h_factor / n; clamp, add and scale as plain supersampling (render_common.resolve)."""
import numpy as np

from conftest import CAM
from render_common import rendering, resolve, take

CAM2 = dict(origin=(1.6, 3.1, -6.5), look=(0.05, -0.15, 1.0), fov=90.0, focal=1.0)      # a clearly different camera (the shutter's other end)


def slot(k, n):
    """sample k = sy * n + sx -> lens cell / shutter slot: k with its 2 log2 n bits reversed"""
    bits = 2 * (n.bit_length() - 1)
    return int(format(k, f"0{bits}b")[::-1], 2)


def pick(render_virtual, W, H, n):
    """render_virtual(k) -> float32 [n*H * n*W, 3] (or any per-virtual-pixel array) of camera k's 1-sample virtual frame -> the frame whose
    virtual pixel (vx, vy) comes from camera (vy mod n) * n + (vx mod n)"""
    out = None
    for sy in range(n):
        for sx in range(n):
            f = np.asarray(render_virtual(sy * n + sx))
            f = f.reshape((n * H, n * W) + f.shape[1:])
            out = np.empty_like(f) if out is None else out
            out[sy::n, sx::n] = f[sy::n, sx::n]
    return out


def composed(render_virtual, cams, W, H, n):
    """-> (packed uint32 [W*H], float32 mean [W*H, 3]) of the frame the table `cams` defines"""
    assert len(cams) == n * n
    return resolve(pick(render_virtual, W, H, n).reshape(-1, 3), W, H, n)


def rows_of(cam):
    """clw_camera / oracle Camera -> float32 [12] = {im_corner, origin, up, right}"""
    return np.concatenate([np.asarray(list(v), np.float32) for v in (cam.im_corner, cam.origin, cam.up, cam.right)])


def virtual_camera(cls, row, base, n):
    """Row of a table + the W x H camera `base` -> the camera (a `cls` structure) of the n*W x n*H 1-sample render that defines its samples."""
    cam = cls()
    for name, k in (("im_corner", 0), ("origin", 3), ("up", 6), ("right", 9)):
        for i in range(3):
            getattr(cam, name)[i] = float(row[k + i])
    cam.w_factor = np.float32(base.w_factor) / np.float32(n)        # what the launch divides: exact for a power of two
    cam.h_factor = np.float32(base.h_factor) / np.float32(n)
    cam.width, cam.height = base.width * n, base.height * n
    return cam


# ---- the GPU side of the definition (R = renderer.Renderer, api = the api module)
def make_table(api, W, H, n, kind, cam=CAM, cam2=CAM2):
    """kind: (aperture, focus) = the lens table, "shutter" = an open shutter from cam to cam2 -> (base camera, float32 [n*n, 12])"""
    base = api.perspective(**cam, width=W, height=H)
    if kind == "shutter":
        return base, api.shutter_cameras(base, api.perspective(**cam2, width=W, height=H), n)
    return base, api.lens_cameras(base, kind[0], kind[1], n)


def gpu_composed(R, api, sc, tex, sky, base, table, W, H, n, depth, strict, setup=None):
    """`composed` over the GPU's own 1-sample virtual frames (one renderer, camera re-set per table entry) -> (packed, float), flags"""
    with rendering(R, sc, tex, sky, n * W, n * H, setup=setup, cam=None, depth=depth, strict=strict) as r:
        def render_virtual(k):
            r.set_camera(virtual_camera(api.clw_camera, table[k], base, n))
            return r.render_rgb()[1]
        return composed(render_virtual, table, W, H, n), r.w.last_trace_flags()


def sampled(R, sc, tex, sky, W, H, n, depth, strict, kind, table=None, count=1, setup=None, cam=CAM, rgb=True, **kw):
    """`count` frames of one supersampled renderer with a lens (kind = (aperture, focus)), an explicit table (kind "shutter" / "table") or
    neither (kind None) -> [(packed, float)], flags, the table the last launch used"""
    def knobs_then_table(w):
        if setup:
            setup(w)
        if kind in ("shutter", "table"):
            w.set_sample_cameras(table)
    with rendering(R, sc, tex, sky, W, H, setup=knobs_then_table, cam=cam, depth=depth, strict=strict, supersample=n,
                   lens=kind if isinstance(kind, tuple) else None, **kw) as r:
        return take(r, count, rgb), r.w.last_trace_flags(), r.w.get_sample_cameras()
