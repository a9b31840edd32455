"""Shared by test_sample_cameras_host.py and test_gpu_sample_cameras.py: the numpy reference of the definition of per-sample cameras.

With factor n and a table cams[0 .. n*n), the sample at virtual pixel (vx, vy) is pixel (vx, vy) of a 1-sample render of the n*W x n*H
frame through cams[(vy mod n) * n + (vx mod n)] with w_factor / n, h_factor / n; clamp, add and scale as plain supersampling (`resolve`)."""
import numpy as np


def resolve(rgb, W, H, n):                      # rgb: float32 [n*H * n*W, 3], virtual-frame order (as in test_gpu_supersample.py)
    s = np.clip(rgb.reshape(H * n, W * n, 3), np.float32(0), np.float32(1))
    k = n
    while k > 1: s = s[:, 0::2] + s[:, 1::2]; k //= 2
    k = n
    while k > 1: s = s[0::2] + s[1::2]; k //= 2
    s = s * np.float32(1.0 / (n * n))
    c = (s * np.float32(255.0)).astype(np.uint32)
    return ((c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).reshape(-1), s.reshape(-1, 3)


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
