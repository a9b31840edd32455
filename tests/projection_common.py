"""Shared by test_projection_host.py and test_gpu_projection.py: the cameras and sizes both files run the camera models beside the pinhole
on (include/hip_wrap_ext.h: clw_projection), the float64 numpy statement of the panorama's formula, the expected primary-hit buffers of a
ray buffer (tests/gbuffer_common.py's recipe with the rays swapped in) and the planner's input with the projection word.

The yardstick of every frame is oracle.trace_rays on the host definition's records (api.projection_rays): the oracle traces any 64-byte ray
record, so the models need nothing added to it."""
import ctypes as C

import numpy as np

import gbuffer_common as gc
import plan_common as pc

F32 = np.float32
# the views: an oblique one over the demo scene (right and up are not unit: the look leaves the horizontal), and an axis-aligned one
VIEW = dict(origin=(0.8, 2.5, -8.0), look=(0.2, -0.15, 1.0))
VIEW_Z = dict(origin=(0.0, 1.5, -6.0), look=(0.0, 0.0, 1.0))
ORTHO_WIDTH = 12.0
# (width, height, first_row, rows or None, bands or None): partial tiles both ways and 11 full raygen blocks plus a partial one; the panorama's
# frame; one row; one pixel; a strip of 67 x 45; bands of 64 x 48
SIZES = {"67x45": (67, 45, 0, None, None), "64x32": (64, 32, 0, None, None), "9x1": (9, 1, 0, None, None), "1x1": (1, 1, 0, None, None),
         "strip": (67, 45, 16, 21, None), "bands": (64, 48, 0, None, (2, 1))}
MODELS = ("ortho", "equirect")


def view_of(api, model, W, H, view=VIEW, span=(360.0, 180.0), ortho_width=ORTHO_WIDTH):
    """(clw_camera, clw_projection) of a model on a W x H frame"""
    if model == "ortho":
        return api.ortho_camera(view["origin"], view["look"], ortho_width, W, H)
    cam = api.perspective(view["origin"], view["look"], 90.0, 1.0, W, H)
    return cam, api.projection(api.PROJ_EQUIRECT if model == "equirect" else api.PROJ_PERSPECTIVE, view["look"], 0.0, span)


def global_ids(W, H, first_row=0, rows=None, bands=None):
    """the global ids of a renderer's work-items, in work-item order"""
    if bands is not None:
        stride, phase = bands
        y = np.arange(H // stride)
        gy = ((y // 8) * stride + phase) * 8 + y % 8
        return (gy[:, None] * W + np.arange(W)[None, :]).reshape(-1)
    rows = H - first_row if rows is None else rows
    return np.arange(first_row * W, (first_row + rows) * W)


def host_rays(api, cam, proj, W, H, first_row=0, rows=None, bands=None):
    """the host definition's records of a renderer's work-items"""
    ids = global_ids(W, H, first_row, rows, bands)
    if bands is None:
        return api.projection_rays(cam, proj, int(ids[0]), int(ids[-1]) + 1)
    return api.projection_rays(cam, proj)[ids]


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


def equirect_f64(cam, proj, W, H):
    """float64 numpy: direction of every pixel, cos(phi) (sin(theta) r + cos(theta) a) + sin(phi) u -> [H, W, 3], and (a, r, u)"""
    a = np.array(proj.axis[:], F32)
    a = (a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])).astype(np.float64)      # the axis is normalised once, in float32
    r = np.array(cam.right[:], np.float64)
    r = unit(r - (r @ a) * a)
    u = np.array(cam.up[:], np.float64)
    u = unit(u - (u @ a) * a - (u @ r) * r)
    hs = np.deg2rad(np.float64(proj.h_span or 360.0))
    vs = np.deg2rad(np.float64(proj.v_span or 180.0))
    th = ((np.arange(W) + 0.5) / W - 0.5) * hs
    ph = (0.5 - (np.arange(H) + 0.5) / H) * vs
    col = np.sin(th)[:, None] * r + np.cos(th)[:, None] * a
    d = np.cos(ph)[:, None, None] * col[None, :, :] + np.sin(ph)[:, None, None] * u
    return d, (a, r, u, th, ph)


class _RaysAs:
    """what gbuffer_common.expected_gbuffer asks of an oracle, with a caller's ray buffer where wo_raygen's would be"""

    def __init__(self, oracle, rays):
        self.lib, self._rays = oracle.lib, np.ascontiguousarray(rays, F32)

    def raygen(self, cam):
        return self._rays


def expected_gbuffer(oracle, scene, tex, sky, rays):
    """gbuffer_common.expected_gbuffer's recipe on `rays`: wo_find_light, wo_intersect_*, wo_find_solid per record"""
    return gc.expected_gbuffer(_RaysAs(oracle, rays), scene, tex, sky, None)


def id_boundary(ids, W):
    """per pixel of a whole-rows image: the set test of G5 -- (its 3x3 neighbourhood holds another id, the neighbours' ids as a [n, 9] array)"""
    img = np.asarray(ids, np.uint32).reshape(-1, W)
    pad = np.pad(img, 1, mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + img.shape[0], 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], -1)
    return (nb != img[..., None]).any(-1).reshape(-1), nb.reshape(-1, 9)


# ---- the planner's input under a camera model (csrc/launch_plan.h: rays_generated = 1 + the model for rays this library generates)
def plan_in(projection=0, **kw):
    """plan_common.plan_in's launch with the generated rays under a projection model (a caller's rays have none)"""
    i = pc.plan_in(**kw)
    if i.rays_generated:
        i.rays_generated = 1 + projection
    return i


plan, refusal = pc.plan, pc.refusal
