"""The raypng.c call protocol as a reusable object.

Every device interaction goes through the six ``cl_wrap_*`` entry points in the order the
reference driver uses them (reference raypng.c:31-89): kernel 0 ("raygen") arguments 0-7
by value and 8 = ray buffer; kernel 1 ("raytracer") argument 0 = the 8-byte handle of
``buffers[0][8]``, 1-3 scene arrays, 4-6 counts, 7 pixel count, 8 texture array,
9 skybox, 10 framebuffer; then ``output(run 0)`` and ``output(run 1, read [1][10])``.

Row strips (multi-GPU): a renderer may own rows ``[first_row, first_row + rows)`` of the
frame; work-item ids, and with them ``id % W``, ``id / W`` and the RNG seed, stay global
(SURVEY.md 8(e)), so a strip is bit-identical to the same rows of a full-frame render.

``supersample=n`` (2, 4, 8): every pixel is the mean of n x n samples traced and resolved inside the
kernel (include/hip_wrap_ext.h, clw_ext_set_supersample); ``render()`` and ``render_rgb()`` still
return W*H entries, and strips compose as before.

``lens=(aperture, focus)`` (with ``supersample`` > 1): the n x n samples of a pixel look through n x n points of a thin lens focused at
distance ``focus`` (clw_ext_set_lens); ``set_sample_cameras`` hands the kernel any table of n x n cameras instead, e.g.
``api.shutter_cameras`` for camera motion blur.

``motion=disp`` (float32 [spheres, 3], with ``supersample`` > 1): object motion blur -- sphere i moves by ``disp[i]`` while the shutter is
open and every sample sees the scene at its own time (clw_ext_set_sphere_motion; ``set_sphere_motion(disp, times)`` to change it).

``adaptive=T`` (0..256, with ``supersample`` > 1, without lens, sample cameras or motion): only the blocks of 8/n x 8/n pixels in which the
1-sample frame shows a contrast of at least T between neighbouring pixels take their n x n samples, the others keep the 1-sample value
(clw_ext_set_adaptive; ``w.read_refine_mask()`` tells which).  A strip is classified on its own rows, so its edge rows may differ from the
full frame's.

``accumulate=N`` (1..65536; without lens, sample cameras, motion or adaptive): progressive accumulation -- while nothing that defines the image
changes, every ``render()`` traces the view once more with its own random numbers and (``jitter=True``) its own sub-pixel offset and returns the
running mean of the frames so far, until N frames are in; then it returns that mean without tracing (clw_ext_set_accumulate).  ``accumulated``
tells how many frames the mean holds, ``reset_accumulation()`` starts again.  ``seed_offset=s`` shifts the random seed of every pixel
(clw_ext_set_seed_offset).  ``render_rgb()`` returns the mean (clamped to [0, 1]) while the mode is on.

``gbuffer()`` / ``pick(x, y)``: the primary-hit pass (clw_ext_render_gbuffer, clw_ext_pick) -- depth, object id, normal, hit point and albedo of
what the launch camera sees first at every pixel of this renderer's rows, or at one pixel of the frame.  No sampling mode above changes them,
and they leave an accumulating view counting.

``highlight(ids, ...)``: the selection overlay (clw_ext_render_overlay) -- the frame of the last ``render()`` with the objects whose ids are listed
(``pick(x, y)["id"]``, up to 64) outlined, tinted, or both, and optionally a line along every object boundary, composed on the device from the
frame and an id pass where they lie.  It never writes the traced frame, leaves ``gbuffer()``'s buffers and an accumulating view alone, and is
not available with row bands.  A strip is composed on its own rows: within ``radius`` rows of its edges it can differ from the full frame's.

``ambient_occlusion(rays, radius, ...)`` / ``ao_counts()``: ray-traced ambient occlusion (clw_ext_render_ao) -- the "clay" view: every visible
point shaded by how much of the hemisphere above it is open within ``radius``, from ``rays`` short any-hit rays per pixel traced on the device
over a primary-hit pass; or, with ``compose=True``, the frame of the last ``render()`` multiplied by it.  It never writes the traced frame, leaves
``gbuffer()``'s buffers, the overlay, the object table and an accumulating view alone, honours the camera model, and is not available with row
bands.  Strips' counts concatenate to the frame's; the filter runs on a strip's own rows.

``cast_rays(origins, dirs, ...)`` / ``cast_rays_device(...)`` / ``line_of_sight(a, b)``: ray queries (clw_ext_cast_rays) -- where the CALLER's
rays meet the scene, from anywhere, no camera involved: the nearest hit (t, id, normal, point) of every ray, or with ``any_hit`` whether it meets
anything within ``tmax``.  Directions are not normalised: t is in units of their length, so ``line_of_sight(a, b)`` casts ``b - a`` with
``tmax = 1``.  Nothing else the renderer holds is touched.

``cast_layers(origins, dirs, K, ...)`` / ``layers(K)`` / ``pick_through(x, y)`` / ``camera_rays()``: layered ray queries
(clw_ext_cast_layers) -- the K (1..8) nearest surfaces of every ray in depth order instead of the first one, in one launch: along the
caller's rays, along every pixel's camera ray, or under one pixel (click again to select the object behind).  ``camera_rays()`` returns the
launch camera's rays as query rays.  Nothing else the renderer holds is touched; not available with row bands.

``cast_paths(origins, dirs, bounces, ...)`` / ``cast_paths_device(...)`` / ``pick_path(x, y)``: path queries (clw_ext_cast_paths) -- where a
ray GOES: its hit, the reference's reflected (with ``transmit``, through glass: refracted) ray from there, that ray's hit, and so on for up
to 8 segments in one launch; ``pick_path`` answers what a pixel shows and what is reflected in that.  Nothing else the renderer holds is
touched; ``pick_path`` is not available with row bands.

``nearest_surface(points, reach)`` / ``within_reach(points, reach)`` / ``near_surfaces(points, K, reach)`` / ``probe_device(...)`` /
``near_surfaces_device(...)`` / ``touching_spheres(margin, K)``: proximity queries (clw_ext_nearest_surface) -- what lies AROUND a point, no
direction involved: the nearest surface within ``reach`` (signed distance, id, normal, nearest point; a point inside a sphere has a negative
distance), whether a ball of that radius touches anything, or the K (1..8) nearest surfaces in order; ``touching_spheres`` asks it of every
sphere of the scene.  Nothing else the renderer holds is touched.

``projection=...`` / ``set_projection(model, ...)`` / ``look_ortho`` / ``look_panorama``: the camera models beside the pinhole
(clw_ext_set_projection) -- ``'ortho'``: parallel rays from the image plane, the top / front / side view of an editor; ``'equirect'``: a
latitude-longitude panorama of up to 360 x 180 degrees around the camera origin.  ``render()``, ``read_rays()``, ``gbuffer()``, ``pick``,
``highlight``, ``objects`` and ``select_rect`` all honour the model; row strips and bands work unchanged (everything is indexed by global id).
A projected frame is traced from a generated ray buffer, so it does not combine with ``supersample`` > 1, ``lens``, sample cameras,
``motion``, ``adaptive`` or ``accumulate``: the trace launch refuses them.

A renderer is a context manager: ``with Renderer(...) as r:`` releases it on the way out; releasing twice is harmless.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import api
from .scene import RAY, Scene


def strip_rows(height: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous row strip of `rank` out of `world`: (first_row, rows).  Rows are dealt in
    multiples of 8 (the tile height) while they last, so every strip but the last is tile-aligned."""
    tiles = (height + 7) // 8
    base, extra = divmod(tiles, world)
    t0 = rank * base + min(rank, extra)
    t1 = t0 + base + (1 if rank < extra else 0)
    r0, r1 = min(t0 * 8, height), min(t1 * 8, height)
    return r0, r1 - r0


class Renderer:
    def __init__(self, scene: Scene, tex: np.ndarray, sky: np.ndarray, width: int, height: int, *,
                 depth: int = 15, strict: bool = False, fuse: bool = True, first_row: int = 0,
                 rows: int | None = None, bands: tuple[int, int] | None = None, framebuffer_ptr: int | None = None, wide_counts: bool | None = None,
                 texture_paths=None, skybox_path=None, supersample: int = 1,
                 lens: tuple[float, float] | None = None, motion=None, adaptive: int | None = None,
                 accumulate: int = 0, jitter: bool = True, seed_offset: int = 0, projection=None):
        self.width, self.height = width, height
        self.first_row = first_row
        self.rows = height - first_row if rows is None else rows
        if bands is not None:                              # (stride, phase): every stride-th 8-row band
            assert first_row == 0 and rows is None and height % (8 * bands[0]) == 0
            self.rows = height // bands[0]
        self.pixels = self.rows * width                   # work-items of this renderer
        self.scene = scene
        w = self.w = api.ClWrap("src/cl/raygen.cl", "raygen", "src/cl/raytracing.cl", "raytracer")
        w.set_depth(depth)
        w.set_strict(strict)
        w.set_fuse(fuse)
        w.set_id_offset(first_row * width)
        if supersample != 1:      # n x n samples per pixel, resolved in the trace kernel: sizes, rows and strips here stay in output pixels
            w.set_supersample(supersample)
        if lens is not None:      # (aperture, focus): depth of field from the samples of a pixel
            w.set_lens(*lens)
        if motion is not None:    # float32 [spheres, 3]: how far each sphere moves while the shutter is open
            w.set_sphere_motion(motion)
        if adaptive is not None:  # contrast threshold 0..256: the samples only where the 1-sample frame shows that much contrast
            w.set_adaptive(adaptive)
        if seed_offset:           # added to the id that seeds a pixel's random numbers
            w.set_seed_offset(seed_offset)
        self.accumulate = int(accumulate)
        if self.accumulate:       # frames a still view accumulates; each with its own seeds and (jitter) sub-pixel offset
            w.set_accumulate(self.accumulate, jitter)
        if bands is not None:
            w.set_row_bands(*bands)
        if projection is not None:      # a model name, an api.PROJ_* value or an api.clw_projection: the camera model beside the pinhole
            self.set_projection(projection)

        u32 = lambda v: np.uint32(v)
        w.load_single_data(0, 6, u32(width))
        w.load_single_data(0, 7, u32(height))
        w.load_global_data(0, 8, None, RAY.itemsize * self.pixels, api.CL_MEM_READ_WRITE)
        w.load_single_data(1, 0, w.buffer_handle(0, 8))
        ns, np_, nl = scene.counts
        w.load_global_data(1, 1, scene.spheres, mem_flags=api.CL_MEM_READ_ONLY)
        w.load_global_data(1, 2, scene.planes, mem_flags=api.CL_MEM_READ_ONLY)
        w.load_global_data(1, 3, scene.lights, mem_flags=api.CL_MEM_READ_ONLY)
        wide = (max(ns, np_, nl) > 255) if wide_counts is None else wide_counts
        cnt = (lambda v: np.uint32(v)) if wide else (lambda v: np.uint8(v))   # uchar in the reference
        w.load_single_data(1, 4, cnt(ns))
        w.load_single_data(1, 5, cnt(np_))
        w.load_single_data(1, 6, cnt(nl))
        # `pixels` = the guard `id >= total_size` (raytracing.cl:24); work-items here are strip-local
        w.load_single_data(1, 7, u32(self.pixels))
        if texture_paths is not None:
            w.load_images(1, 8, *texture_paths)
        else:
            w.load_images_raw(1, 8, tex)
        if skybox_path is not None:
            w.load_images(1, 9, skybox_path)
        else:
            w.load_images_raw(1, 9, sky)
        if framebuffer_ptr is not None:
            w.bind_device_buffer(1, 10, framebuffer_ptr, 4 * self.pixels)
        else:
            w.load_global_data(1, 10, None, 4 * self.pixels, api.CL_MEM_WRITE_ONLY)
        self._rgb_dev = None
        self._camera_set = False

    # ---- camera: the six values of rgen_perspective, re-settable at any time (rayinteractive.c:98-103)
    def set_camera(self, cam) -> None:
        w = self.w
        f3 = lambda v: np.array([v[0], v[1], v[2], 0.0], np.float32)     # cl_float3 = 16 bytes
        w.load_single_data(0, 0, f3(cam.im_corner))
        w.load_single_data(0, 1, f3(cam.origin))
        w.load_single_data(0, 2, f3(cam.up))
        w.load_single_data(0, 3, f3(cam.right))
        w.load_single_data(0, 4, np.float32(cam.w_factor))
        w.load_single_data(0, 5, np.float32(cam.h_factor))
        self._camera_set = True

    def set_sample_cameras(self, cams) -> None:
        """float32 [n*n, 12]: sample k = sy * n + sx of every pixel looks through camera k (None = the launch camera); replaces a lens."""
        self.w.set_sample_cameras(cams)

    def set_sphere_motion(self, disp, times=None) -> None:
        """float32 [spheres, 3]: sample k of every pixel sees sphere i at centre + times[k] * disp[i] (None = the shutter times of
        api.sample_times); disp None / empty / all zero = the scene stands still."""
        self.w.set_sphere_motion(disp, times)

    def look(self, origin, look, fov=90.0, focal=1.0):
        cam = api.perspective(origin, look, fov, focal, self.width, self.height)
        self.set_camera(cam)
        return cam

    # ---- the camera models beside the pinhole
    def set_projection(self, model, *, axis=None, ortho_width: float = 0.0, span=(360, 180)) -> None:
        """model: None / 'perspective' (the pinhole), 'ortho', 'equirect', an api.PROJ_* value, or a ready api.clw_projection.  axis: the view
        direction (None = from the camera origin to the centre of its image plane); ortho_width: the world units an orthographic frame's width
        spans (0 = the camera's image plane as it stands); span: the (horizontal, vertical) degrees a panorama covers."""
        if model is None or isinstance(model, api.clw_projection):
            self.w.set_projection(model)
        else:
            self.w.set_projection(api.projection(model, axis, ortho_width, span))

    def look_ortho(self, origin, look, view_width: float):
        """An orthographic view from `origin` along `look` whose frame spans `view_width` world units -> the camera set."""
        cam, proj = api.ortho_camera(origin, look, view_width, self.width, self.height)
        self.set_camera(cam)
        self.w.set_projection(proj)
        return cam

    def look_panorama(self, origin, look=(0, 0, 1), span=(360, 180)):
        """A latitude-longitude panorama around `origin` whose centre column looks along `look` -> the camera set."""
        cam = api.perspective(origin, look, 90.0, 1.0, self.width, self.height)
        self.set_camera(cam)
        self.w.set_projection(api.projection(api.PROJ_EQUIRECT, look, 0.0, span))
        return cam

    # ---- one frame: raygen launch + trace launch (+ blocking read-back)
    def render(self, readback: bool = True):
        self.w.output(self.pixels, 0, 0, 0, 0, None)
        if not readback:
            self.w.output(self.pixels, 0, 1, 1, 10, None)
            return None
        out = np.empty(self.pixels, np.uint32)
        self.w.output(self.pixels, out.nbytes, 1, 1, 10, out)
        return out

    def render_rgb(self):
        """-> (packed uint32[n], float32[n,3]): the optional float debug output -- un-clamped radiance of a 1-sample launch, the resolved mean of a
        supersampled one, the running mean (in [0, 1]) while a view accumulates."""
        if self._rgb_dev is None:
            self.w.load_global_data(1, 31, None, 12 * self.pixels, api.CL_MEM_WRITE_ONLY)  # spare arg slot
            self._rgb_dev = self.w.device_ptr(1, 31)
        self.w.set_debug_rgb(self._rgb_dev)
        out = self.render()
        rgb = np.empty((self.pixels, 3), np.float32)
        # cl_wrap_output reads a buffer back only behind a launch: the trace launch again -- but while a view accumulates that would be its next
        # frame, so then the raygen launch, which in fused mode only latches the camera again; equal camera values do not restart the sum
        # (hip_wrap_ext.h, clw_ext_set_accumulate: the key compares them by value)
        accumulating = hasattr(self.w.L, "clw_ext_get_accumulated") and self.accumulated > 0      # (set here or by CLWRAP_ACCUMULATE)
        self.w.output(self.pixels, rgb.nbytes, 0 if accumulating else 1, 1, 31, rgb)
        self.w.set_debug_rgb(0)
        return out, rgb

    @property
    def accumulated(self) -> int:
        """Frames in the running mean after the last render (0 = the mode is off)."""
        return self.w.get_accumulated()

    def reset_accumulation(self) -> None:
        self.w.reset_accumulation()

    def _latch_camera(self) -> None:
        """Ahead of every inspection pass: the raygen launch latches the camera set last (in fused mode it does nothing else)."""
        if self._camera_set:
            self.w.output(self.pixels, 0, 0, 0, 0, None)

    # ---- the primary-hit pass
    def gbuffer(self, channels: int = api.GB_ALL) -> dict:
        """{"depth": [n], "id": [n], "normal": [n, 3], "point": [n, 3], "albedo": [n, 3]} of the requested channels (api.GB_*) for the n work-items
        of this renderer, through the camera set last."""
        self._latch_camera()
        if self.w.render_gbuffer(channels) != self.pixels:
            raise RuntimeError("the primary-hit pass did not cover this renderer's range (is a camera set, is `channels` a mask of api.GB_*?)")
        return {name: self.w.read_gbuffer(bit) for name, (bit, _, _) in api.GB_CHANNELS.items() if channels & bit}

    def pick(self, x: int, y: int) -> dict | None:
        """What lies under pixel (x, y) of the frame: {"id", "kind", "index", "depth", "point", "normal", "albedo"} -- the entries of that pixel in
        ``gbuffer()``, bit for bit -- or None when the pixel is not one of this renderer's rows (or no camera has been set)."""
        self._latch_camera()
        p = self.w.pick(x, y)
        if p is None:
            return None
        return api.id_entry(p.id, depth=np.float32(p.depth), point=np.array(p.point[:], np.float32), normal=np.array(p.normal[:], np.float32),
                            albedo=np.array(p.albedo[:], np.float32))

    # ---- the selection overlay
    def highlight(self, ids, *, outline: int | None = 0xFFFF00, radius: int = 2, fill: int | None = None, alpha: int = 96,
                  edges: int | None = None) -> np.ndarray:
        """The frame of the last ``render()`` with the objects in `ids` (an id or up to 64 of them, e.g. ``pick(x, y)["id"]``) shown as selected
        -> uint32 [pixels].  outline: colour of a band of `radius` (1..4) pixels around them, None = none; fill: colour blended over them with
        weight alpha / 256, None = none; edges: colour of a line along every boundary between two objects, None = none.  Colours are 0x00RRGGBB."""
        flags = (api.OV_OUTLINE if outline is not None else 0) | (api.OV_FILL if fill is not None else 0) | (api.OV_EDGES if edges is not None else 0)
        style = api.overlay_style(flags, radius, outline or 0, fill or 0, alpha, edges or 0)
        self._latch_camera()
        if self.w.render_overlay(style, ids) != self.pixels:
            raise RuntimeError("the selection overlay was refused (a camera set and a frame rendered? at most 64 ids, radius in 1..4, alpha in "
                               "0..256, something to draw, no row bands?)")
        return self.w.read_overlay()

    # ---- ambient occlusion
    def ambient_occlusion(self, rays: int = 8, radius: float = 1.0, strength: int = 256, filter: bool = True, compose: bool = False) -> np.ndarray:
        """The view shaded by geometry alone -> uint32 [rows, width], grey 0x00VVVVVV: `rays` (1..32) short any-hit rays of length `radius` (world
        units; inf = unlimited) over the hemisphere of every visible point's normal, traced on the device from a primary-hit pass; `strength`
        (0..256) scales how much of the occlusion shows; `filter` averages the 4 x 4 interleaved ray patterns away among pixels of the same
        object; `compose` multiplies the frame of the last ``render()`` by the result instead."""
        ao = api.ao_params(rays, radius, strength, filter, compose)
        self._latch_camera()
        if self.w.render_ao(ao) != self.pixels:
            raise RuntimeError("the ambient occlusion pass was refused (a camera set? rays in 1..32, radius > 0, strength in 0..256, no row bands, "
                               "with compose a frame rendered?)")
        return self.w.read_ao(api.AO_FRAME).reshape(self.rows, self.width)

    def ao_counts(self) -> np.ndarray:
        """The open rays (0..rays) of every pixel in the last ``ambient_occlusion()`` -> uint8 [rows, width]."""
        counts = self.w.read_ao(api.AO_COUNTS)
        if counts.size != self.pixels:
            raise RuntimeError("no ambient occlusion pass has run on this renderer's range yet")
        return counts.reshape(self.rows, self.width)

    # ---- ray queries
    def cast_rays(self, origins, dirs, tmax=np.inf, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False, any_hit: bool = False) -> np.ndarray:
        """Where the rays origins[k] + t * dirs[k] (arrays of [n, 3]; dirs as given, not normalised: t is in units of their length) meet the scene
        -> api.HIT [n]: t (inf = a miss), id (api.ID_NONE = a miss), normal, point of the nearest primitive with 0 < t <= tmax; with `any_hit` a
        bool [n] instead: does the ray meet anything that near.  tmax and ignore (the id word of the one primitive a ray does not test, e.g. the
        object it starts on; None = none) are scalar or per ray; kinds: which of 'sphere', 'plane', 'light' take part; opaque_only: transparent
        spheres let the ray pass.  Needs no camera."""
        rays = api.make_rays(origins, dirs, tmax, ignore)
        flags = api.cast_flags(kinds, opaque_only)
        got = self.w.occluded_rays(rays, flags) if any_hit else self.w.cast_rays(rays, flags)
        if got is None:
            raise RuntimeError("the ray query was refused (at least one ray, at least one kind?)")
        return got.astype(bool) if any_hit else got

    def cast_rays_device(self, rays_ptr: int, n: int, hits_ptr: int | None = None, blocked_ptr: int | None = None, kinds=("sphere", "plane"),
                         opaque_only: bool = False) -> int:
        """The query over the caller's device memory, by integer device address as ``framebuffer_ptr``: n api.RAY_QUERY records in, n api.HIT
        records (`hits_ptr`: nearest) or n bytes (`blocked_ptr`: any) out -- exactly one of the two.  Launched on the wrapper's stream
        (``w.set_stream``) without waiting -> n."""
        got = self.w.cast_rays_device(rays_ptr, n, api.cast_flags(kinds, opaque_only), hits_ptr, blocked_ptr)
        if got != n:
            raise RuntimeError("the ray query was refused (at least one ray, at least one kind, exactly one of hits_ptr and blocked_ptr?)")
        return got

    def line_of_sight(self, a, b, opaque_only: bool = True) -> np.ndarray:
        """Can a[k] see b[k]? -> bool [n]: no sphere or plane (with `opaque_only`, no opaque one) is met by the ray from a to b with direction
        b - a at 0 < t <= 1 -- t is in units of |b - a|, so tmax = 1 ends the ray exactly at b."""
        a = np.asarray(a, np.float32).reshape(-1, 3)
        b = np.asarray(b, np.float32).reshape(-1, 3)
        return ~self.cast_rays(a, b - a, tmax=1.0, opaque_only=opaque_only, any_hit=True)

    # ---- proximity queries
    def nearest_surface(self, points, reach=np.inf, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False) -> np.ndarray:
        """The surface nearest to every point (array of [n, 3]) among those within `reach` of it -> api.HIT [n]: t = the distance (signed for a
        sphere or light: negative inside; inf = nothing within reach), id (api.ID_NONE = nothing), the surface's normal toward the point and its
        nearest point.  reach and ignore (the id word of the one primitive a probe does not test; None = none) are scalar or per point; a
        negative reach asks for penetrations at least that deep; kinds and opaque_only as ``cast_rays``.  Needs no camera."""
        got = self.w.nearest_surface(api.make_probes(points, reach), api.cast_flags(kinds, opaque_only), ignore)
        if got is None:
            raise RuntimeError("the proximity query was refused (at least one point, at least one kind?)")
        return got

    def within_reach(self, points, reach, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False) -> np.ndarray:
        """Does a ball of radius `reach` placed at every point touch anything? -> bool [n] (arguments as ``nearest_surface``)."""
        got = self.w.within_reach(api.make_probes(points, reach), api.cast_flags(kinds, opaque_only), ignore)
        if got is None:
            raise RuntimeError("the proximity query was refused (at least one point, at least one kind?)")
        return got.astype(bool)

    def near_surfaces(self, points, K: int = 4, reach=np.inf, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False) -> dict:
        """The K nearest surfaces within `reach` of every point (arguments as ``nearest_surface``) -> {"d": float32 [K, n], "id": uint32 [K, n]}:
        entry k of point i at [k, i], ordered by (d, id word), every primitive at most once, entries past a point's candidates {inf,
        api.ID_NONE}.  K is 1..8; there is no total count: a full K-th row means "ask for more"."""
        got = self.w.near_surfaces(api.make_probes(points, reach), api.cast_flags(kinds, opaque_only), K, ignore)
        if got is None:
            raise RuntimeError("the proximity query was refused (at least one point, at least one kind, K in 1..8?)")
        return got

    @staticmethod
    def _address(buffer):
        """the device address of a torch tensor (``data_ptr()``), or the integer address itself; None stays None"""
        return buffer if buffer is None else int(buffer.data_ptr() if hasattr(buffer, "data_ptr") else buffer)

    def probe_device(self, probes, n: int, hits=None, within=None, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False) -> int:
        """The nearest-surface or the within-reach query over the caller's device memory -- torch tensors or integer device addresses: n
        api.PROBE records in (float32 [n, 4]: point, reach), optionally n uint32 ignore words, n api.HIT records (`hits`: float32 [n, 8]) or n
        bytes (`within`) out -- exactly one of the two.  Launched on the wrapper's stream (``w.set_stream``) without waiting -> n."""
        got = self.w.probe_device(self._address(probes), n, api.cast_flags(kinds, opaque_only), self._address(ignore), self._address(hits),
                                  self._address(within))
        if got != n:
            raise RuntimeError("the proximity query was refused (at least one point, at least one kind, exactly one of hits and within?)")
        return got

    def near_surfaces_device(self, probes, n: int, K: int, d, ids, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False) -> int:
        """The K-nearest query over the caller's device memory (torch tensors or integer device addresses): n api.PROBE records in, K * n floats
        and K * n id words out, layer-major.  Launched on the wrapper's stream without waiting -> n."""
        got = self.w.near_surfaces_device(self._address(probes), n, api.cast_flags(kinds, opaque_only), K, self._address(d), self._address(ids),
                                          self._address(ignore))
        if got != n:
            raise RuntimeError("the proximity query was refused (at least one point, at least one kind, K in 1..8, all three addresses?)")
        return got

    def touching_spheres(self, margin: float = 0.0, K: int = 8):
        """Which spheres of the scene touch each other (or come within `margin`)?  Probe i sits at sphere i's centre, reaches |r_i| + margin
        (float32) and ignores sphere i; only spheres take part -> (id uint32 [K, ns], gap float32 [K, ns]): the up to K spheres nearest to
        sphere i's surface in order, gap = their distance from it (d - |r_i|, float32; negative = they overlap), empty entries {api.ID_NONE,
        inf}.  A full K-th row means "ask for more"."""
        s = self.scene.spheres
        r = np.abs(s["radius"].astype(np.float32))
        got = self.near_surfaces(s["origin"], K, reach=r + np.float32(margin), ignore=np.arange(len(s), dtype=np.uint32), kinds=("sphere",))
        return got["id"], got["d"] - r[None, :]

    # ---- layered ray queries
    def cast_layers(self, origins, dirs, K: int = 4, tmax=np.inf, ignore=None, kinds=("sphere", "plane"), opaque_only: bool = False) -> dict:
        """The K nearest surfaces of every ray (arguments as ``cast_rays``) -> {"t": float32 [K, n], "id": uint32 [K, n]}: layer k of ray i at
        [k, i], ordered by (t, id word), every primitive at most once, entries past a ray's candidates {inf, api.ID_NONE}.  K is 1..8; there
        is no total count: ask for K + 1 to learn whether there is more."""
        got = self.w.cast_layers(api.make_rays(origins, dirs, tmax, ignore), api.cast_flags(kinds, opaque_only), K)
        if got is None:
            raise RuntimeError("the layered ray query was refused (at least one ray, at least one kind, K in 1..8?)")
        return got

    def cast_layers_device(self, rays_ptr: int, n: int, K: int, t_ptr: int, id_ptr: int, kinds=("sphere", "plane"), opaque_only: bool = False) -> int:
        """The layered query over the caller's device memory, by integer device address: n api.RAY_QUERY records in, K * n floats and K * n id
        words out, layer-major.  Launched on the wrapper's stream (``w.set_stream``) without waiting -> n."""
        got = self.w.cast_layers_device(rays_ptr, n, api.cast_flags(kinds, opaque_only), K, t_ptr, id_ptr)
        if got != n:
            raise RuntimeError("the layered ray query was refused (at least one ray, at least one kind, K in 1..8, all three addresses?)")
        return got

    def camera_rays(self) -> np.ndarray:
        """The rays of this renderer's pixels through the camera set last, under the camera model, as query rays -> api.RAY_QUERY [pixels]
        (tmax = inf, ignore = api.ID_NONE): what ``cast_rays`` / ``cast_layers`` take.  Not available with row bands."""
        self._latch_camera()
        got = self.w.camera_rays(self.pixels)
        if got is None or got.size != self.pixels:
            raise RuntimeError("the camera rays were refused (a camera set? no row bands? a projection that resolves?)")
        return got

    def layers(self, K: int = 4, kinds=("sphere", "plane"), opaque_only: bool = False) -> dict:
        """What lies behind every pixel, in depth order -> {"t": float32 [K, rows, width], "id": uint32 [K, rows, width]}: the K nearest surfaces
        along the pixel's camera ray (``camera_rays()`` through ``cast_layers``, both on the device).  Layer 0 is what ``gbuffer()`` sees where
        the kinds agree; t is in units of the ray's direction (unit for the pinhole and the panorama)."""
        self._latch_camera()
        if self.w.render_layers(api.cast_flags(kinds, opaque_only), K) != self.pixels:
            raise RuntimeError("the layers pass was refused (a camera set? at least one kind, K in 1..8, no row bands?)")
        shape = (int(K), self.rows, self.width)
        return {"t": self.w.read_layers(api.LAYERS_T).reshape(shape), "id": self.w.read_layers(api.LAYERS_ID).reshape(shape)}

    def pick_through(self, x: int, y: int, K: int = 8, kinds=("sphere", "plane"), opaque_only: bool = False) -> list | None:
        """Everything under pixel (x, y) of the frame, nearest first -> a list of {"id", "kind", "index", "depth"} of at most K entries (click
        again to select the object behind: the next entry), empty where the ray meets nothing; None when the pixel is not one of this
        renderer's rows (or no camera has been set)."""
        self._latch_camera()
        got = self.w.pick_layers(x, y, api.cast_flags(kinds, opaque_only), K)
        if got is None:
            return None
        return [api.id_entry(e["id"], depth=np.float32(e["t"])) for e in got if int(e["id"]) != api.ID_NONE]

    # ---- path queries
    def cast_paths(self, origins, dirs, bounces: int = 4, transmit: bool = False, all_surfaces: bool = False, tmax=np.inf, ignore=None,
                   kinds=("sphere", "plane", "light"), opaque_only: bool = False) -> dict:
        """Where every ray GOES (arguments as ``cast_rays``; dirs should be unit: the refraction rule takes them for unit) -> {"t", "id",
        "normal", "point"} as [bounces, n] arrays (normal and point [bounces, n, 3]): segment 0 is ``cast_rays`` of the ray, segment k + 1 the
        hit of the reference's reflected ray -- with `transmit`, through a transparent surface, of its refracted ray -- from segment k's hit;
        "count" [n]: the hits recorded, entries past it are misses; "reason" [n]: api.PATH_REASON_BOUNCES (all `bounces` recorded),
        _MISSED (the last ray met nothing) or _ENDED (on a light, or on a surface that is neither reflective, dielectric nor transparent --
        `all_surfaces` reflects off those too); "next" api.RAY_QUERY [n]: the ray the path would go on with (after _MISSED the ray that
        missed: look the sky up with it; after _ENDED a zero direction).  One launch whatever `bounces` (1..8) is; tmax bounds each segment."""
        got = self.w.cast_paths(api.make_rays(origins, dirs, tmax, ignore), api.path_flags(kinds, opaque_only, transmit, all_surfaces), bounces)
        if got is None:
            raise RuntimeError("the path query was refused (at least one ray, at least one kind, bounces in 1..8?)")
        return got

    def cast_paths_device(self, rays_ptr: int, n: int, hits_ptr: int, status_ptr: int, next_ptr: int | None = None, bounces: int = 4,
                          transmit: bool = False, all_surfaces: bool = False, kinds=("sphere", "plane", "light"), opaque_only: bool = False) -> int:
        """The path query over the caller's device memory, by integer device address (``tensor.data_ptr()``): n api.RAY_QUERY records in,
        bounces * n api.HIT records (segment-major), n status bytes and, if `next_ptr` is given, n api.RAY_QUERY records out.  Launched on the
        wrapper's stream (``w.set_stream``) without waiting -> n."""
        got = self.w.cast_paths_device(rays_ptr, n, api.path_flags(kinds, opaque_only, transmit, all_surfaces), bounces, hits_ptr, status_ptr, next_ptr)
        if got != n:
            raise RuntimeError("the path query was refused (at least one ray, at least one kind, bounces in 1..8, the three addresses?)")
        return got

    def pick_path(self, x: int, y: int, bounces: int = 4, transmit: bool = False) -> list | None:
        """What pixel (x, y) of the frame shows and what shows in THAT: the objects along the path of the pixel's camera ray -> a list of
        {"id", "kind", "index", "depth", "point", "normal"} of at most `bounces` entries -- the first is what ``pick(x, y)`` answers (a light
        behind a transparent sphere aside: the path meets the sphere), the second the object reflected in it (with `transmit`: seen through
        it), ...; depth is the segment's t, point the point shading uses (moved by EPSILON along the normal, where the next segment starts).
        Empty where the ray meets nothing; None when the pixel is not one of this renderer's rows (or no camera has been set)."""
        self._latch_camera()
        got = self.w.pick_path(x, y, bounces, api.path_flags(transmit=transmit))
        if got is None:
            return None
        hits, status = got
        return [api.id_entry(h["id"], depth=np.float32(h["t"]), point=h["point"] + h["normal"] * api.PATH_EPSILON, normal=h["normal"].copy())
                for h in hits[:status & 15]]

    # ---- the visible-object table
    def objects(self, rect=None) -> np.ndarray:
        """Which objects show inside `rect` = (x, y, width, height) in frame pixels (None = the whole frame) on this renderer's rows, through the
        camera set last -> api.OBJECT_STAT [objects], sorted by id: id, pixels, the inclusive bounding box x0, y0, x1, y1 in frame coordinates,
        depth_min, depth_max, and sum_x, sum_y (centroid = sum / pixels).  Reduced on the device: only the records travel."""
        self._latch_camera()
        got = self.w.object_stats(rect)
        if got is None:
            raise RuntimeError("the visible-object table was refused (a camera set? a rectangle of at least one pixel? no row bands?)")
        return got[0]

    def select_rect(self, x0: int, y0: int, x1: int, y1: int, *, min_pixels: int = 1, kinds=(api.ID_SPHERE, api.ID_PLANE)) -> np.ndarray:
        """Rubber-band selection: the ids of the objects of `kinds` that show at least `min_pixels` pixels inside the inclusive rectangle
        (x0, y0) .. (x1, y1) of the frame (the corners in either order) -> uint32 [<= 64], largest first, ties by id: what ``highlight`` takes."""
        xa, xb, ya, yb = min(int(x0), int(x1)), max(int(x0), int(x1)), min(int(y0), int(y1)), max(int(y0), int(y1))
        if xa < 0 or ya < 0:
            raise RuntimeError("the visible-object table was refused (a rectangle with a negative corner)")
        t = self.objects((xa, ya, xb - xa + 1, yb - ya + 1))
        t = t[np.isin(api.id_kind(t["id"]), np.asarray(kinds, np.uint32).reshape(-1)) & (t["id"] != api.ID_NONE) & (t["pixels"] >= min_pixels)]
        order = np.lexsort((t["id"], -t["pixels"].astype(np.int64)))
        return np.ascontiguousarray(t["id"][order][:64], np.uint32)

    def read_rays(self) -> np.ndarray:
        """The 64-B rray records of buffers[0][8] (materialised on demand in fused mode)."""
        rays = np.empty((self.pixels, 16), np.float32)
        self.w.output(self.pixels, rays.nbytes, 0, 0, 8, rays)
        return rays

    def release(self):
        self.w.release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
