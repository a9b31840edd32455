"""Time one BASELINE.json configuration through the C-ABI (kernel-only, frames back to back) and print JSON.
   python tools/run_config.py c2|c3|c4|c5strip|ref800 [--strict 1] [--frames N] [--variant V] [--depth D] [--size WxH] [--supersample N] [--aperture A --focus F | --copies] [--motion move|equal] [--no-tail] [--accumulate N [--no-jitter]]
   --supersample N: n x n samples per pixel resolved in the kernel (the frame stays WxH); --size: another frame size for the configuration's
   scene and camera -- e.g. the n*W x n*H frame a supersampled launch traces, to time the same work without the resolve.
   --aperture A --focus F: a thin lens over the samples (clw_ext_set_lens); --copies: an explicit table of n*n copies of the launch camera
   (clw_ext_set_sample_cameras) -- the plain supersampled image through the table path, to time the mechanism alone.
   --motion move: every third sphere of the scene moves by (0.5, 0, -0.3) while the shutter is open (clw_ext_set_sphere_motion); --motion equal:
   the same table with every sample time 0.5 -- the per-test fma and table read without the extra divergence; --no-tail: the tree-parallel tail
   off (clw_ext_set_tpt), as a moving deep launch runs.
   --accumulate N [--no-jitter]: progressive accumulation over N frames (clw_ext_set_accumulate), every frame with its own seeds and, unless
   --no-jitter, sub-pixel offset; the sum starts again before every timed loop, so N >= --frames times launches that all trace (a converged
   view issues none).
   --repeats R: the N-frame loop R times (0 = until 50 ms have been timed, as bench.py --full does), median / min / max of the repeats."""
import argparse, json, math, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("config")
ap.add_argument("--strict", type=int, default=0)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--variant", type=int, default=0)
ap.add_argument("--depth", type=int, default=None)
ap.add_argument("--png", default=None)
ap.add_argument("--size", default=None)
ap.add_argument("--supersample", type=int, default=1)
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--aperture", type=float, default=0.0)
ap.add_argument("--focus", type=float, default=1.0)
ap.add_argument("--copies", action="store_true")
ap.add_argument("--motion", choices=["move", "equal"], default=None)
ap.add_argument("--no-tail", action="store_true")
ap.add_argument("--accumulate", type=int, default=0)
ap.add_argument("--no-jitter", action="store_true")
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
cam = pkg.CAMERA_RAYPNG
kw = {}
if a.config == "c2":
    sc, W, H, depth = scene.render_map_scene(), 1920, 1080, 4
elif a.config == "c3":      # 4096x4096 depth 8, 64 dielectric spheres (divergence stress)
    sc, W, H, depth = scene.dielectric_field_scene(8), 4096, 4096, 8
    cam = dict(origin=(3.5, 3.0, -6.0), look=(0.0, -2.5, 9.5), fov=90.0, focal=1.0)
elif a.config == "c4":      # 10k-sphere grid, 1920x1080 depth 4 (geometry streamed, not LDS/SGPR resident)
    sc, W, H, depth = scene.sphere_grid_scene(100, 100), 1920, 1080, 4
    cam = dict(origin=(0.0, 12.0, -10.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)
elif a.config == "c5strip":  # one GPU's 8192x1024 strip of the 8192x8192 frame (rank 3 of 8)
    sc, W, H, depth = scene.render_map_scene(), 8192, 8192, 4
    kw = dict(first_row=3 * 1024, rows=1024)
elif a.config == "ref800":  # the reference driver's own configuration: 800x600, depth 15
    sc, W, H, depth = scene.render_map_scene(), 800, 600, 15
else:
    raise SystemExit("unknown config")
depth = a.depth or depth
if a.size:
    W, H = (int(v) for v in a.size.lower().split("x"))
if a.supersample != 1:
    kw["supersample"] = a.supersample
if a.accumulate:
    if a.accumulate < a.frames:
        raise SystemExit("--accumulate N needs N >= --frames: a converged view issues no launch to time")
    kw.update(accumulate=a.accumulate, jitter=not a.no_jitter)
r = Renderer(sc, tex, sky, W, H, depth=depth, strict=bool(a.strict), **kw)
r.w.set_variant(a.variant)
camera = r.look(**cam)
if a.aperture:
    r.w.set_lens(a.aperture, a.focus)
elif a.copies:
    r.set_sample_cameras(np.tile(np.concatenate([np.asarray(v, np.float32) for v in (camera.im_corner, camera.origin, camera.up, camera.right)]), (a.supersample ** 2, 1)))
if a.motion:
    disp = np.zeros((len(sc.spheres), 3), np.float32)
    disp[1::3] = (0.5, 0.0, -0.3)
    r.set_sphere_motion(disp, np.full(a.supersample ** 2, 0.5, np.float32) if a.motion == "equal" else None)
if a.no_tail:
    r.w.set_tpt(max_lanes=0)
r.render(readback=False); r.render(readback=False)
r.w.enable_counters(1); r.render(readback=False); c = r.w.read_counters(); r.w.enable_counters(0)
r.w.set_async(1)
kms, walls, reps = [], [], a.repeats
while len(kms) < max(reps, 1):
    if a.accumulate:
        r.reset_accumulation()
    r.w.timing_reset()
    t = time.perf_counter()
    for _ in range(a.frames):
        r.render(readback=False)
    r.w.sync()
    walls.append((time.perf_counter() - t) / a.frames)
    n, ms = r.w.timing_get(1)
    kms.append(ms / n)
    if reps == 0:
        reps = min(200, max(1, math.ceil(0.05 / max(walls[0] * a.frames, 1e-6))))
wall, ms, n = statistics.median(walls), statistics.median(kms), 1
r.w.set_async(0)
img = r.render()
rays = c["segments"] + c["shadow_rays"]
px = r.pixels
print(json.dumps(dict(config=a.config, frame=f"{W}x{H}", pixels=px, depth=depth, strict=a.strict, variant=a.variant, supersample=a.supersample, aperture=a.aperture, focus=a.focus, copies=int(a.copies), motion=a.motion, no_tail=int(a.no_tail), accumulate=a.accumulate, jitter=int(not a.no_jitter), kernel_ms=round(ms / n, 4),
                      kernel_ms_min=round(min(kms), 4), kernel_ms_max=round(max(kms), 4), repeats=len(kms),
                      wall_ms_per_frame=round(wall * 1e3, 4), rays_per_px=round(rays / px, 3), Mrays_s=round(rays / (ms / n) / 1e3, 1),
                      lane_util=round(c["lane_iters"] / max(c["wave_iters_x64"], 1), 4), counters=c)), flush=True)
if a.png:
    from example_gui_opencl_raytracer_amd import api
    api.write_png(a.png, img, W, r.rows)
r.release()
