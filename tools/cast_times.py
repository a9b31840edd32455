"""Kernel time of the ray queries (clw_ext_cast_rays_device: wt_cast), with what there is to compare them with beside them (clw_ext_timing_*;
one process, launches back to back on device memory).
   python tools/cast_times.py [--frames N] [--repeats R] [--baseline] [--batches] [--out FILE]
   The demo scene and the 10 000-sphere scene, 1920 x 1080 = 2 073 600 rays, both builds, nearest and any, spheres and planes:
     (a) the camera's own rays in pixel order (the records of read_rays() as clw_ray);
     (b) the same rays under one fixed permutation (incoherent: neighbouring lanes look anywhere);
     (c) short rays from the primary-hit pass's points along its normals, tmax = 1, each ignoring the primitive it starts on.
   Beside them: the primary-hit pass with depth + id + normal + point (the same search for (a), without reading a ray); a device-to-device copy
   of the 64 MB ray array (the traffic a query adds); and the route without the feature, clw_ext_unit_scene op 0 on the same rays, host arrays
   and round trip included (wall clock, one call).
   Every kernel figure is the median (min .. max) of R repeats of N launches after two warm-up launches.
   --batches: (a) and (c) on the demo scene and on a 256-sphere scene, nearest, with 1, 2, 4, 8 and 16 batches of 64 rays per staging (CLWRAP_CAST_BATCHES): what
   launch_plan.h's WT_CAST_BATCHES_LDS was chosen from.
   --baseline: the depth-1 and depth-4 trace launches alone -- nothing of the feature is called, so the run also works against a library built
   from the parent commit (CLWRAP_LIB=<its .so>): the feature unused must cost what the parent costs, inside the spread printed here."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before the shim is loaded: both then share the ROCm runtime torch ships)
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import api, scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", action="store_true")
ap.add_argument("--batches", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
W, H = 1920, 1080
N = W * H
SCENES = (("demo", scene.render_map_scene, pkg.CAMERA_RAYPNG),
          ("10k", lambda: scene.sphere_grid_scene(100, 100), dict(origin=(0.0, 12.0, -10.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)))
FLAGS = api.CAST_SPHERES | api.CAST_PLANES
lines = []


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def repeats(r, launch, tid):
    """R repeats of N launches -> (median, min, max) ms per logged launch of timing id `tid`"""
    launch(); launch()
    ms = []
    for _ in range(a.repeats):
        r.w.timing_reset()
        for _ in range(a.frames):
            launch()
        r.w.sync()
        n, total = r.w.timing_get(tid)
        assert n == a.frames, (tid, n)
        ms.append(total / n)
    return stats(ms)


def say(text):
    lines.append(text)
    print(text, flush=True)


def row(name, what, v):
    say(f"{name:<4} | {what:<64} | {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})")


def device(arr):
    return torch.from_numpy(np.frombuffer(arr.tobytes(), np.uint8).copy()).cuda()


def ray_sets(r):
    """(a), (b), (c) as api.RAY_QUERY arrays, from the renderer's own rays and primary-hit pass"""
    rec = r.read_rays()
    camera = api.make_rays(rec[:, 0:3], rec[:, 4:7])
    g = r.gbuffer(api.GB_POINT | api.GB_NORMAL | api.GB_ID)
    short = api.make_rays(g["point"], g["normal"], tmax=1.0, ignore=g["id"])
    return (("(a) camera rays, pixel order", camera), ("(b) camera rays, permuted", camera[np.random.default_rng(1).permutation(N)]),
            ("(c) short rays off the surfaces, tmax 1", short))


say(f"# tools/cast_times.py{' --baseline' if a.baseline else ''}{' --batches' if a.batches else ''}: median (min .. max) of {a.repeats} x {a.frames} "
    f"launches, {N} rays ({W}x{H}); kernels {api.kernel_source_hash()}")
say("# scene | launch | ms")
if a.baseline:
    for name, make, cam in SCENES:
        sc = make()
        for depth in (1, 4):
            r = Renderer(sc, tex, sky, W, H, depth=depth)
            r.look(**cam)
            r.w.set_async(1)
            row(name, f"trace, depth {depth}", repeats(r, lambda: r.render(readback=False), 1))
            r.release()
elif a.batches:
    # the demo scene (16 float4 staged) and 256 spheres (the most the LDS flavour ever stages: 4.2 KiB)
    for name, make, cam in (SCENES[0], ("256", lambda: scene.sphere_grid_scene(16, 16), SCENES[1][2])):
        sc = make()
        for batches in (1, 2, 4, 8, 16):
            os.environ["CLWRAP_CAST_BATCHES"] = str(batches)
            r = Renderer(sc, tex, sky, W, H, depth=1)
            r.look(**cam)
            r.render(readback=False)
            sets = ray_sets(r)
            r.w.set_async(1)
            d_hits = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
            for what, rays in (sets[0], sets[2]):
                d_rays = device(rays)
                torch.cuda.synchronize()
                row(name, f"fast nearest {what}, {batches:>2} batches per staging",
                    repeats(r, lambda: r.w.cast_rays_device(d_rays.data_ptr(), N, FLAGS, hits_ptr=d_hits.data_ptr()), api.TIMING_CAST))
            r.release()
        os.environ.pop("CLWRAP_CAST_BATCHES")
else:
    for name, make, cam in SCENES:
        sc = make()
        for strict in (False, True):
            build = "strict" if strict else "fast"
            r = Renderer(sc, tex, sky, W, H, depth=1, strict=strict)
            r.look(**cam)
            r.render(readback=False)
            sets = ray_sets(r)
            r.w.set_async(1)
            gb = api.GB_DEPTH | api.GB_ID | api.GB_NORMAL | api.GB_POINT

            def primary():
                assert r.w.render_gbuffer(gb) == N
            row(name, f"{build} primary-hit pass, depth + id + normal + point (32 B/px)", repeats(r, primary, api.TIMING_GBUFFER))
            d_hits = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
            d_blocked = torch.empty(N, dtype=torch.uint8, device="cuda")
            for what, rays in sets:
                d_rays = device(rays)
                torch.cuda.synchronize()
                row(name, f"{build} nearest {what}", repeats(r, lambda: r.w.cast_rays_device(d_rays.data_ptr(), N, FLAGS, hits_ptr=d_hits.data_ptr()), api.TIMING_CAST))
                row(name, f"{build} any     {what}", repeats(r, lambda: r.w.cast_rays_device(d_rays.data_ptr(), N, FLAGS, blocked_ptr=d_blocked.data_ptr()), api.TIMING_CAST))
                if strict and what.startswith("(a)"):
                    hit = d_hits.cpu().numpy().view(api.HIT)
                    say(f"{name:<4} | (a): {float((hit['id'] != api.ID_NONE).mean()):.4f} of the rays hit; blocked {float(d_blocked.cpu().numpy().mean()):.4f}")
            if not strict:
                # the traffic a query adds: the 64 MB ray array, device to device
                d_rays, d_copy = device(sets[0][1]), torch.empty(N * 32, dtype=torch.uint8, device="cuda")
                ms = []
                for _ in range(a.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(a.frames):
                        d_copy.copy_(d_rays)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1) / a.frames)
                row(name, "device-to-device copy of the ray array (64 MB read, 64 MB written)", stats(ms))
                # the route without the feature: host arrays in, 22 floats per ray out, waits
                rows6 = np.ascontiguousarray(np.concatenate([sets[0][1]["origin"], sets[0][1]["dir"]], 1))
                r.w.sync()
                r.w.unit_scene(0, rows6[:4096], 22)
                t0 = time.perf_counter()
                r.w.unit_scene(0, rows6, 22)
                say(f"{name:<4} | {build} clw_ext_unit_scene op 0 on (a), host arrays, round trip (wall clock, 1 call) | {(time.perf_counter() - t0) * 1e3:.1f}")
                t0 = time.perf_counter()
                r.w.cast_rays(sets[0][1], FLAGS)
                say(f"{name:<4} | {build} clw_ext_cast_rays on (a), host arrays, round trip (wall clock, 1 call)       | {(time.perf_counter() - t0) * 1e3:.1f}")
            r.release()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
