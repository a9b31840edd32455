"""Kernel time of the layered ray queries (clw_ext_cast_layers_device: wt_cast_layers; clw_ext_camera_rays_device: wt_camera_rays), with the
nearest-hit query of the same session on the same rays beside every figure (clw_ext_timing_*; one process, launches back to back on device
memory).
   python tools/layers_times.py [--frames N] [--repeats R] [--strict] [--out FILE]
   The demo scene and the 10 000-sphere scene, 1920 x 1080 = 2 073 600 camera rays (clw_ext_camera_rays_device's own output), in pixel order
   and under one fixed permutation, spheres and planes:
     - wt_cast nearest on those rays: the yardstick;
     - wt_cast_layers at K = 1, 2, 4, 8 -- K <= 4 once with the C = 4 kernel (what a call runs) and once with the C = 8 kernel
       (CLWRAP_LAYERS_CAPACITY=8) --, each with its ratio to the yardstick and, beside it, the cost of K peeled nearest casts (K x the
       yardstick, launches only: the K - 1 round trips that rebuild the rays are not counted);
     - wt_camera_rays beside a device-to-device copy of the same 64 MB.
   Every kernel figure is the median (min .. max) of R repeats of N launches after two warm-up launches."""
import argparse, os, statistics, sys
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
ap.add_argument("--strict", action="store_true")
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


def fmt(v):
    return f"{v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})"


build = "strict" if a.strict else "fast"
say(f"# tools/layers_times.py{' --strict' if a.strict else ''}: median (min .. max) of {a.repeats} x {a.frames} launches, {N} rays ({W}x{H}), "
    f"{build} build; kernels {api.kernel_source_hash()}")
say("# scene | launch | ms | ratio to the nearest-hit cast of the same rays | K peeled nearest casts, ms")
for name, make, cam in SCENES:
    sc = make()
    r = Renderer(sc, tex, sky, W, H, depth=1, strict=a.strict)
    r.look(**cam)
    r.render(readback=False)
    r.w.set_async(1)
    d_cam = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def camera():
        assert r.w.camera_rays_device(d_cam.data_ptr(), N) == N
    v = repeats(r, camera, api.TIMING_CAMRAYS)
    say(f"{name:<4} | wt_camera_rays, 64 MB written | {fmt(v)}")
    d_copy = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.frames):
            d_copy.copy_(d_cam)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.frames)
    say(f"{name:<4} | device-to-device copy of the ray array (64 MB read, 64 MB written) | {fmt(stats(ms))}")
    perm = torch.from_numpy(np.random.default_rng(1).permutation(N)).cuda()
    d_perm = d_cam.view(N, 32)[perm].contiguous().view(-1)
    d_hits = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
    d_t = torch.empty(8 * N, dtype=torch.float32, device="cuda")
    d_id = torch.empty(8 * N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for what, d_rays in (("pixel order", d_cam), ("permuted", d_perm)):
        near = repeats(r, lambda: r.w.cast_rays_device(d_rays.data_ptr(), N, FLAGS, hits_ptr=d_hits.data_ptr()), api.TIMING_CAST)
        say(f"{name:<4} | wt_cast nearest, camera rays {what} | {fmt(near)} | 1.00 |")
        for K in (1, 2, 4, 8):
            for capacity in ((4, 8) if K <= 4 else (8,)):
                os.environ["CLWRAP_LAYERS_CAPACITY"] = str(capacity)
                v = repeats(r, lambda: r.w.cast_layers_device(d_rays.data_ptr(), N, FLAGS, K, d_t.data_ptr(), d_id.data_ptr()), api.TIMING_LAYERS)
                say(f"{name:<4} | wt_cast_layers K = {K}, C = {capacity}, camera rays {what} | {fmt(v)} | {v[0] / near[0]:.2f} | {K * near[0]:.4f}")
        os.environ.pop("CLWRAP_LAYERS_CAPACITY")
        listed = (d_id.view(8, N) != -1).sum(0)
        say(f"{name:<4} | camera rays {what}: listed candidates per ray among the first 8: mean {float(listed.float().mean()):.2f}, "
            f"{float((listed == 8).float().mean()):.4f} of the rays fill all 8")
    r.release()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
