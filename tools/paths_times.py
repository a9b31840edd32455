"""Kernel time of the path queries (clw_ext_cast_paths_device: wt_cast_paths) beside the route that existed before them -- B successive
nearest-hit casts (clw_ext_cast_rays_device) with a bounce step in torch between them -- in one session, on the same rays, on device memory.
   python tools/paths_times.py [--frames N] [--repeats R] [--strict] [--out FILE]
   The demo scene and the 10 000-sphere scene, 1920 x 1080 = 2 073 600 camera rays (clw_ext_camera_rays_device's own output), in pixel order
   and under one fixed permutation; spheres and planes, every surface reflecting (CLW_PATH_ALL_SURFACES), so that both routes follow the same
   paths: a path ends where its ray meets nothing.  For B = 1, 2, 4, 8:
     - wt_cast_paths, one launch: the wrapper's own timer (clw_ext_timing_*: the kernel alone) and, like the other route, torch events around
       the call on torch's stream;
     - B x (wt_cast nearest, then the reflected rays built by torch: about ten small kernels), torch events around the whole sequence;
     - their ratio.  B = 1 stands beside wt_cast's nearest query of the same rays: the same scan, plus the status byte, the outgoing ray (32
       more bytes written per ray) and the material gather.
   Both routes run on ONE stream (a torch stream the wrapper is given with clw_ext_set_stream), so the events bracket all of a route's work.
   Every figure is the median (min .. max) of R repeats of N launches (sequences) after two warm-up ones."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before the shim is loaded: both then share the ROCm runtime torch ships)
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import api, scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--strict", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
W, H = 1920, 1080
N = W * H
SCENES = (("demo", scene.render_map_scene, pkg.CAMERA_RAYPNG),
          ("10k", lambda: scene.sphere_grid_scene(100, 100), dict(origin=(0.0, 12.0, -10.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)))
CAST = api.CAST_SPHERES | api.CAST_PLANES
PATH = CAST | api.PATH_ALL_SURFACES
EPS = float(api.PATH_EPSILON)
lines = []


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def by_timer(r, launch, tid):
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


def by_events(run):
    """R repeats of N runs -> (median, min, max) ms per run between two torch events on the current stream"""
    run(); run()
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.frames):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.frames)
    return stats(ms)


def say(text):
    lines.append(text)
    print(text, flush=True)


def fmt(v):
    return f"{v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})"


def bounce(rays, hits):
    """the reflected rays of `hits` into `rays` (both float32 [N, 8] views of the records): what a caller wrote between two casts"""
    n, p, d = hits[:, 2:5], hits[:, 5:8], rays[:, 4:7]
    hit = (hits[:, 1].view(torch.int32) != -1).unsqueeze(1)
    out = torch.where(hit, d + n * (2 * -(n * d).sum(1, keepdim=True)), torch.zeros_like(d))
    rays[:, 0:3] = p + n * EPS
    rays[:, 4:7] = out
    rays[:, 7].view(torch.int32).fill_(-1)


build = "strict" if a.strict else "fast"
say(f"# tools/paths_times.py{' --strict' if a.strict else ''}: median (min .. max) of {a.repeats} x {a.frames} launches, {N} rays ({W}x{H}), "
    f"{build} build; kernels {api.kernel_source_hash()}")
say("# scene | rays | B | wt_cast_paths, one launch: kernel ms (wrapper timer) | the same, torch events | B x (wt_cast nearest + torch bounce), torch events | B launches / one launch")
stream = torch.cuda.Stream()      # one stream for both routes: the wrapper launches on it, torch's kernels and events are queued on it
torch.cuda.set_stream(stream)
for name, make, cam in SCENES:
    sc = make()
    r = Renderer(sc, tex, sky, W, H, depth=1, strict=a.strict)
    r.look(**cam)
    r.render(readback=False)
    r.w.set_async(1)
    r.w.set_stream(stream.cuda_stream)
    d_cam = torch.empty(N * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert r.w.camera_rays_device(d_cam.data_ptr(), N) == N
    r.w.sync()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(N)).cuda()
    d_perm = d_cam.view(N, 8)[perm].contiguous().view(-1)
    d_work = torch.empty(N * 8, dtype=torch.float32, device="cuda")
    d_hits = torch.empty(8 * N * 8, dtype=torch.float32, device="cuda")
    d_status = torch.empty(N, dtype=torch.uint8, device="cuda")
    d_next = torch.empty(N * 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for what, d_rays in (("pixel order", d_cam), ("permuted", d_perm)):
        near = by_timer(r, lambda: r.w.cast_rays_device(d_rays.data_ptr(), N, CAST, hits_ptr=d_hits.data_ptr()), api.TIMING_CAST)
        say(f"{name:<4} | {what} | - | wt_cast nearest: {fmt(near)} | | |")
        for B in (1, 2, 4, 8):
            def one():
                assert r.w.cast_paths_device(d_rays.data_ptr(), N, PATH, B, d_hits.data_ptr(), d_status.data_ptr(), d_next.data_ptr()) == N

            def many():
                d_work.copy_(d_rays)
                for k in range(B):
                    layer = d_hits[k * N * 8:(k + 1) * N * 8]
                    r.w.cast_rays_device(d_work.data_ptr(), N, CAST, hits_ptr=layer.data_ptr())
                    bounce(d_work.view(N, 8), layer.view(N, 8))
            kernel = by_timer(r, one, api.TIMING_PATHS)
            single = by_events(one)
            chain = by_events(many)
            say(f"{name:<4} | {what} | {B} | {fmt(kernel)} | {fmt(single)} | {fmt(chain)} | {chain[0] / single[0]:.2f}"
                + (f" | B = 1 / wt_cast nearest: {kernel[0] / near[0]:.2f}" if B == 1 else ""))
        count = (d_status & 15).float()
        say(f"{name:<4} | {what}: hits recorded per path at B = 8: mean {float(count.mean()):.2f}, {float((count == 8).float().mean()):.4f} of the paths reach 8")
    r.w.set_stream(0)
    r.release()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
