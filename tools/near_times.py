"""Kernel time of the proximity queries (clw_ext_probe_device, clw_ext_near_surfaces_device: wt_near), with what there is to compare them with
beside them (clw_ext_timing_*; one process, launches back to back on device memory).
   python tools/near_times.py [--frames N] [--repeats R] [--cap-sweep] [--out FILE]
   The demo scene and the 10 000-sphere scene, 1920 x 1080 = 2 073 600 probes: the points of the primary-hit pass of the view (a pixel that
   sees the sky probes the origin), reaching 0.5, 1 and 2 mean sphere radii, in pixel order and under one fixed permutation; fast build; spheres
   and planes; nearest, within, and the K = 1 / 4 / 8 nearest.
   Beside them, in the same session: wt_cast's nearest query of the camera's 2 073 600 rays on the same scene, and the route without the
   feature in torch -- cdist of the points to the sphere centres minus the radii, then min (nearest) or topk (K = 8), in chunks of probes
   where the n x ns matrix does not fit (spheres only: it knows no planes).
   Every figure is the median (min .. max) of R repeats of N launches after two warm-up launches.
   --cap-sweep: the 10 000-sphere scene, nearest and K = 8, pixel order, every reach, under CLWRAP_NEAR_BOX_CELLS = 0, 8, 27, 64, 125, 216,
   512, 1000, 4096 and 2^30: what launch_plan.h's WT_NEAR_BOX_CELLS is chosen from."""
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
ap.add_argument("--cap-sweep", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
W, H = 1920, 1080
N = W * H
SCENES = (("demo", scene.render_map_scene, pkg.CAMERA_RAYPNG),
          ("10k", lambda: scene.sphere_grid_scene(100, 100), dict(origin=(0.0, 12.0, -10.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)))
FLAGS = api.CAST_SPHERES | api.CAST_PLANES
REACHES = (0.5, 1.0, 2.0)
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


def torch_repeats(launch):
    launch(); launch()
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def say(text):
    lines.append(text)
    print(text, flush=True)


def row(name, what, v):
    say(f"{name:<4} | {what:<72} | {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})")
    return v[0]


def device(arr):
    return torch.from_numpy(np.frombuffer(arr.tobytes(), np.uint8).copy()).cuda()


def torch_route(points, centres, radii, K):
    """the n x ns distance matrix in chunks of at most 2^28 entries: nearest (K = 0: min) or the K nearest (topk)"""
    chunk = max(1, (1 << 28) // max(len(centres), 1))
    out = []
    for b in range(0, len(points), chunk):
        d = torch.cdist(points[b:b + chunk], centres) - radii[None, :]
        out.append(d.min(1) if K == 0 else torch.topk(d, K, dim=1, largest=False))
    return out


say(f"# tools/near_times.py{' --cap-sweep' if a.cap_sweep else ''}: median (min .. max) of {a.repeats} x {a.frames} launches, {N} probes ({W}x{H}); "
    f"kernels {api.kernel_source_hash()}")
say("# scene | launch | ms")
for name, make, cam in (SCENES[1:] if a.cap_sweep else SCENES):
    sc = make()
    rbar = float(np.abs(sc.spheres["radius"]).mean())
    r = Renderer(sc, tex, sky, W, H, depth=1)
    r.look(**cam)
    r.render(readback=False)
    points = r.gbuffer(api.GB_POINT)["point"].reshape(N, 3)
    rec = r.read_rays()
    camera = api.make_rays(rec[:, 0:3], rec[:, 4:7])
    r.w.set_async(1)
    perm = np.random.default_rng(1).permutation(N)
    d_hits = torch.empty(N * 32, dtype=torch.uint8, device="cuda")
    d_within = torch.empty(N, dtype=torch.uint8, device="cuda")
    d_d, d_id = torch.empty(8 * N, dtype=torch.float32, device="cuda"), torch.empty(8 * N, dtype=torch.int32, device="cuda")
    if a.cap_sweep:
        for cap in (0, 8, 27, 64, 125, 216, 512, 1000, 4096, 1 << 30):
            os.environ["CLWRAP_NEAR_BOX_CELLS"] = str(cap)
            for reach in REACHES:
                d_probes = device(api.make_probes(points, reach * rbar))
                torch.cuda.synchronize()
                row(name, f"cap {cap:>10} reach {reach} r: nearest", repeats(r, lambda: r.w.probe_device(d_probes.data_ptr(), N, FLAGS, hits_ptr=d_hits.data_ptr()), api.TIMING_NEAR))
                row(name, f"cap {cap:>10} reach {reach} r: K = 8", repeats(r, lambda: r.w.near_surfaces_device(d_probes.data_ptr(), N, FLAGS, 8, d_d.data_ptr(), d_id.data_ptr()), api.TIMING_NEAR))
        os.environ.pop("CLWRAP_NEAR_BOX_CELLS")
        r.release()
        continue
    d_rays = device(camera)
    torch.cuda.synchronize()
    cast = row(name, "wt_cast nearest, the camera's rays, pixel order", repeats(r, lambda: r.w.cast_rays_device(d_rays.data_ptr(), N, FLAGS, hits_ptr=d_hits.data_ptr()), api.TIMING_CAST))
    near = {}
    for order, idx in (("pixel order", None), ("permuted", perm)):
        for reach in REACHES:
            probes = api.make_probes(points if idx is None else points[idx], reach * rbar)
            d_probes = device(probes)
            torch.cuda.synchronize()
            what = f"{order}, reach {reach} r"
            near[(order, reach)] = row(name, f"nearest, {what}", repeats(r, lambda: r.w.probe_device(d_probes.data_ptr(), N, FLAGS, hits_ptr=d_hits.data_ptr()), api.TIMING_NEAR))
            row(name, f"within,  {what}", repeats(r, lambda: r.w.probe_device(d_probes.data_ptr(), N, FLAGS, within_ptr=d_within.data_ptr()), api.TIMING_NEAR))
            for K in (1, 4, 8):
                row(name, f"K = {K},   {what}", repeats(r, lambda: r.w.near_surfaces_device(d_probes.data_ptr(), N, FLAGS, K, d_d.data_ptr(), d_id.data_ptr()), api.TIMING_NEAR))
            if idx is None and reach == 1.0:
                say(f"{name:<4} | {what}: within {float(d_within.cpu().numpy().mean()):.4f} of the probes")
    r.w.sync()
    t_points = torch.from_numpy(points.copy()).cuda()
    t_centres = torch.from_numpy(sc.spheres["origin"].astype(np.float32)).cuda()
    t_radii = torch.from_numpy(np.abs(sc.spheres["radius"].astype(np.float32))).cuda()
    t_min = row(name, "torch: cdist - r, min  (spheres only, unlimited reach, pixel order)", torch_repeats(lambda: torch_route(t_points, t_centres, t_radii, 0)))
    k8 = min(8, len(sc.spheres))
    t_top = row(name, f"torch: cdist - r, topk {k8} (spheres only, unlimited reach, pixel order)", torch_repeats(lambda: torch_route(t_points, t_centres, t_radii, k8)))
    ref = near[("pixel order", 1.0)]
    say(f"{name:<4} | nearest, pixel order, reach 1 r = {ref / cast:.2f} x wt_cast's nearest query; the torch min = {t_min / ref:.1f} x it, the torch topk = {t_top / ref:.1f} x it")
    r.release()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
