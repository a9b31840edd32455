"""Kernel time of the ambient occlusion pass (clw_ext_render_ao): its primary-hit pass, wt_ao_trace and wt_ao_resolve each on their own, with
the trace launches of the same frame beside them (clw_ext_timing_*; one process, launches back to back).
   python tools/ao_times.py [--frames N] [--repeats R] [--baseline] [--out FILE]
   The demo scene and the 10 000-sphere scene at 1920x1080: ms per launch of the point + normal + id primary-hit pass the AO pass runs (logged
   under TIMING_GBUFFER), of wt_ao_trace (TIMING_AO) at K = 4, 8, 16 with radius 1 and +inf, of wt_ao_resolve (TIMING_AO_RESOLVE) with and
   without FILTER; then the depth-1 and depth-4 trace launches, and the depth-1 trace launch with an AO call (K = 8, radius 1) between frames.
   Every figure is the median (min .. max) of R repeats of N launches after two warm-up launches.
   --baseline: the trace launches alone -- nothing of the AO pass is called, so the run also works against a library built from the parent
   commit (CLWRAP_LIB=<its .so>): the feature unused must cost what the parent costs, inside the spread printed here.
   Read off: wt_ao_trace against the depth-1 trace launch (K any-hit rays against one Whitted bounce); radius 1 against +inf (the reach check
   and the clipped grid walk); the resolve with FILTER against without (the 35 x 11 staged halo)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import api, scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--baseline", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
W, H = 1920, 1080
SCENES = (("demo", scene.render_map_scene, pkg.CAMERA_RAYPNG),
          ("10k", lambda: scene.sphere_grid_scene(100, 100), dict(origin=(0.0, 12.0, -10.0), look=(0.0, -0.45, 1.0), fov=90.0, focal=1.0)))


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def repeats(r, launch, ids, per_launch=1):
    """R repeats of N launches -> {timing id: (median, min, max) ms per logged launch}"""
    launch(); launch()
    ms = {k: [] for k in ids}
    for _ in range(a.repeats):
        r.w.timing_reset()
        for _ in range(a.frames):
            launch()
        r.w.sync()
        for k in ids:
            n, total = r.w.timing_get(k)
            assert n == a.frames * per_launch, (k, n)
            ms[k].append(total / n)
    return {k: stats(v) for k, v in ms.items()}


lines = [f"# tools/ao_times.py{' --baseline' if a.baseline else ''}: median (min .. max) of {a.repeats} x {a.frames} launches at {W}x{H}; "
         f"kernels {api.kernel_source_hash()}", "# scene | launch | ms"]
for name, make, cam in SCENES:
    sc = make()

    def row(what, v):
        lines.append(f"{name:<4} | {what:<52} | {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})")
        print(lines[-1], flush=True)

    if not a.baseline:
        r = Renderer(sc, tex, sky, W, H, depth=1)
        r.look(**cam)
        r.render(readback=False)                     # the frame COMPOSE would read; latches the camera, prepares the scene
        r.w.set_async(1)
        for radius in (1.0, float("inf")):
            for K in (4, 8, 16):
                ao = api.ao_params(K, radius, 256, True, False)

                def launch():
                    assert r.w.render_ao(ao) == W * H
                t = repeats(r, launch, (api.TIMING_GBUFFER, api.TIMING_AO, api.TIMING_AO_RESOLVE))
                if K == 4 and radius == 1.0:
                    row("AO: primary-hit pass, point + normal + id (28 B/px)", t[api.TIMING_GBUFFER])
                    row("AO: wt_ao_resolve, FILTER", t[api.TIMING_AO_RESOLVE])
                row(f"AO: wt_ao_trace, K = {K:>2}, radius {radius:g}", t[api.TIMING_AO])
        for flags, what in ((0, "no flag"), (api.AO_COMPOSE, "COMPOSE"), (api.AO_FILTER | api.AO_COMPOSE, "FILTER | COMPOSE")):
            ao = api.clw_ao(flags, 8, 1.0, 256)

            def launch():
                assert r.w.render_ao(ao) == W * H
            row(f"AO: wt_ao_resolve, {what}", repeats(r, launch, (api.TIMING_AO_RESOLVE,))[api.TIMING_AO_RESOLVE])
        counts = r.w.read_ao(api.AO_COUNTS)
        lines.append(f"{name:<4} | mean open fraction at K = 8, radius 1: {counts.mean() / 8:.4f}")
        print(lines[-1], flush=True)
        r.release()
    for depth in (1, 4):
        r = Renderer(sc, tex, sky, W, H, depth=depth)
        r.look(**cam)
        r.w.set_async(1)
        row(f"trace, depth {depth}", repeats(r, lambda: r.render(readback=False), (1,))[1])
        if depth == 1 and not a.baseline:
            ao = api.ao_params(8, 1.0)

            def launch():
                r.render(readback=False)
                assert r.w.render_ao(ao) == W * H
            row("trace, depth 1, an AO call between frames", repeats(r, launch, (1,))[1])
        r.release()
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
