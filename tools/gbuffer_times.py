"""Kernel time of the primary-hit pass (clw_ext_render_gbuffer), the wall time of a pick, and the 1-sample trace launches of the same frame beside
them (clw_ext_timing_*; one process, launches back to back).
   python tools/gbuffer_times.py [--frames N] [--repeats R] [--out FILE]
   The demo scene at 1920x1080 and 800x600 and sphere_grid_scene() (10 000 spheres, the uniform grid) at 1920x1080: ms per launch of the pass with
   all five channels (52 bytes stored per pixel) and with depth + id only (8 bytes), microseconds per pick (the whole call: one launch, a 44-byte
   read-back, the wait), and ms per depth-1 and depth-4 trace launch.  Every figure is the median (min .. max) of R repeats of N launches after two
   warm-up launches.
   Read off: the depth + id pass against the depth-1 trace launch (it does a subset of that launch's work); all channels - depth + id = what the
   other 44 bytes per pixel cost, printed as a store rate.
   With CLWRAP_LIB=<a library built from an earlier commit> only the trace rows are printed: the same frames on that commit's kernels, for the A/B
   of the unchanged trace launches (this build's median should lie inside the other build's min .. max)."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import api, scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
HAVE_PASS = hasattr(api.load_library(), "clw_ext_render_gbuffer")
CAM_GRID = dict(origin=(0.0, 6.0, -2.0), look=(0.1, -0.3, 1.0), fov=90.0, focal=1.0)      # over the field of spheres


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def timed_trace(sc, cam, W, H, depth):
    r = Renderer(sc, tex, sky, W, H, depth=depth)
    r.look(**cam)
    r.render(readback=False); r.render(readback=False)
    r.w.set_async(1)
    ms = []
    for _ in range(a.repeats):
        r.w.timing_reset()
        for _ in range(a.frames):
            r.render(readback=False)
        r.w.sync()
        k, total = r.w.timing_get(1)
        assert k == a.frames
        ms.append(total / k)
    r.release()
    return stats(ms)


def timed_pass(sc, cam, W, H, channels):
    r = Renderer(sc, tex, sky, W, H, depth=4)
    r.look(**cam)
    r.render(readback=False)                     # latches the camera, prepares the scene
    assert r.w.render_gbuffer(channels) == W * H and r.w.render_gbuffer(channels) == W * H
    ms = []
    for _ in range(a.repeats):
        r.w.timing_reset()
        for _ in range(a.frames):
            r.w.render_gbuffer(channels)
        r.w.sync()
        k, total = r.w.timing_get(api.TIMING_GBUFFER)
        assert k == a.frames
        ms.append(total / k)
    r.release()
    return stats(ms)


def timed_pick(sc, cam, W, H):
    r = Renderer(sc, tex, sky, W, H, depth=4)
    r.look(**cam)
    r.render(readback=False)
    assert r.w.pick(W // 2, H // 2) is not None and r.w.pick(1, 1) is not None
    us = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for k in range(a.frames):
            r.w.pick((W // 2 + 37 * k) % W, (H // 2 + 11 * k) % H)
        us.append((time.perf_counter() - t0) * 1e6 / a.frames)
    r.release()
    return stats(us)


lines = [f"# tools/gbuffer_times.py: median (min .. max) of {a.repeats} x {a.frames} launches; kernels {api.kernel_source_hash()}"
         + ("" if HAVE_PASS else " (a build without the pass: trace launches only)"),
         "# scene frame | launch | ms (pick: us of wall time per call)"]
for name, sc, cam, W, H in (("demo", scene.render_map_scene(), pkg.CAMERA_RAYPNG, 1920, 1080), ("demo", None, pkg.CAMERA_RAYPNG, 800, 600),
                            ("grid10000", scene.sphere_grid_scene(), CAM_GRID, 1920, 1080)):
    sc = sc if sc is not None else scene.render_map_scene()
    def row(what, v, unit="ms"):
        lines.append(f"{name} {W}x{H} | {what:<28} | {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f}){'' if unit == 'ms' else ' ' + unit}")
        print(lines[-1], flush=True)
    if HAVE_PASS:
        full = timed_pass(sc, cam, W, H, api.GB_ALL)
        row("pass, all channels (52 B/px)", full)
        thin = timed_pass(sc, cam, W, H, api.GB_DEPTH | api.GB_ID)
        row("pass, depth + id (8 B/px)", thin)
        row("pick, wall time of the call", timed_pick(sc, cam, W, H), "us")
    d1 = timed_trace(sc, cam, W, H, 1)
    row("trace, depth 1", d1)
    row("trace, depth 4", timed_trace(sc, cam, W, H, 4))
    if HAVE_PASS:
        extra = full[0] - thin[0]
        lines.append(f"{name} {W}x{H} | depth + id pass / depth-1 trace = {thin[0] / d1[0]:.2f}; all channels - depth + id = {extra:+.4f} ms = "
                     f"{44e-6 * W * H / max(extra, 1e-9):.0f} GB/s for its 44 more bytes per pixel; all channels alone = {52e-6 * W * H / full[0]:.0f} GB/s of stores")
        print(lines[-1], flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
