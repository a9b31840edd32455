"""Kernel time of the selection overlay (clw_ext_render_overlay): its id pass and wt_overlay each on their own, with the depth + id G-buffer pass
and the depth-1 trace launch of the same frame beside them (clw_ext_timing_*; one process, launches back to back).
   python tools/overlay_times.py [--frames N] [--repeats R] [--out FILE]
   The demo scene at 1920x1080 and 800x600, the sphere under the middle of the frame's sphere pixels selected: ms per launch of the id-only
   primary-hit pass the overlay runs (logged under TIMING_GBUFFER) and of wt_overlay (TIMING_OVERLAY), for radius 1 and 4, with all three flags
   and with OUTLINE alone; then the depth + id pass of clw_ext_render_gbuffer and the depth-1 trace launch.  Every figure is the median
   (min .. max) of R repeats of N launches after two warm-up launches.
   Read off: wt_overlay against the id pass (the issue's expectation: a fraction of it); radius 4 against radius 1 (the halo: 40 x 16 staged
   words per 32 x 8 tile against 34 x 10); OUTLINE alone against all flags."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import api, scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def repeats(r, launch, ids):
    """R repeats of N launches -> {timing id: (median, min, max) ms per launch}"""
    launch(); launch()
    ms = {k: [] for k in ids}
    for _ in range(a.repeats):
        r.w.timing_reset()
        for _ in range(a.frames):
            launch()
        r.w.sync()
        for k in ids:
            n, total = r.w.timing_get(k)
            assert n == a.frames, (k, n)
            ms[k].append(total / n)
    return {k: stats(v) for k, v in ms.items()}


lines = [f"# tools/overlay_times.py: median (min .. max) of {a.repeats} x {a.frames} launches; kernels {api.kernel_source_hash()}",
         "# scene frame | launch | ms"]
sc = scene.render_map_scene()
for W, H in ((1920, 1080), (800, 600)):
    def row(what, v):
        lines.append(f"demo {W}x{H} | {what:<44} | {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})")
        print(lines[-1], flush=True)
    r = Renderer(sc, tex, sky, W, H, depth=4)
    r.look(**pkg.CAMERA_RAYPNG)
    r.render(readback=False)                     # the frame the overlay reads; latches the camera, prepares the scene
    ids = r.gbuffer(api.GB_ID)["id"]
    on = np.flatnonzero(api.id_kind(ids) == api.ID_SPHERE)
    sel = [int(ids[on[on.size // 2]])]
    r.w.set_async(1)
    for flags, name in ((api.OV_ALL, "all flags"), (api.OV_OUTLINE, "OUTLINE alone")):
        for radius in (1, 4):
            style = api.overlay_style(flags, radius, 0xFFFF00, 0x2060E0, 96, 0x00FF40)
            def launch():
                assert r.w.render_overlay(style, sel) == W * H
            t = repeats(r, launch, (api.TIMING_GBUFFER, api.TIMING_OVERLAY))
            row(f"overlay {name}, radius {radius}: id pass", t[api.TIMING_GBUFFER])
            row(f"overlay {name}, radius {radius}: wt_overlay", t[api.TIMING_OVERLAY])
    selected = int((ids == sel[0]).sum())
    row("G-buffer pass, depth + id (8 B/px)", repeats(r, lambda: r.w.render_gbuffer(api.GB_DEPTH | api.GB_ID), (api.TIMING_GBUFFER,))[api.TIMING_GBUFFER])
    r.release()
    r = Renderer(sc, tex, sky, W, H, depth=1)
    r.look(**pkg.CAMERA_RAYPNG)
    r.w.set_async(1)
    row("trace, depth 1", repeats(r, lambda: r.render(readback=False), (1,))[1])
    r.release()
    lines.append(f"demo {W}x{H} | selected: sphere id {sel[0]}, {selected} of {W * H} pixels")
    print(lines[-1], flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
