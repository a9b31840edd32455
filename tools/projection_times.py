"""Kernel times of the camera models beside the pinhole (clw_ext_set_projection) next to the pinhole's own launches of the same frame
(clw_ext_timing_*; one process, launches back to back).
   python tools/projection_times.py [--frames N] [--repeats R] [--out FILE]
   The demo scene and sphere_grid_scene() (10 000 spheres, the uniform grid) at 1920x1080 and 800x600, depth 1 and 4.  Per frame and model:
     wt_raygen_proj         ms per launch; the camera origin moves a little every frame, so every frame generates its records (a still view would
                            generate them once) -- the origin is not part of a panorama's tables, so no table is rebuilt
     trace from the buffer  ms per launch of the ray-buffer trace behind it
     their sum              against the fused pinhole launch of the same frame and depth
     pass                   the primary-hit pass (all channels / depth + id) under the model, against the pinhole's
   and once per frame size: wt_raygen_proj against the plain wt_raygen (CLWRAP_FUSE=0) of the same size in the same run, both as a store rate
   (64 bytes per ray).  Every figure is the median (min .. max) of R repeats of N launches after two warm-up launches.
   With --pinhole-only, and with CLWRAP_LIB=<a library built from the parent commit>, only the pinhole rows are printed: the same frames on that commit's kernels, for
   the A/B of the unchanged launches (this build's median should lie inside the other build's min .. max)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import api, scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pinhole-only", action="store_true", help="the pinhole's rows only: the short run of an A/B against another build")
ap.add_argument("--out", default=None)
a = ap.parse_args()
tex, sky = textures.texture_layers(), textures.skybox_cross(4096)
HAVE = hasattr(api.load_library(), "clw_ext_set_projection")
CAM_DEMO = dict(origin=pkg.CAMERA_RAYPNG["origin"], look=pkg.CAMERA_RAYPNG["look"])
CAM_GRID = dict(origin=(0.0, 6.0, -2.0), look=(0.1, -0.3, 1.0))      # over the field of spheres
lines = []


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def point(cam, model, r, k=0):
    """the view of frame k through `model` (None = the pinhole): the origin moves by 1e-3 per frame"""
    origin = (cam["origin"][0] + 1e-3 * k, cam["origin"][1], cam["origin"][2])
    if model == "ortho":
        r.look_ortho(origin, cam["look"], 12.0 if cam is CAM_DEMO else 40.0)
    elif model == "equirect":
        r.look_panorama(origin, cam["look"])
    else:
        r.look(origin, cam["look"])


def timed_frames(sc, cam, W, H, depth, model, fuse=True):
    """-> (raygen kernel ms, trace kernel ms) per launch; a raygen figure of None = no raygen kernel ran (the fused pinhole launch)"""
    r = Renderer(sc, tex, sky, W, H, depth=depth, fuse=fuse)
    for k in (0, 1):
        point(cam, model, r, k)
        r.render(readback=False)
    r.w.set_async(1)
    gen, trace = [], []
    for _ in range(a.repeats):
        r.w.timing_reset()
        for k in range(a.frames):
            point(cam, model, r, 2 + k)
            r.render(readback=False)
        r.w.sync()
        n0, ms0 = r.w.timing_get(0)
        n1, ms1 = r.w.timing_get(1)
        assert n1 == a.frames and n0 in (0, a.frames), (n0, n1)
        gen.append(ms0 / n0 if n0 else None)
        trace.append(ms1 / n1)
    flags = r.w.last_trace_flags()
    r.release()
    return (stats(gen) if gen[0] is not None else None), stats(trace), flags


def timed_pass(sc, cam, W, H, channels, model):
    r = Renderer(sc, tex, sky, W, H, depth=4)
    point(cam, model, r)
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


def row(where, what, v, note=""):
    lines.append(f"{where} | {what:<44} | {v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f}){note}")
    print(lines[-1], flush=True)


lines.append(f"# tools/projection_times.py: kernel ms, median (min .. max) of {a.repeats} x {a.frames} launches; kernels {api.kernel_source_hash()}"
             + ("" if HAVE else " (a build without the camera models: the pinhole's launches only)"))
print(lines[-1], flush=True)
HAVE = HAVE and not a.pinhole_only
models = (None, "ortho", "equirect") if HAVE else (None,)
for name, sc, cam in (("demo", scene.render_map_scene(), CAM_DEMO), ("grid10000", scene.sphere_grid_scene(), CAM_GRID)):
    for W, H in ((1920, 1080), (800, 600)):
        where = f"{name} {W}x{H}"
        for depth in (1, 4):
            fused = None
            for model in models:
                gen, trace, flags = timed_frames(sc, cam, W, H, depth, model)
                if model is None:
                    fused = trace
                    row(where, f"depth {depth} pinhole, fused launch", trace, f"  flags {flags}")
                    continue
                row(where, f"depth {depth} {model}: wt_raygen_proj", gen, f"  = {64e-6 * W * H / gen[0]:.0f} GB/s of stores")
                row(where, f"depth {depth} {model}: trace from the buffer", trace, f"  flags {flags}")
                total = gen[0] + trace[0]
                lines.append(f"{where} | depth {depth} {model}: raygen + trace = {total:.4f} ms = {total / fused[0]:.2f} x the fused pinhole launch "
                             f"({total - fused[0]:+.4f} ms)")
                print(lines[-1], flush=True)
        for model in models:
            tag = model or "pinhole"
            row(where, f"pass, all channels (52 B/px), {tag}", timed_pass(sc, cam, W, H, api.GB_ALL, model))
            row(where, f"pass, depth + id (8 B/px), {tag}", timed_pass(sc, cam, W, H, api.GB_DEPTH | api.GB_ID, model))
    if name == "demo" and HAVE:      # the raygen kernels alone: the scene does not matter to them
        for W, H in ((1920, 1080), (800, 600), (4096, 4096)):
            plain, _, _ = timed_frames(sc, cam, W, H, 1, None, fuse=False)
            row(f"raygen {W}x{H}", "wt_raygen (pinhole, CLWRAP_FUSE=0)", plain, f"  = {64e-6 * W * H / plain[0]:.0f} GB/s of stores")
            for model in ("ortho", "equirect"):
                gen, _, _ = timed_frames(sc, cam, W, H, 1, model)
                row(f"raygen {W}x{H}", f"wt_raygen_proj, {model}", gen, f"  = {64e-6 * W * H / gen[0]:.0f} GB/s of stores; {gen[0] / plain[0]:.2f} x wt_raygen")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
