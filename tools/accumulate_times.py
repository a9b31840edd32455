"""Kernel time of progressive frame accumulation, and of the plain launch beside it (clw_ext_timing_*; one process, frames back to back).
   python tools/accumulate_times.py [--frames N] [--repeats R] [--out FILE]
   The demo scene at 1920x1080 depth 4 (C2), at 800x600 depth 15 and at 1920x1080 depth 4 with 2 x 2 samples: ms per frame with the mode off,
   and with it on, jitter on and off.  Every figure is the median (min .. max) of R repeats of N frames after two warm-up frames.
   Read off: on - off = the cost of the 12-byte read-modify-write per output pixel; jitter on - jitter off = what a sub-pixel offset per frame
   costs the cost-sorted dispatch (the order is the still view's).
   With CLWRAP_LIB=<a library built from an earlier commit> only the mode-off rows are printed: the same frames on that commit's kernels, for
   the A/B of the plain launch (its median should lie inside the other build's min .. max)."""
import argparse, os, statistics, sys
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
sc = scene.render_map_scene()
HAVE_MODE = hasattr(api.load_library(), "clw_ext_set_accumulate")


def timed(W, H, depth, n, mode):
    """mode: None = off, True / False = on with / without jitter -> (median kernel ms per frame, min, max)"""
    kw = {} if mode is None else dict(accumulate=65536, jitter=mode)
    r = Renderer(sc, tex, sky, W, H, depth=depth, supersample=n, **kw)
    r.look(**pkg.CAMERA_RAYPNG)
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
    if mode is not None:
        assert r.accumulated == 2 + a.repeats * a.frames
    r.release()
    return statistics.median(ms), min(ms), max(ms)


lines = [f"# tools/accumulate_times.py: kernel ms per frame, median (min .. max) of {a.repeats} x {a.frames} frames; kernels {api.kernel_source_hash()}"
         + ("" if HAVE_MODE else " (a build without the mode: plain launches only)"),
         "# frame depth n | launch | ms"]
for (W, H, depth, n) in ((1920, 1080, 4, 1), (800, 600, 15, 1), (1920, 1080, 4, 2)):
    off = timed(W, H, depth, n, None)
    lines.append(f"{W}x{H} d{depth} n={n} | mode off            | {off[0]:.4f} ({off[1]:.4f} .. {off[2]:.4f})")
    print(lines[-1], flush=True)
    if not HAVE_MODE:
        continue
    res = {}
    for jitter in (True, False):
        res[jitter] = timed(W, H, depth, n, jitter)
        lines.append(f"{W}x{H} d{depth} n={n} | accumulate jitter={int(jitter)} | {res[jitter][0]:.4f} ({res[jitter][1]:.4f} .. {res[jitter][2]:.4f})")
        print(lines[-1], flush=True)
    lines.append(f"{W}x{H} d{depth} n={n} | cost of the mode (jitter off - off) {res[False][0] - off[0]:+.4f} ms = {24e-6 * (W * H) / max(res[False][0] - off[0], 1e-9):.0f} GB/s for its "
                 f"24 bytes per pixel | jitter on - jitter off {res[True][0] - res[False][0]:+.4f} ms")
    print(lines[-1], flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
