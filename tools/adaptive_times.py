"""Kernel time of adaptive supersampling against the 1-sample and the plain n x n launch (clw_ext_timing_*; one process, frames back to back).
   python tools/adaptive_times.py [--frames N] [--repeats R] [--out FILE]
   The demo scene at 1920x1080 depth 4 and at 800x600 depth 15, n in {2, 4}: ms per frame of the 1-sample launch, the plain n x n launch and
   the adaptive launch (base pass + classifier + refine pass, timed as one) at T in {0, 16, 64, 256}, with the share of blocks refined.
   Read off: adaptive(256) - 1-sample = the fixed cost of the classifier and an empty refine launch; adaptive(0) - plain = the worst case;
   adaptive(16) against plain = the gain.  Every figure is the median of R repeats of N frames after two warm-up frames."""
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


def timed(W, H, depth, n, T):
    """-> (median kernel ms per frame, min, max, share of blocks refined or None)"""
    r = Renderer(sc, tex, sky, W, H, depth=depth, supersample=n, adaptive=T)
    r.look(**pkg.CAMERA_RAYPNG)
    r.render(readback=False); r.render(readback=False)
    share = None
    if T is not None:
        m = r.w.read_refine_mask()
        share = float(m.mean())
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
    return statistics.median(ms), min(ms), max(ms), share


lines = [f"# tools/adaptive_times.py: kernel ms per frame, median (min .. max) of {a.repeats} x {a.frames} frames; kernels {api.kernel_source_hash()}",
         "# frame depth n | launch | ms | blocks refined"]
for (W, H, depth) in ((1920, 1080, 4), (800, 600, 15)):
    one = timed(W, H, depth, 1, None)
    lines.append(f"{W}x{H} d{depth} n=1 | 1-sample       | {one[0]:.4f} ({one[1]:.4f} .. {one[2]:.4f}) |")
    print(lines[-1], flush=True)
    for n in (2, 4):
        res = {None: timed(W, H, depth, n, None)}
        lines.append(f"{W}x{H} d{depth} n={n} | plain {n}x{n}      | {res[None][0]:.4f} ({res[None][1]:.4f} .. {res[None][2]:.4f}) | 100.0 %")
        print(lines[-1], flush=True)
        for T in (0, 16, 64, 256):
            res[T] = timed(W, H, depth, n, T)
            lines.append(f"{W}x{H} d{depth} n={n} | adaptive T={T:<3d} | {res[T][0]:.4f} ({res[T][1]:.4f} .. {res[T][2]:.4f}) | {res[T][3] * 100:5.1f} %")
            print(lines[-1], flush=True)
        lines.append(f"{W}x{H} d{depth} n={n} | fixed overhead (T=256 - 1-sample) {res[256][0] - one[0]:+.4f} ms | worst case (T=0 - plain) {res[0][0] - res[None][0]:+.4f} ms | "
                     f"T=16 / plain {res[16][0] / res[None][0]:.3f} | T=64 / plain {res[64][0] / res[None][0]:.3f}")
        print(lines[-1], flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
