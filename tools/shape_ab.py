"""A/B of the shaped trace kernel (the scene's counts compiled in, wt_shape) against the generic one (variant 8192): kernel ms of
small-scene shallow launches -- render.map at several frame sizes and depths -- each side in a fresh process, the two sides
alternated `rounds` times, and whether the frames are identical.  Prints one JSON line per (frame, depth).
   python tools/shape_ab.py [rounds]"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = r'''
import sys, json, zlib
sys.path.insert(0, %r)
import torch
import example_gui_opencl_raytracer_amd as pkg
from example_gui_opencl_raytracer_amd import scene, textures
from example_gui_opencl_raytracer_amd.renderer import Renderer
W, H, depth, variant = map(int, sys.argv[1:5])
r = Renderer(scene.render_map_scene(), textures.texture_layers(), textures.skybox_cross(4096), W, H, depth=depth)
r.w.set_variant(variant); r.look(**pkg.CAMERA_RAYPNG)
crc = zlib.crc32(r.render().tobytes())
for _ in range(5): r.render(readback=False)
r.w.timing_reset(); r.w.set_async(1)
for _ in range(200): r.render(readback=False)
r.w.sync(); n, ms = r.w.timing_get(1)
print(json.dumps(dict(flags=r.w.last_trace_flags(), kernel_ms=ms / n, crc=crc)))
''' % ROOT
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
for (W, H, depth) in ((1920, 1080, 4), (1920, 1080, 1), (1280, 720, 4), (2560, 1440, 4), (3840, 2160, 4)):
    res = {0: [], 8192: []}
    crcs, flags = set(), {}
    for _ in range(rounds):
        for variant in (8192, 0):
            out = subprocess.run([sys.executable, "-c", code, str(W), str(H), str(depth), str(variant)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(out.stdout[-500:], out.stderr[-1500:], flush=True)
                raise SystemExit(f"run failed: {W}x{H} depth {depth} variant {variant} rc {out.returncode}")
            d = json.loads(out.stdout.strip().splitlines()[-1])
            res[variant].append(d["kernel_ms"]); crcs.add(d["crc"]); flags[variant] = d["flags"]
    g, s = min(res[8192]), min(res[0])
    print(json.dumps(dict(frame=f"{W}x{H}", depth=depth, generic_ms=[round(x, 4) for x in res[8192]], shaped_ms=[round(x, 4) for x in res[0]],
                          shaped_flags=flags[0], generic_flags=flags[8192], best_gain_pct=round(100 * (1 - s / g), 1), identical=len(crcs) == 1)), flush=True)
