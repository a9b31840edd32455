"""A/B of the trimmed trace loop (no bounce block on a path's last level, tile cost reduced by DPP; csrc/whitted_bounce.inc, wt_wave_reduce)
against the untrimmed one (variant 16384, same kernel): kernel ms of render.map at several frame sizes and depths -- each side in a
fresh process, the two sides alternated `rounds` times, and whether the frames are identical.  Prints one JSON line per (frame, depth).
   python tools/trim_ab.py [rounds] [base variant, e.g. 8192 for the generic kernel]"""
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
base = int(sys.argv[2]) if len(sys.argv) > 2 else 0
OLD, NEW = base | 16384, base
for (W, H, depth) in ((1920, 1080, 4), (1920, 1080, 1), (1280, 720, 4), (3840, 2160, 4)):
    res = {NEW: [], OLD: []}
    crcs, flags = set(), {}
    for _ in range(rounds):
        for variant in (OLD, NEW):
            out = subprocess.run([sys.executable, "-c", code, str(W), str(H), str(depth), str(variant)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(out.stdout[-500:], out.stderr[-1500:], flush=True)
                raise SystemExit(f"run failed: {W}x{H} depth {depth} variant {variant} rc {out.returncode}")
            d = json.loads(out.stdout.strip().splitlines()[-1])
            res[variant].append(d["kernel_ms"]); crcs.add(d["crc"]); flags[variant] = d["flags"]
    g, s = min(res[OLD]), min(res[NEW])
    print(json.dumps(dict(frame=f"{W}x{H}", depth=depth, untrimmed_ms=[round(x, 4) for x in res[OLD]], trimmed_ms=[round(x, 4) for x in res[NEW]],
                          flags=flags[NEW], same_kernel=flags[NEW] == flags[OLD], best_gain_pct=round(100 * (1 - s / g), 1), identical=len(crcs) == 1)), flush=True)
