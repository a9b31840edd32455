/*
 * hip_wrap_ext.h -- entry points the reference API has no slot for.
 *
 * The reference bakes these into compile-time macros or has no notion of them:
 *   depth           #define MAX_DEPTH 15            (reference raytracing.cl:9)
 *   frame size      #define WIDTH/HEIGHT 800/600    (raypng.c:8-9, rayinteractive.c:13-14)
 *   counts          one byte each                   (raytracing.cl:17, cpu_obj.c:62-68)
 *   device / queue  platform 0, device 0, one queue (opencl_wrap.c:26-34, 118-119)
 * They are needed by the bench driver, the row-strip multi-GPU mode and the parity
 * tests.  Everything here is optional: a caller that only uses opencl_wrap.h gets the
 * reference's behaviour.  Plain C ABI: pointers and sizes only.
 *
 * Environment variables read once by cl_wrap_init (same meaning as the setters):
 *   CLWRAP_DEPTH=<1..32>   CLWRAP_STRICT=<0|1>   CLWRAP_FUSE=<0|1>   CLWRAP_DEVICE=<ordinal>   CLWRAP_PIPELINE=<0|1>   CLWRAP_THROUGH=<float>
 *   CLWRAP_SUPERSAMPLE=<1|2|4|8>   CLWRAP_APERTURE=<float >= 0>   CLWRAP_FOCUS=<float > 0>   (thin lens: clw_ext_set_lens)
 *   CLWRAP_ADAPTIVE=<0..256>   CLWRAP_SEED_OFFSET=<uint32>   CLWRAP_ACCUMULATE=<0..65536>   CLWRAP_ACC_JITTER=<0|1>   (clw_ext_set_accumulate)
 *   CLWRAP_PROJECTION=<ortho|equirect>   CLWRAP_ORTHO_WIDTH=<float >= 0>   CLWRAP_PANO_SPAN=<h>,<v>   (camera model: clw_ext_set_projection)
 * Tuning / experiment knobs (defaults are the measured optima): CLWRAP_GRID_MIN, CLWRAP_GRID_DENSITY (uniform grid),
 *   CLWRAP_OCC_TILES_PER_DEPTH (deep launches of >= this x depth tiles take the high-occupancy kernel flavour),
 *   CLWRAP_TIMING_EVERY, CLWRAP_VARIANT (bit mask of clw_ext_set_variant).
 */
#ifndef HIP_WRAP_EXT_H
#define HIP_WRAP_EXT_H
#include "opencl_wrap.h"
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLW_MAX_DEPTH 32

/* Trace depth (reference MAX_DEPTH).  Default 15.  Errors (print + exit(1)) outside [1, 32]. */
void clw_ext_set_depth(cl_wrap* wrap, int depth);
int  clw_ext_get_depth(const cl_wrap* wrap);

/* Arithmetic mode of the trace kernel: 0 = fast (FMA contraction, native rcp/rsq/sqrt --
 * the envelope an OpenCL device build of the reference is allowed), 1 = strict (no
 * contraction, IEEE divide/sqrt: tracks the un-contracted oracle). Default 0. */
void clw_ext_set_strict(cl_wrap* wrap, int strict);

/* 1 (default): a "raygen" launch latches its eight by-value arguments and the trace
 * kernel synthesises primary rays in registers; the 64 B/pixel ray buffer is only
 * materialised if somebody reads it back.  0: run the two kernels as the reference does. */
void clw_ext_set_fuse(cl_wrap* wrap, int fuse);

/* Row strips / sub-ranges: work-item i of the next launches has global id first_id + i
 * (used for id %% width, id / width and the RNG seed; reference raygen.cl:13-14,
 * raytracing.cl:33).  Buffers are indexed by i.  Default 0. */
void clw_ext_set_id_offset(cl_wrap* wrap, uint64_t first_id);

/* Interleaved row bands (balanced multi-GPU sharding): with stride S > 1 the next launches own
 * every S-th 8-row band of the frame, starting at band `phase`: local row y is global row
 * ((y / 8) * S + phase) * 8 + y % 8.  Needs height % (8 * S) == 0 and id offset 0.
 * stride 1 (default) = one contiguous range. */
void clw_ext_set_row_bands(cl_wrap* wrap, uint32_t stride, uint32_t phase);

/* 1: cl_wrap_output returns without waiting for the kernel (no host read-back may be
 * requested in that mode); clw_ext_sync waits.  Default 0 = the reference's behaviour. */
void clw_ext_set_async(cl_wrap* wrap, int async);
void clw_ext_sync(cl_wrap* wrap);

/* Launch on a caller-owned hipStream_t (e.g. torch's current stream) instead of the
 * wrapper's own stream.  NULL restores the wrapper's stream. */
void clw_ext_set_stream(cl_wrap* wrap, void* hip_stream);

/* Per-kernel device timing from hipEvents recorded around every launch on the launch
 * stream, from the first clw_ext_timing_reset on (a wrapper nobody asks for timings records no events).
 * reset clears the log; get waits for the logged launches and returns how many
 * there were and their summed duration in milliseconds. */
void clw_ext_timing_reset(cl_wrap* wrap);
void clw_ext_timing_get(cl_wrap* wrap, cl_uint kernel_id, uint32_t* launches, double* total_ms);
/* Pipelined read-back (default on; env CLWRAP_PIPELINE=0): a blocking cl_wrap_output that renders a frame of >= 16 MB
 * at depth <= 4 and reads that same framebuffer back is executed as four strips, strip c being copied to the host while
 * strip c+1 renders (3840x2160: 940 -> 1 340 frames/s).  Same pixels, same semantics -- the call returns with the whole
 * frame in host memory.  Smaller frames and deep launches keep the single launch + single copy (measured: no gain / a
 * loss there). */
void clw_ext_set_pipeline(cl_wrap* wrap, int on);

/* Record the events around every n-th launch only (default 1 = every launch; env CLWRAP_TIMING_EVERY; 0 = none until the next
 * clw_ext_timing_reset / clw_ext_set_timing_every).  An event record between two kernels of a stream keeps the second from being
 * dispatched while the first drains: at 1920x1080 depth 4 that is 5 us per 125-us frame, so bench.py times its throughput loops
 * with no events at all and measures the kernel in one extra pass with events around every launch. */
void clw_ext_set_timing_every(cl_wrap* wrap, uint32_t n);

/* Texture / skybox layer stack from memory instead of PNG files: `rgba` is
 * layers*h*w*4 bytes, layer-major, row-major (the image cl_wrap_load_images builds,
 * opencl_wrap.c:212-332). */
void clw_ext_load_images_raw(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, const uint8_t* rgba,
                             uint32_t width, uint32_t height, uint32_t layers);

/* Register caller-owned device memory as buffer argument `arg_id` (not freed by release). */
void clw_ext_bind_device_buffer(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, void* device_ptr,
                                size_t size);
/* The scene arrays (raytracer args 1-3) are SNAPSHOTTED when first traced: the shim derives its prepared geometry
 * (and, for big scenes, the uniform grid) from them once per (buffers, counts).  A caller that rewrites a bound or
 * uploaded scene buffer in place calls this to have the next launch prepare the scene again. */
void clw_ext_invalidate_scene(cl_wrap* wrap);
/* Device address of a buffer argument (allocates a lazily created buffer). */
void* clw_ext_device_ptr(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id);

/* Optional float radiance output of the trace kernel: 3 floats per work-item, written
 * before the 8-bit pack (reference raytracing.cl:193).  NULL disables. */
void clw_ext_set_debug_rgb(cl_wrap* wrap, void* device_ptr_f32x3);

/* n x n supersampling (anti-aliasing) inside the trace kernel; n = 1 (default), 2, 4 or 8; env CLWRAP_SUPERSAMPLE.
 * With n > 1 a fused trace launch of W x H pixels (or a strip of whole rows of it) traces the n*W x n*H frame the same
 * camera gives -- same im_corner, origin, up and right, w_factor / n, h_factor / n, work-item ids (the RNG seeds) of
 * that frame: bit for bit the samples of a 1-sample render of n*W x n*H -- and writes W x H pixels.  Each sample is
 * clamped to [0, 1] like raytracing.cl:193; the n x n samples of a pixel are added in float32, adjacent pairs along x
 * (log2 n rounds), then adjacent pairs along y, times 1 / n^2, and the mean is packed as usual; the float debug output,
 * when bound, receives the mean (3 floats per OUTPUT pixel).  The samples of a pixel are traced by neighbouring lanes of
 * one wavefront and added in registers: the large frame never exists in memory.  Everything the caller sizes --
 * framebuffer, `pixels` argument, ray buffer (which keeps its one-ray-per-pixel W x H meaning when read back), id
 * offset, row strips -- stays in output pixels.  Work counters and clw_ext_read_tile_costs describe the n*W x n*H frame.
 * Refused with an error and exit(1): launches that are not fused (CLWRAP_FUSE=0, caller-written rays), ranges that
 * are not whole rows, interleaved row bands, linear ids (variant 2), n * n * W * H >= 2^32. */
void clw_ext_set_supersample(cl_wrap* wrap, int n);
int clw_ext_get_supersample(const cl_wrap* wrap);

/* Per-sample cameras: with supersampling factor n in {2, 4, 8} and a table cams[0 .. n*n) in effect, the sample at virtual pixel
 * (vx, vy) -- sub-sample (sx, sy) = (vx mod n, vy mod n) of output pixel (vx div n, vy div n) -- is pixel (vx, vy) of a 1-sample
 * render of the n*W x n*H frame with im_corner, origin, up and right of cams[sy * n + sx] and the launch's w_factor / n, h_factor / n:
 * same primary-ray arithmetic, same ids (RNG seeds), same clamp, resolve and pack as plain supersampling.  A table whose entries all
 * equal the launch camera gives the plain supersampled frame bit for bit.  The ray buffer keeps its meaning (one ray per OUTPUT pixel
 * through the launch camera).  `cams` is copied; count 0 or NULL = no table (and it clears a lens).  Refused at the next trace launch
 * with an error and exit(1): a table whose count is not n * n of the factor then in effect (any table with factor 1 included). */
typedef struct clw_sample_camera { float im_corner[3], origin[3], up[3], right[3]; } clw_sample_camera;   /* 48 bytes */
void     clw_ext_set_sample_cameras(cl_wrap* wrap, const clw_sample_camera* cams, uint32_t count);
/* The table the LAST trace launch used (explicit or lens-derived), in sy * n + sx order -> its count (0 = none); copies the entries
 * if `cap` suffices. */
uint32_t clw_ext_get_sample_cameras(const cl_wrap* wrap, clw_sample_camera* out, uint32_t cap);

/* Thin lens (depth of field) on top of the table: with aperture > 0 every fused trace launch derives its table with
 * clw_host_lens_cameras from the camera latched by the raygen launch (the W x H one), so a driver that moves its camera every frame
 * gets the lens for free.  aperture 0 (default) = pinhole; env CLWRAP_APERTURE, CLWRAP_FOCUS (default focus 1).  An explicit table
 * and the lens are alternatives: the later call wins and clears the other.  Errors (print + exit(1)): aperture negative or not
 * finite, focus <= 0 or not finite; at launch, aperture > 0 with supersampling factor 1 (a lens needs samples). */
void clw_ext_set_lens(cl_wrap* wrap, float aperture, float focus);

/* Moving spheres (object motion blur): with supersampling factor n in {2, 4, 8}, a displacement table disp[0 .. ns) -- three floats per
 * sphere, the movement of its centre while the shutter is open -- and sample times t[0 .. n*n) in effect, let S(t) be the scene whose
 * sphere i has centre fmaf(t, disp[i], c[i]) per component (float32, one rounding; clw_host_spheres_at), radius, material, planes and
 * lights unchanged.  The sample at virtual pixel (vx, vy), k = (vy mod n) * n + (vx mod n), is pixel (vx, vy) of the 1-sample render of
 * the n*W x n*H frame of S(t[k]) -- through the launch camera, or through cams[k] when a table of sample cameras or a lens is in
 * effect; w_factor / n, h_factor / n, ids (RNG seeds), clamp, resolve and pack as plain supersampling.  times == NULL: the times of
 * clw_host_sample_times for the factor in effect at the launch (`count` is then ignored) -- the clock of clw_host_shutter_cameras, so a
 * sphere and a shutter-blurred camera move together.  Both arrays are copied.  disp == NULL or ns == 0 clears the table, and a table
 * whose entries are all zero IS no table: frame, kernel flavour, tile costs and counters are those of the plain launch.
 * Moving launches of deep traces run without the tree-parallel tail and without splitting heavy tiles (a tail node is traced by
 * whichever lane takes it, which would need the owning pixel's time): same image, the tail's speed-up is lost.  The table is staged
 * into LDS behind the prepared geometry and counts in the 16 KiB staging rule: a scene the table pushes over it runs the kernels that
 * read the geometry (and the table) from global memory instead -- same image, another kernel family and its speed.
 * Errors (print + exit(1)): at the call, a displacement or time that is not finite; at the next trace launch, a table with factor 1,
 * count != n * n of the factor then in effect, ns != the scene's sphere count, a scene of more than 256 spheres (the uniform grid's
 * cell lists are built for one set of centres), and whatever plain supersampling refuses. */
void     clw_ext_set_sphere_motion(cl_wrap* wrap, const float* disp /* 3 per sphere */, uint32_t ns, const float* times /* NULL = shutter times */, uint32_t count);
/* The sample times the LAST trace launch used, in sy * n + sx order -> their count (0 = the scene stood still); copies them if `cap`
 * suffices. */
uint32_t clw_ext_get_sample_times(const cl_wrap* wrap, float* out, uint32_t cap);

/* Adaptive supersampling: the n x n samples only where the 1-sample frame shows contrast.  threshold T in [0, 256] turns it on, -1 (the
 * default) off; also CLWRAP_ADAPTIVE=<0..256> in the environment of cl_wrap_init.  It applies to what clw_ext_set_supersample applies to --
 * a fused, tiled trace launch of W x H output pixels, or a strip of whole rows of it -- with a factor n of 2, 4 or 8, and is exact:
 *   1. the base frame B is the launch range traced as the factor-1 launch traces it (camera, ids, RNG seeds, clamp, pack);
 *   2. c(p) = the largest |ch(p) - ch(q)| over the channels R, G, B and the 4-neighbours q of p INSIDE the launch range, on the packed 8-bit
 *      channels of B; p is flagged iff c(p) >= T (T = 0 flags every pixel, T = 256 none);
 *   3. the range is cut into blocks of b x b output pixels, b = 8 / n, from its first row and column 0 (edge blocks are partial) -- the 8x8 tiles
 *      of the virtual frame; a block is refined iff one of its pixels is flagged (clw_host_refine_mask below is THE definition of 2 and 3);
 *   4. the pixels of refined blocks take the value the plain supersampled launch of that range gives them, all others keep B; the float debug
 *      output likewise (un-clamped radiance in kept pixels, the resolved mean in refined ones).
 * One launch is three on the launch stream, none waited for (clw_ext_set_async holds): the base pass -- an ordinary 1-sample launch, which keeps
 * the cost-sorted dispatch and whose costs clw_ext_read_tile_costs returns --, the classifier, which writes the mask and appends the refined tiles
 * to eight per-XCD lists on the device, and the refine pass: the supersampled kernel in its list-driven flavour (clw_ext_last_trace_flags: WT_F_SS |
 * WT_F_LIST, 1 << 19), its grid sized for full lists, a wavefront beyond its list's end leaving at once.  The refine pass keeps the tree-parallel
 * tail, the high-occupancy flavour and the uniform grid as the plain supersampled launch of the frame chooses them; heavy tiles are not split.
 * Work counters add up over both passes; the launch timer brackets all three as one launch.  The pipelined read-back of cl_wrap_output declines
 * while the mode is on.  A strip is defined on its OWN range: the pixels of its first and last row have no neighbour beyond it, so those rows may
 * differ from the same rows of the full frame (the strips of a multi-GPU frame do not compose bit for bit; each equals the definition above).
 * Errors (print + exit(1)): at the call, T outside [-1, 256]; at the next trace launch, the mode with factor 1, with a table of sample cameras, a
 * lens or moving spheres (they change every pixel: a 1-sample contrast test says nothing), a range of more than 4095 blocks either way (a list entry
 * packs block column and row in 12 bits each: at most 16380 pixels per row and rows per range with n = 2, 8190 with n = 4, 4095 with n = 8 -- narrower
 * than what plain supersampling accepts), and whatever plain supersampling refuses; at cl_wrap_init, a CLWRAP_ADAPTIVE that is not such an integer. */
void     clw_ext_set_adaptive(cl_wrap* wrap, int threshold);
int      clw_ext_get_adaptive(const cl_wrap* wrap);
/* The block mask of the LAST trace launch if it was adaptive: one byte (0 / 1) per block, row-major, ceil(rows / b) x ceil(W / b) -> their count
 * (0 = the last launch was not adaptive); copies them if `cap` suffices.  Waits for the launch. */
uint32_t clw_ext_read_refine_mask(cl_wrap* wrap, uint8_t* out, uint32_t cap);

/* Seed offset: the xorshift state of a work-item of every following trace launch starts at (uint32_t)(id + s), `id` being the global id that
 * seeds it otherwise (reference raytracing.cl:33; the VIRTUAL frame's id in a supersampled launch).  Nothing else reads s: pixel positions,
 * buffers and the `pixels` guard keep the id.  It applies to every launch flavour of both arithmetic builds -- fused and caller-written rays,
 * tiled, linear and banded ranges, supersampled, moving and list-driven launches, the uniform grid, the tree-parallel tail.  The work-item with
 * id + s = 0 (mod 2^32) has the stuck generator that id 0 has in the reference.  Default 0 = the reference's seeds; env CLWRAP_SEED_OFFSET=<0..4294967295> (anything else is an error at cl_wrap_init).
 * (The strict build's shallow counting and grid kernels take the offset, and the accumulation below, as a twin flavour -- bit 1 << 20 of
 * clw_ext_last_trace_flags, WT_F_ACC -- which such a launch runs only when s != 0 or it accumulates.) */
void     clw_ext_set_seed_offset(cl_wrap* wrap, uint32_t s);
uint32_t clw_ext_get_seed_offset(const cl_wrap* wrap);

/* Progressive frame accumulation: a still view converges over frames at the price of a plain frame each.  max_frames 0 (default) = off,
 * 1 .. 65536 = on; jitter 0 / 1 = every frame looks through the latched camera / through its own sub-pixel offset.  Env CLWRAP_ACCUMULATE=<0..65536>,
 * CLWRAP_ACC_JITTER=<0|1> (default 1).  The shim keeps, per cl_wrap, a count K (0 at first) and a device buffer `sum` of 3 floats per OUTPUT pixel
 * of the launch range.  A fused trace launch with the mode on and K < max_frames, exactly:
 *   1. is frame f = K: traced as the plain launch would be, but with seed offset s + clw_host_frame_seed(f) (s = clw_ext_set_seed_offset's, the sum
 *      mod 2^32) and, with jitter on, through clw_host_jitter_camera(latched camera, f, n), n the supersampling factor.  Only the trace's camera
 *      words change: the ray buffer keeps its meaning (one ray per output pixel through the latched camera);
 *   2. c_f, per output pixel and channel, is what the plain launch would pack: the sample clamped to [0, 1], or with supersampling the resolved mean;
 *   3. sum = c_0 for f = 0 (a store, no read: the buffer is never cleared), else sum = sum + c_f (float32, one rounding);
 *   4. mean = fminf(sum * r, 1.0f), r = 1.0f / (float)(f + 1) rounded on the host;
 *   5. the framebuffer receives mean packed as usual, (unsigned)(v * 255.0f) per channel;
 *   6. the float debug output, when bound, receives mean;
 *   7. K becomes f + 1.
 * Frame 0 is the plain frame bit for bit, packed and float -- except that the float output of a 1-SAMPLE launch is the CLAMPED value while the mode
 * is on (the un-clamped radiance otherwise); supersampled launches' float output is bit-equal.
 * Holding: with K == max_frames no trace launch is issued -- framebuffer, sum, tile costs, timing log and clw_ext_last_trace_flags stay as the last
 * frame left them; a cl_wrap_output that asks for a read-back still copies.  A converged view costs nothing.  (To read a buffer back WITHOUT
 * adding a frame, ride the read-back on the raygen launch: cl_wrap_output(run = the raygen kernel, read = the buffer); in fused mode that launch
 * only latches the camera again, and equal values do not restart the sum.  Renderer.render_rgb reads the float output that way.)
 * Restart: K := 0 at the next trace launch whenever the key of the image differs from the previous trace launch's -- the eight latched raygen
 * values (by value: a driver that re-uploads equal bytes does not restart), id offset, range, rows and bands; depth, strict, fuse; the
 * supersampling factor; the shadow `through` factor; the seed offset; max_frames and jitter; identity and sizes of the scene, count, texture and
 * skybox arguments and of the framebuffer; any cl_wrap_load_* on raytracer arguments 1-9; clw_ext_invalidate_scene; clw_ext_bind_device_buffer on
 * the framebuffer; clw_ext_reset_accumulation; a trace launch with the mode off in between.  Pure scheduling knobs do not restart it (the image is
 * the same): variant, grid, tile order, the tail's thresholds, counters, the stream (the sum is fenced across clw_ext_set_stream).
 * The tile order of a still view keeps serving its frames: the offset moves what a tile shows by less than a pixel.
 * Errors (print + exit(1)): at the call, max_frames outside [0, 65536] or jitter not 0 / 1; at the next trace launch, the mode together with
 * caller-written rays or CLWRAP_FUSE=0 (the shim must own the camera), a table of sample cameras, a lens, moving spheres (their per-frame
 * decorrelated lens points and times are not built) or adaptive supersampling.  The pipelined read-back of cl_wrap_output declines while the mode is on. */
void     clw_ext_set_accumulate(cl_wrap* wrap, int max_frames, int jitter);
/* K, the number of frames in the sum after the last trace launch; 0 = the mode is off. */
uint32_t clw_ext_get_accumulated(cl_wrap* wrap);
/* The next trace launch starts the sum again at frame 0. */
void     clw_ext_reset_accumulation(cl_wrap* wrap);

/* The primary-hit pass: the geometric buffers of the view, and which object lies under a pixel.  One launch of its own kernel (wt_gbuffer,
 * csrc/whitted_gbuffer.inc, in both arithmetic builds) generates the primary ray of every work-item exactly as the 1-sample trace launch does --
 * the camera and range latched by the last raygen launch, clipped by the raytracer's `pixels` argument (its argument 7), id offset and row bands
 * included -- and runs the first segment's two searches with the trace kernel's own arithmetic: findLightIntersection first, a visible light
 * ending the search (reference primitives.cl:262-318), then the nearest of the spheres, then of the planes, ties keeping the earlier primitive
 * (primitives.cl:322-394); the scene is read as the trace launch reads it (staged in LDS, from global memory, or through the uniform grid).
 * WHICH object wins is decided in the arithmetic of the build in use, so the pass names the object that build's trace launch shades; the winner's
 * depth, point and normal and a light's colour are then evaluated for that one primitive in the reference's arithmetic (IEEE divide and square
 * root, no fused operation) in BOTH builds: the fast build's buffers are the strict build's bit for bit wherever the two agree on the winner.
 * Nothing is shaded: no shadow rays, no skybox fetch, no random numbers.  The pass always sees the LAUNCH camera at pixel centres and the scene
 * as it stands: supersampling factor, lens, sample cameras, moving spheres, adaptive mode, accumulation (its jitter included) and the seed offset
 * have no effect on it, and it does not restart an accumulating view.
 * The channels are planar device buffers owned by the wrapper, indexed by work-item like the framebuffer, one per bit of `channels`:
 *   bit              type     a sphere / plane is hit                                        a light is seen                    miss
 *   CLW_GB_DEPTH     f32      the winning t along the unit primary direction                 the light's t                      +inf
 *   CLW_GB_ID        u32      kind << 30 | index: kind 0 = sphere, 1 = plane; the index is   2 << 30 | index of the light       CLW_ID_NONE
 *                             the one of the caller's array
 *   CLW_GB_NORMAL    f32[3]   the normal findSolidIntersection returns (a plane's is never   0                                  0
 *                             flipped toward the ray)
 *   CLW_GB_POINT     f32[3]   the hit point shading uses: moved by EPSILON along the normal  0                                  0
 *   CLW_GB_ALBEDO    f32[3]   the winner's material colour; a textured plane's texel         the colour findLightIntersection   0
 *                                                                                            returns
 * clw_ext_render_gbuffer launches the pass, without waiting for it, on the wrapper's stream and returns the number of work-items; 0 -- and no
 * launch, no error -- when no raygen launch has latched a camera yet, the raytracer's scene arguments are not all set, or `channels` holds no
 * known bit.  Buffers are allocated when a channel is first asked for and again when the range changes; cl_wrap_release frees them. */
#define CLW_GB_DEPTH  1u
#define CLW_GB_ID     2u
#define CLW_GB_NORMAL 4u
#define CLW_GB_POINT  8u
#define CLW_GB_ALBEDO 16u
#define CLW_GB_ALL    31u
#define CLW_ID_NONE   0xFFFFFFFFu
uint32_t clw_ext_render_gbuffer(cl_wrap* wrap, uint32_t channels);
/* One channel (a single CLW_GB_* bit) of the last pass -> its size in bytes, 4 or 12 per work-item; waits for the pass and copies it if `out` is
 * not NULL and `capacity_bytes` suffices.  0 for a channel the last pass did not write. */
uint32_t clw_ext_read_gbuffer(cl_wrap* wrap, uint32_t channel, void* out, uint32_t capacity_bytes);
/* The device buffer of one channel of the last pass, for consumers on the device (in the order of the wrapper's stream); NULL for a channel
 * the last pass did not write.  The next pass over another range frees it. */
void*    clw_ext_gbuffer_device_ptr(cl_wrap* wrap, uint32_t channel);
/* What lies under pixel (x, y) of the FRAME: one launch of the same kernel on that one-pixel range -- the pass's arithmetic, so the values are
 * the entry of that pixel in the buffers bit for bit -- and a 44-byte read-back; the call waits for it.  Returns 1, or 0 with `out` untouched
 * when no camera is latched (see above) or the pixel is not one of the wrapper's work-items (outside the frame, outside its id range or its row
 * bands).  The buffers of the last pass stay as they are. */
typedef struct clw_pick { uint32_t id; float depth, point[3], normal[3], albedo[3]; } clw_pick;   /* 44 bytes */
int      clw_ext_pick(cl_wrap* wrap, uint32_t x, uint32_t y, clw_pick* out);
/* The pass's launches are logged under this id in clw_ext_timing_get (a pick is not logged). */
#define CLW_TIMING_GBUFFER 0x47425546u

/* The selection overlay: shows which objects are selected -- an outline around them, a tint over them, a line along every object boundary --
 * composed on the device from the traced frame and the ids of the primary-hit pass, both read where they lie.  Integer arithmetic only, the
 * same in both builds; clw_host_overlay is THE definition, and the device pass (wt_overlay, csrc/whitted_overlay.inc) equals it bit for bit.
 * For pixel p = (x, y) of a width x rows image: sel(p) is true iff ids[p] equals one of the `count` words of `sel` (any 32-bit value may be
 * listed; CLW_ID_NONE selects the sky); pixels outside the image are absent, neither selected nor different.  In this order:
 *   1. c = frame[p] & 0x00FFFFFF;
 *   2. with CLW_OV_EDGES: if (x + 1 < width && ids[p] != ids[p + 1]) || (y + 1 < rows && ids[p] != ids[p + width]), c = edge_rgb & 0xFFFFFF;
 *   3. with CLW_OV_FILL and sel(p): every 8-bit channel becomes (c_ch * (256 - a) + t_ch * a + 128) >> 8, a = fill_alpha, t = fill_rgb
 *      (a = 0 leaves c as it is, a = 256 gives t exactly);
 *   4. with CLW_OV_OUTLINE and !sel(p): if some present q with |qx - x| <= radius && |qy - y| <= radius has sel(q), c = outline_rgb & 0xFFFFFF
 *      -- an OUTER band: a selected object is never covered by its own outline;
 *   5. out[p] = c (the top byte is 0).
 * Refused (0 returned, nothing written): unknown flag bits, flags == 0, OUTLINE with a radius outside 1..4, FILL with alpha > 256, count > 64,
 * count > 0 with sel == NULL, a width or rows of zero (and a NULL frame, ids, style or out).  count == 0 is legal: only EDGES can then draw. */
#define CLW_OV_OUTLINE 1u
#define CLW_OV_FILL    2u
#define CLW_OV_EDGES   4u
#define CLW_OV_ALL     7u
typedef struct clw_overlay {      /* 24 bytes */
    uint32_t flags;               /* CLW_OV_OUTLINE | CLW_OV_FILL | CLW_OV_EDGES */
    uint32_t radius;              /* outline width in pixels, 1..4 (read only with OUTLINE) */
    uint32_t outline_rgb;         /* 0x00RRGGBB */
    uint32_t fill_rgb;            /* 0x00RRGGBB */
    uint32_t fill_alpha;          /* 0..256 (read only with FILL) */
    uint32_t edge_rgb;            /* 0x00RRGGBB */
} clw_overlay;
int clw_host_overlay(const uint32_t* frame, const uint32_t* ids, uint32_t width, uint32_t rows,
                     const clw_overlay* style, const uint32_t* sel, uint32_t count, uint32_t* out);   /* 1 = done, 0 = refused */
/* clw_ext_render_overlay composes the overlay of the wrapper's range on its stream, without waiting: an id-only primary-hit pass over the range
 * the next trace launch would cover (as clw_ext_render_gbuffer, into an id buffer the overlay owns), then wt_overlay over those ids and the
 * raytracer's framebuffer argument (its argument 10) as the last launch left it, in stream order with that launch, into a packed u32 frame the
 * wrapper owns.  Returns the number of work-items.  The traced framebuffer is never written; the buffers of clw_ext_render_gbuffer (channels,
 * what an earlier clw_ext_read_gbuffer returned), an accumulating view, its float sum and the tile order are left alone.
 * Returns 0 -- no launch, and the process goes on -- when the style or the selection is refused as above, no camera is latched, no scene is
 * bound, no framebuffer is registered (or it is smaller than the range), the wrapper has row bands, or the range is not a whole number of rows.
 * A strip (an id offset of whole rows) is composed on its OWN rows: rows of other strips are absent, so a strip's overlay can differ from the
 * full frame's within `radius` rows of its edges (and EDGES in its last row).
 * Buffers are allocated at first use and again when the range changes; cl_wrap_release frees them.  The id pass is logged under
 * CLW_TIMING_GBUFFER, wt_overlay under CLW_TIMING_OVERLAY in clw_ext_timing_get.
 * Not built: a latched mode in which cl_wrap_output hands the unchanged drivers the overlay frame instead of the traced one -- it would touch
 * the blocking and the pipelined read-back paths. */
uint32_t clw_ext_render_overlay(cl_wrap* wrap, const clw_overlay* style, const uint32_t* sel, uint32_t count);
/* The overlay frame of the last clw_ext_render_overlay -> its size in bytes, 4 per work-item (0 = there is none); waits for the pass and
 * copies it if `out` is not NULL and `capacity_bytes` suffices. */
uint32_t clw_ext_read_overlay(cl_wrap* wrap, void* out, uint32_t capacity_bytes);
/* Its device buffer, for consumers on the device (in the order of the wrapper's stream); NULL before the first pass.  A pass over another
 * range frees it. */
void*    clw_ext_overlay_device_ptr(cl_wrap* wrap);
/* Test seam: uploads a caller's synthetic frame and ids (width x rows words each), runs the kernel instantiation and launch shape that
 * clw_ext_render_overlay would run for this style, and reads the result back into `out`.  Returns width * rows, or 0 -- nothing launched,
 * `out` untouched -- when refused as clw_host_overlay refuses (or width * rows does not fit 32 bits).  Waits. */
uint32_t clw_ext_unit_overlay(cl_wrap* wrap, const uint32_t* frame, const uint32_t* ids, uint32_t width, uint32_t rows,
                              const clw_overlay* style, const uint32_t* sel, uint32_t count, uint32_t* out);
#define CLW_TIMING_OVERLAY 0x4F564C59u

/* The visible-object table: which objects show inside a rectangle of the view, each with its pixel count, screen bounding box, depth range and
 * the sums its centroid comes from -- what rubber-band selection, placing a label or a gizmo, zooming or focusing on an object and a
 * visibility list need -- reduced on the device from the id and depth channels of the primary-hit pass, read where they lie: a few 48-byte
 * records travel to the host, not the channels.  Integer work only (comparisons, counts, minima, maxima, integer sums), the same in both
 * builds; clw_host_object_stats is THE definition, and the device pass (wt_objects_reduce, wt_objects_compact: csrc/whitted_objects.inc)
 * equals it bit for bit.
 * Take a range of whole rows -- width x rows pixels, its first row being row `first_row` of the frame --, its id channel (CLW_GB_ID words),
 * optionally its depth channel, and a rectangle in FRAME pixels (NULL = the whole frame), clipped in 64-bit arithmetic to the columns of the
 * frame and the rows of the range.  counts[3] = (spheres, planes, lights); an id is KNOWN if its kind is 0..2 and its index below that kind's
 * count, or if it is CLW_ID_NONE.  The table has one record per distinct known id among the pixels of the range inside the rectangle, sorted
 * by id ascending as uint32: spheres, then planes, then lights, CLW_ID_NONE last.  A pixel whose id is not known enters no record and is
 * counted in summary.foreign (the primary-hit pass writes no such id).  summary.pixels = the pixels of the range inside the rectangle, foreign
 * ones included; summary.objects = the number of records, whatever `capacity` is: the first min(objects, capacity) are written (out == NULL
 * counts as capacity 0).  Depth extremes are defined on BIT PATTERNS read as uint32, so a NaN needs no rule; for the pass's own depths (t > 0,
 * +inf for the sky) that is the order of the values.
 * Refused (0 returned, nothing written): a NULL ids, counts or summary, a width or rows of zero, a rectangle of zero width or height,
 * counts[0] + counts[1] + counts[2] + 1 > 1 << 24, width * rows not fitting 30 bits (and first_row + rows > 2^32: y would not fit).  A
 * rectangle that misses the range is NOT refused: objects = pixels = 0. */
typedef struct clw_rect { uint32_t x, y, width, height; } clw_rect;                 /* 16 bytes, frame pixels */
typedef struct clw_object_stat {                                                     /* 48 bytes */
    uint32_t id;                 /* as CLW_GB_ID */
    uint32_t pixels;             /* pixels of the rectangle that show it */
    uint32_t x0, y0, x1, y1;     /* inclusive bounding box of those pixels, FRAME coordinates */
    float    depth_min, depth_max;   /* the two depths whose bit patterns, read as uint32, are smallest / largest; 0, 0 without a depth channel */
    uint64_t sum_x, sum_y;       /* sums of the frame coordinates of those pixels: centroid = sum / pixels */
} clw_object_stat;
typedef struct clw_object_summary { uint32_t objects, pixels, foreign, reserved; } clw_object_summary;   /* 16 bytes */
int clw_host_object_stats(const uint32_t* ids, const float* depth /* or NULL */, uint32_t width, uint32_t rows, uint32_t first_row,
                          const clw_rect* rect, const uint32_t counts[3], clw_object_stat* out, uint32_t capacity,
                          clw_object_summary* summary);                                                   /* 1 = done, 0 = refused */
/* Two tables sorted by id -> the table of both, sorted: an object in both has its pixels and sums added, its boxes united, its depth extremes
 * combined by bit pattern.  Returns the merged count and writes the first min(count, capacity) records (`out` may be neither input).  The
 * tables of two strips of a frame, merged, are the frame's table exactly: boxes and sums are in frame coordinates. */
uint32_t clw_host_merge_object_stats(const clw_object_stat* a, uint32_t na, const clw_object_stat* b, uint32_t nb, clw_object_stat* out,
                                     uint32_t capacity);
/* clw_ext_object_stats builds the table of the wrapper's range on its stream and WAITS for it (as clw_ext_pick): an id + depth primary-hit
 * pass over the range the next trace launch would cover (as clw_ext_render_gbuffer, into two buffers the table owns), a clear of the slot
 * table, wt_objects_reduce and wt_objects_compact -- first_row and counts being the launch's own -- then a read-back of the 16-byte summary
 * and of min(objects, capacity) records.  Returns 1.  The slot table is direct-indexed, one 48-byte slot per possible id, so a scene of n
 * primitives costs 96 (n + 1) bytes of device memory from the first call on.
 * Returns 0 -- no launch, `out` and `summary` untouched, and the process goes on -- when the arguments are refused as above, no camera is
 * latched, no scene is bound, the wrapper has row bands, or the range is not a whole number of rows.
 * The traced framebuffer, the buffers of clw_ext_render_gbuffer and of the overlay, an accumulating view, its count and the tile order are
 * left alone.  A strip (an id offset of whole rows) gives the table of its OWN rows in frame coordinates: merge the strips' tables.
 * Buffers are allocated at first use and again when the range or the counts change; cl_wrap_release frees them.  The id pass is logged under
 * CLW_TIMING_GBUFFER; the clear and the two kernels, as one entry, under CLW_TIMING_OBJECTS in clw_ext_timing_get.
 * Not built: a latched mode in which every trace launch is followed by its table, and with it a per-frame automatic table a driver could
 * poll -- each call is one explicit pass; nor a device-resident result for consumers on the device. */
int clw_ext_object_stats(cl_wrap* wrap, const clw_rect* rect, clw_object_stat* out, uint32_t capacity, clw_object_summary* summary);
/* Test seam: uploads a caller's synthetic id field (and depth field, or NULL), runs the clear, the two kernels and the read-back that
 * clw_ext_object_stats would run for them, with the caller's first_row and counts.  Returns 1, or 0 -- nothing launched, `out` and `summary`
 * untouched -- when refused as clw_host_object_stats refuses.  Waits. */
int clw_ext_unit_object_stats(cl_wrap* wrap, const uint32_t* ids, const float* depth, uint32_t width, uint32_t rows, uint32_t first_row,
                              const clw_rect* rect, const uint32_t counts[3], clw_object_stat* out, uint32_t capacity,
                              clw_object_summary* summary);
#define CLW_TIMING_OBJECTS 0x4F424A53u

/* Camera models beside the pinhole: the orthographic view (parallel rays: the top / front / side views of an editor; size does not depend on
 * distance) and the equirectangular panorama (a latitude-longitude frame of up to 360 x 180 degrees: the environment map OUT of a tracer that
 * takes one in).  clw_host_projection_rays is THE definition: it writes the 64-byte records {origin, 0, dir, 0, 0,0,0,0, 0,0,0,0} of the global
 * ids [id_begin, id_end) of the camera's width x height frame, x = id % width, y = id / width, and returns 1 -- or 0, writing nothing, for what it
 * refuses.  Every ray is a few float32 operations, one rounding each, no fused operation, IEEE square root and divide, on terms the host resolves
 * once per (camera, frame, projection); the device (csrc/whitted_projection.inc) performs the same operations on the same terms and equals it bit for bit.
 *   axis a: `axis`, or -- all zero -- the centre of the camera's image plane relative to its origin, im_corner + right (w_factor W / 2) - up
 *     (h_factor H / 2) [double, rounded to float]; normalised once: a / sqrtf(a.a) [float32].
 *   CLW_PROJ_PERSPECTIVE: the pinhole of raygen.cl:13-21 -- direction normalize(v), v = im_corner + right w_factor x - up h_factor y [float32, in
 *     that order], origin the camera's.
 *   CLW_PROJ_ORTHO: every ray has direction a; the origin of pixel (x, y) is the camera origin + v, v as above: the image plane is the near plane.
 *     ortho_width > 0 first rescales the plane about its centre so that the frame's width, |right| w_factor W, spans that many world units:
 *     w_factor and h_factor times s = ortho_width / (|right| |w_factor| W), im_corner moved accordingly [double, each stored to float].
 *   CLW_PROJ_EQUIRECT: pixel centres are sampled -- longitude theta(x) = ((x + 1/2) / W - 1/2) h_span, latitude phi(y) = (1/2 - (y + 1/2) / H)
 *     v_span, evaluated as (2x + 1 - W) / 2W and (H - 1 - 2y) / 2H so that mirrored columns and rows get exactly opposite angles -- and the
 *     direction is cos(phi) (sin(theta) r + cos(theta) a) + sin(phi) u, r and u the camera's right and up made orthonormal to a (Gram-Schmidt:
 *     r first, then u against both).  All of this in double, in clw_host_projection_tables, which fills a column table of W float4
 *     {sin(theta) r + cos(theta) a, 0} and a row table of H float4 {cos(phi), sin(phi) u}; the ray is normalize(col[x].xyz * row[y].x +
 *     row[y].yzw) [float32, multiply then add], its origin the camera's.  Returns 1, or 0 for what is refused and for the other two models.
 * Refused: a NULL pointer, an empty frame, ids outside it, an unknown model, reserved != 0, an ortho_width that is not finite or negative, a span
 * that is not finite, negative or above 360 / 180 (every field is checked whatever the model), an axis or a camera value that is not finite, a
 * zero axis when the camera's own centre direction is zero too (shorter than 1e-6 of the image plane's half diagonal: what float32 rounding leaves
 * of a plane centred on the origin is no direction; or a normalised to something not finite), ORTHO with ortho_width > 0 over a camera
 * of zero `right` or w_factor, EQUIRECT with a `right` parallel to the axis or an `up` in the plane of both. */
enum { CLW_PROJ_PERSPECTIVE = 0, CLW_PROJ_ORTHO = 1, CLW_PROJ_EQUIRECT = 2 };
typedef struct clw_projection {      /* 32 bytes */
    uint32_t model;
    float axis[3];        /* view direction; all zero = the direction from the camera origin to the centre of its image plane */
    float ortho_width;    /* ORTHO: world units the frame's width spans; 0 = the camera's own image plane as it stands */
    float h_span, v_span; /* EQUIRECT: degrees covered, (0, 360] and (0, 180]; 0 = 360 / 180 */
    uint32_t reserved;    /* 0 */
} clw_projection;
/* (the camera structure is declared further down with its helper; a declaration of the tag is enough here) */
struct clw_camera;
int clw_host_projection_rays(const struct clw_camera* cam, const clw_projection* proj, uint64_t id_begin, uint64_t id_end, float* rays16);
int clw_host_projection_tables(const struct clw_camera* cam, const clw_projection* proj, float* col4 /* 4 W floats */, float* row4 /* 4 H floats */);
/* The convenience most callers want: an orthographic view from `origin` along `look` (need not be normalised) whose frame's width spans
 * `view_width` world units.  The camera has `right` and `up` as clw_host_perspective builds them, the image plane THROUGH the origin, square
 * pixels and w_factor = h_factor = view_width / width; the projection has axis = look / |look| and ortho_width = view_width (`right` is not unit
 * when `look` leaves the horizontal: the rescaling above makes the span hold whatever its length).  Returns 0 for a NULL pointer, an empty frame,
 * a look that is zero, not finite or vertical, a view_width that is not finite or not positive, else 1. */
int clw_host_ortho_camera(const float origin[3], const float look[3], float view_width, uint32_t width, uint32_t height, struct clw_camera* cam,
                          clw_projection* proj);
/* The model of the wrapper's launches and inspection passes; NULL or model CLW_PROJ_PERSPECTIVE = the pinhole, the default (then nothing here
 * applies and every launch is what it was).  Env CLWRAP_PROJECTION=ortho|equirect, CLWRAP_ORTHO_WIDTH=<float >= 0>, CLWRAP_PANO_SPAN=<h>,<v>:
 * with them the unchanged raypng / rayinteractive drivers render a plan view or a panorama.  With a model set:
 *   - the raygen launch latches its eight arguments as ever; the trace launch -- or a read of the ray buffer -- materialises the records of the
 *     model with wt_raygen_proj (logged under the raygen kernel's id in clw_ext_timing_get), and the trace runs the ray-buffer flavour (WT_F_RAYS in
 *     clw_ext_last_trace_flags) it would run for a caller's ray buffer, with the ids, width, height and bands of the generating launch.  It is NEVER
 *     fused, and it takes no direction for unit: the frame is bit for bit the frame of the same records uploaded by a caller;
 *   - the records stay valid while the latched values, the range and the projection do not change: a still view generates them once.  The two
 *     tables of a panorama belong to the wrapper and are rebuilt only when the camera's right or up, the frame size, the axis or a span changes;
 *   - rays a caller wrote (the buffer's pointer handed out, clw_ext_device_ptr) are traced as written, as without a model;
 *   - the primary-hit pass and everything built on it -- clw_ext_render_gbuffer, clw_ext_pick, clw_ext_render_overlay, clw_ext_object_stats -- see
 *     the model's rays where they see the pinhole's (depth is the distance along the unit direction from the ray's origin: for ORTHO, from the
 *     image plane); they return 0 when the projection cannot be resolved for the latched camera;
 *   - the pipelined read-back of cl_wrap_output declines.
 * Errors (print + exit(1)): at the call or at cl_wrap_init, a field the definition refuses whatever the camera; at the trace launch, a projection
 * that cannot be resolved for the latched camera, and the modes that need the fused launch: supersampling, a lens or a table of sample cameras,
 * moving spheres, adaptive supersampling, frame accumulation.
 * Not built: a fused projected trace flavour (the cost of the ray buffer's round trip is measured in DESIGN.md), and with it the modes above. */
void clw_ext_set_projection(cl_wrap* wrap, const clw_projection* proj);
void clw_ext_get_projection(const cl_wrap* wrap, clw_projection* out);
/* Test seam: runs wt_raygen_proj for the ids [id_begin, id_end) of a synthetic camera's frame into a scratch buffer and reads the records back
 * into `out_rays` (16 floats each).  Needs no scene.  Returns 1, or 0 -- nothing launched, `out_rays` untouched -- when refused as
 * clw_host_projection_rays refuses, and for CLW_PROJ_PERSPECTIVE (whose kernel is wt_raygen).  Waits; not logged in the timing log. */
int clw_ext_unit_projection(cl_wrap* wrap, const struct clw_camera* cam, const clw_projection* proj, uint64_t id_begin, uint64_t id_end,
                            float* out_rays);

/* Ray-traced ambient occlusion: the view shaded by geometry alone (the "clay" view of an editor) -- how much of the hemisphere above every
 * visible point is open within `radius` -- traced on the device from the point, normal and id channels of the primary-hit pass: K short any-hit
 * rays per pixel against the spheres and planes of the scene.  All of its arithmetic is defined here, on the host: clw_host_ao_dirs,
 * clw_host_ao_open and clw_host_ao_resolve are THE definition, and the device pass (wt_ao_trace, wt_ao_resolve: csrc/whitted_ao.inc) equals
 * them bit for bit in both builds.  float32 operations are rounded once each, never fused; square root and divide are IEEE.
 * (a) clw_host_ao_dirs: the direction table, indexed [j][i], pattern j = 0..15, ray i = 0..K-1; the only trigonometry and the only double
 *     arithmetic of the feature.  In double: u1 = (i + (j + 0.5) / 16) / K; u2 = frac(i * 0.6180339887498949 + rev4(j) / 16), rev4 = the 4-bit
 *     reversal of j; l = (sqrt(u1) cos(2 pi u2), sqrt(u1) sin(2 pi u2), sqrt(1 - u1)), each component rounded once to float, w = 0.
 *     Cosine-weighted (the open fraction IS the estimate), stratified in elevation per pixel, rotated and jittered across the 16 patterns of a
 *     4 x 4 block of pixels; l.z >= sqrt(0.03125 / K) > 0.
 * (b) clw_host_ao_open: point and normal (3 floats per pixel) and ids (CLW_GB_ID words), planar, of a range of `rows` whole rows whose first
 *     row is row `first_row` of the frame; spheres / planes = the 96-byte records of the scene arrays, read through the prepared words
 *     {centre, +-r * r} and {n}, {p0} the device reads.  For pixel (x, y) of the range, p = y * width + x:
 *       - ids[p] is neither a sphere (kind 0, index < ns) nor a plane (kind 1, index < np) -- the sky, a light, any other word: open[p] = K;
 *       - else o = point[p] (the EPSILON-offset point) and n = normal[p] as stored (a plane's normal is not flipped toward the viewer, as in
 *         the reference's shading), and the branchless orthonormal basis, every operation left to right:
 *           sg = copysignf(1, n.z); a = -1 / (sg + n.z); b = n.x * n.y * a;
 *           t = (1 + sg * n.x * n.x * a, sg * b, -sg * n.x); u = (b, sg + n.y * n.y * a, -n.y);
 *       - pattern j = (x & 3) | ((first_row + y) & 3) << 2; ray i has direction d = t * l.x + u * l.y + n * l.z, l = dirs[j][i], per component
 *         three products, then two sums left to right; it is NOT normalised;
 *       - ray i is occluded iff some sphere 0..ns-1 (whatever its material) or some plane 0..np-1 gives hit && t <= radius, with
 *           sphere {c, q}: A = d.d; v = o - c; C = v.v - |q|; B = v.d; D = B * B + (-(A * C)); s = sqrtf(D); t0 = (-B - s) / A;
 *                          t = t0 < 0 ? (-B + s) / A : t0; hit = !(D < 0) && !(t <= 0);
 *           plane {n, p0}: num = (p0 - o).n; B = d.n; t = num / B; hit = !(B == 0) && !(t <= 0);
 *         (a dot product is x x' + y y' + z z' left to right) -- the primary-hit pass's own evaluation of its winner.  Lights never occlude;
 *       - open[p] = the number of rays that are not occluded.  The comparisons as written decide a zero or NaN normal: a NaN direction is
 *         never occluded.
 * (c) clw_host_ao_resolve, integers only.  W(p) = {p}, or with CLW_AO_FILTER the present pixels q with x - 2 <= qx <= x + 1, y - 2 <= qy <=
 *     y + 1 and ids[q] == ids[p] (any 4 x 4 window holds every pattern once); S = the sum of open over W(p), m = |W(p)|;
 *     v = (255 S + (m K >> 1)) / (m K); v' = 255 - (((255 - v) strength + 128) >> 8); out[p] = v' * 0x010101, or with CLW_AO_COMPOSE every
 *     8-bit channel c of frame[p] & 0xFFFFFF becomes (c v' + 127) / 255.  The top byte is 0.
 * Refused (0 returned, nothing written), by every function where it applies: a NULL pointer (ns or np > 0 with its array NULL; COMPOSE with a
 * NULL frame), unknown flag bits, rays outside 1..32, a radius that is NaN or <= 0 (+inf = unlimited is legal), strength > 256, a width or rows
 * of zero, width * rows not fitting 30 bits. */
#define CLW_AO_FILTER  1u   /* average the 4x4 interleave pattern away, among pixels of the same id */
#define CLW_AO_COMPOSE 2u   /* multiply the traced frame by the result instead of showing it as grey */
typedef struct clw_ao {     /* 16 bytes */
    uint32_t flags;         /* CLW_AO_FILTER | CLW_AO_COMPOSE; 0 is legal */
    uint32_t rays;          /* K, 1..32 rays per pixel */
    float    radius;        /* > 0; +inf = unlimited; NaN, 0 and negative are refused */
    uint32_t strength;      /* 0..256: how much of the occlusion shows */
} clw_ao;
int clw_host_ao_dirs(uint32_t K, float* dirs4 /* 16 * K float4 */);                                         /* 1 = done, 0 = refused */
int clw_host_ao_open(const float* point, const float* normal, const uint32_t* ids, uint32_t width, uint32_t rows, uint32_t first_row,
                     const void* spheres, uint32_t ns, const void* planes, uint32_t np, const clw_ao* ao, const float* dirs4,
                     uint8_t* open_u8);
int clw_host_ao_resolve(const uint8_t* open_u8, const uint32_t* ids, const uint32_t* frame /* or NULL without COMPOSE */, uint32_t width,
                        uint32_t rows, const clw_ao* ao, uint32_t* out_u32);
/* clw_ext_render_ao composes the pass of the wrapper's range on its stream, without waiting: (1) a point + normal + id primary-hit pass over
 * the range the next trace launch would cover (as clw_ext_render_gbuffer -- every camera model -- into buffers the pass owns); (2) wt_ao_trace
 * into a u8 count buffer, the scene read as the primary-hit pass reads it (staged in LDS, from global memory, or through the uniform grid);
 * (3) wt_ao_resolve over the counts, the ids and, with COMPOSE, the raytracer's framebuffer argument (its argument 10) as the last launch left
 * it, into a packed u32 frame the wrapper owns.  Returns the number of work-items.
 * Returns 0 -- no launch, and the process goes on -- for what the definition refuses, when no camera is latched or no scene is bound, the
 * wrapper has row bands, the range is not a whole number of rows, or, with COMPOSE, no framebuffer is registered or it is smaller than the range.
 * A strip (an id offset of whole rows) is traced with FRAME row numbers, so the strips' counts concatenate to the frame's exactly; it is resolved
 * on its OWN rows (rows of other strips are absent from a window), as the overlay is.
 * The traced framebuffer, the buffers of clw_ext_render_gbuffer, the overlay, the object table, an accumulating view, its count and the tile
 * order are left alone.  The direction table is rebuilt only when K changes; the other buffers are allocated at first use and again when the
 * range changes; cl_wrap_release frees them.  The primary-hit pass is logged under CLW_TIMING_GBUFFER, wt_ao_trace under CLW_TIMING_AO,
 * wt_ao_resolve under CLW_TIMING_AO_RESOLVE in clw_ext_timing_get.
 * Not built: a latched mode in which cl_wrap_output hands the unchanged drivers the AO frame; facing the hemisphere toward the viewer (a plane
 * seen from behind is shaded by what lies on its normal's side); accumulation of AO over frames. */
uint32_t clw_ext_render_ao(cl_wrap* wrap, const clw_ao* ao);
/* What the last clw_ext_render_ao left: what = 0 the frame (u32 per work-item), 1 the open-ray counts (u8 per work-item) -> its size in bytes
 * (0 = there is none, or `what` is neither); waits for the pass and copies it if `out` is not NULL and `capacity_bytes` suffices. */
uint32_t clw_ext_read_ao(cl_wrap* wrap, uint32_t what, void* out, uint32_t capacity_bytes);
/* Its device buffer, for consumers on the device (in the order of the wrapper's stream); NULL before the first pass.  A pass over another
 * range frees it. */
void*    clw_ext_ao_device_ptr(cl_wrap* wrap, uint32_t what);
/* Test seam: uploads synthetic channels and runs the wt_ao_trace instantiation and launch shape clw_ext_render_ao would run for the wrapper's
 * bound scene, grid setting and variant; reads the counts back into `open_u8`.  Returns width * rows, or 0 -- nothing launched, `open_u8`
 * untouched -- when refused as clw_host_ao_open refuses or no scene is bound.  Waits; not logged. */
uint32_t clw_ext_unit_ao_open(cl_wrap* wrap, const float* point, const float* normal, const uint32_t* ids, uint32_t width, uint32_t rows,
                              uint32_t first_row, const clw_ao* ao, uint8_t* open_u8);
/* Test seam: wt_ao_resolve over synthetic counts, ids and (with COMPOSE) frame -> `out`.  Needs no scene.  Returns width * rows, or 0 when
 * refused as clw_host_ao_resolve refuses.  Waits; not logged. */
uint32_t clw_ext_unit_ao_resolve(cl_wrap* wrap, const uint8_t* open_u8, const uint32_t* ids, const uint32_t* frame, uint32_t width,
                                 uint32_t rows, const clw_ao* ao, uint32_t* out);
#define CLW_TIMING_AO         0x414F5452u
#define CLW_TIMING_AO_RESOLVE 0x414F5253u

/* Ray queries: where a CALLER's rays meet the scene -- from anywhere, toward anything, no camera involved: drop an object onto what lies below
 * it, snap to the surface under a point, measure a distance, ask whether a light sees a sphere, scan a fan of sensor rays, send a second bounce
 * from the points a first query returned.  A nearest-hit query answers a clw_hit per ray, an any-hit query one byte.  All of the arithmetic is
 * defined here, on the host: clw_host_cast_rays and clw_host_occluded_rays are THE definition, and the device pass (wt_cast:
 * csrc/whitted_cast.inc) equals them bit for bit in both builds.  float32 operations are rounded once each, never fused; square root and divide
 * are IEEE.  spheres / planes / lights = the 96- / 96- / 48-byte records of the scene arrays, read through the prepared words the device reads:
 * {centre, +-r * r} per sphere (sign bit set = material.transperent != 0), {n}, {p0} per plane, {centre, r * r} per light.
 * Per ray {o = origin, tmax, d = dir, ignore}:
 *   - d is used as given, NOT normalised; t is in units of |d|: the ray from a to b with d = b - a and tmax = 1 ends exactly at b.
 *   - The primitives that take part: the kinds enabled in `flags`, in the order spheres 0..ns-1, planes 0..np-1, lights 0..nl-1 (a light is the
 *     plain sphere of its radius).  A primitive whose id word -- kind << 30 | index as CLW_GB_ID: kind 0 sphere, 1 plane, 2 light -- equals
 *     `ignore` is skipped (the object a ray starts on); CLW_ID_NONE skips nothing.  With CLW_CAST_OPAQUE a sphere whose prepared r * r word has
 *     its sign bit set is skipped: the ray passes transparent spheres.
 *   - The tests, a dot product being x x' + y y' + z z' left to right:
 *       sphere or light {c, q}: A = d.d; v = o - c; C = v.v - |q|; B = v.d; D = B * B + (-(A * C)); s = sqrtf(D); t0 = (-B - s) / A;
 *                               t = t0 < 0 ? (-B + s) / A : t0; hit = !(D < 0) && !(t <= 0);
 *       plane {n, p0}:          num = (p0 - o).n; B = d.n; t = num / B; hit = !(B == 0) && !(t <= 0);
 *     -- the primary-hit pass's own evaluation of its winner.  A ray that starts inside a sphere meets its far side.
 *   - A primitive is a CANDIDATE iff hit && t <= tmax.  So a NaN t, a NaN ray or a NaN tmax meets nothing -- this is NOT the trace kernel's
 *     rule, under which a poisoned ray "hits" the last primitive --, a zero direction meets nothing, and tmax = +inf means unlimited.
 *   - Nearest: a candidate replaces the best iff t < tbest; equal t keeps the earlier primitive in the order above.
 *       miss: {t = +inf, id = CLW_ID_NONE, normal = 0, point = 0};
 *       hit:  t, id, point = d * t + o per component (the product, then the sum; WITHOUT the EPSILON offset of the primary-hit pass's point
 *             channel), normal = (point - c) / sqrtf((point - c).(point - c)) per component for a sphere or a light, the stored normal for a
 *             plane (never flipped toward the ray).
 *   - Any: blocked[k] = 1 iff ray k has a candidate, else 0.
 * Refused (0 returned, nothing written): a NULL pointer (a count > 0 with its array NULL), n == 0 or n >= 1 << 30, a flag bit beside the five
 * below, no kind bit set. */
typedef struct clw_ray { float origin[3]; float tmax; float dir[3]; uint32_t ignore; } clw_ray;   /* 32 bytes */
typedef struct clw_hit { float t; uint32_t id; float normal[3]; float point[3]; } clw_hit;        /* 32 bytes */
#define CLW_CAST_SPHERES 1u
#define CLW_CAST_PLANES  2u
#define CLW_CAST_LIGHTS  4u     /* light spheres as plain geometry, kind 2 ids */
#define CLW_CAST_KINDS   7u
#define CLW_CAST_OPAQUE  8u     /* transparent spheres (material.transperent != 0) let the ray pass */
int clw_host_cast_rays(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                       const void* lights, uint32_t nl, clw_hit* hits);          /* 1 = done, 0 = refused */
int clw_host_occluded_rays(const clw_ray* rays, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns, const void* planes, uint32_t np,
                           const void* lights, uint32_t nl, uint8_t* blocked);   /* blocked[k] = 0 / 1 */
/* The queries on the device, against the wrapper's bound scene (the raytracer's arguments 1-6: the three arrays and their counts); no camera,
 * no ray buffer, no framebuffer and no textures are needed.  The scene is prepared if no launch has prepared it yet, exactly as a primary-hit
 * pass does, and read as that pass reads it: staged in LDS, from global memory, or through the uniform grid (which only skips tests: the answer
 * is the definition's in every flavour).  A call after clw_ext_invalidate_scene sees the rewritten scene.
 * clw_ext_cast_rays / clw_ext_occluded_rays take HOST arrays: they upload the rays into a buffer the feature owns, launch on the wrapper's
 * stream, wait, read the answers back and return n.  The buffers are allocated at first use, grown when n grows and freed by cl_wrap_release.
 * clw_ext_cast_rays_device takes the caller's DEVICE memory (n clw_ray; n clw_hit or n bytes): exactly one of d_hits / d_blocked is non-NULL and
 * selects nearest or any.  It launches on the wrapper's stream -- the caller's after clw_ext_set_stream --, does not wait, and returns n; the
 * caller orders its own reads and writes on that stream.
 * All three return 0 -- nothing launched, the outputs untouched, and the process goes on -- for what the definition refuses (for the device
 * entry point also both or neither output given) and when no scene is bound.
 * The framebuffer, the buffers of clw_ext_render_gbuffer, the overlay, the object table and the AO pass, an accumulating view and its count, the
 * tile order and clw_ext_last_trace_flags are left alone.  Launches are logged under CLW_TIMING_CAST in clw_ext_timing_get.
 * Not built: sorting incoherent rays by grid cell before the launch; per-ray flags; the texel or the material of the hit; a latched "bounce"
 * helper that turns hits into the next rays on the device. */
uint32_t clw_ext_cast_rays(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, clw_hit* hits);          /* host arrays; waits */
uint32_t clw_ext_occluded_rays(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, uint8_t* blocked);  /* host arrays; waits */
uint32_t clw_ext_cast_rays_device(cl_wrap* wrap, const void* d_rays, uint32_t n, uint32_t flags, void* d_hits, void* d_blocked);
#define CLW_TIMING_CAST 0x43415354u

/* Layered ray queries: not the first thing a ray meets but the K nearest, in depth order -- select the object behind the one just selected,
 * list what lies under the cursor, count the surfaces between two points, measure how far behind a glass sphere the floor is -- in ONE launch
 * and one scan of the scene, where peeling with `ignore` costs K of each and loses or doubles the second of two primitives at the same t.
 * clw_host_cast_layers is THE definition; the device pass (wt_cast_layers: csrc/whitted_layers.inc) equals it bit for bit in both builds.
 * Rays, flags (CLW_CAST_*), the kinds that take part, `ignore`, CLW_CAST_OPAQUE, the sphere and plane tests and the rule `candidate iff hit &&
 * t <= tmax` are exactly those of clw_host_cast_rays above.  On top of them:
 *   - A candidate is LISTED iff additionally t < +inf.  {+inf, CLW_ID_NONE} is the empty entry, so a candidate at infinity cannot be told from
 *     none.
 *   - The listed candidates of a ray are ordered by (t ascending, id word ascending as uint32).  The id word is kind << 30 | index, so its
 *     order is the scan order spheres, planes, lights: equal t keeps the earlier primitive first, as the nearest query does.  A primitive
 *     appears at most once.  A sphere is listed at the one t its test returns -- its near side, or its far side for a ray that starts
 *     inside.
 *   - Output is planar, layer-major: entry k of ray i is t[k * n + i], id[k * n + i], k = 0 .. K-1; entries past the number of listed
 *     candidates hold {+inf, CLW_ID_NONE}.  A caller who needs to know whether there is more asks for K + 1.
 *   - Refused (0 returned, nothing written): whatever clw_host_cast_rays refuses; K == 0 or K > 8; a NULL t or id.
 * So layer 0 is {t, id} of clw_host_cast_rays for every ray whose nearest t is finite, and the layers for K are a prefix of those for K + 1.
 * clw_host_camera_rays: the records of clw_host_projection_rays for the global ids [id_begin, id_end) of the camera's frame, repacked as query
 * rays {origin, tmax = +inf, dir, ignore = CLW_ID_NONE} -- all three models, the pinhole included (its direction is the raygen's, normalised);
 * it refuses what clw_host_projection_rays refuses.  The device kernel (wt_camera_rays) equals it bit for bit. */
typedef struct clw_layer { float t; uint32_t id; } clw_layer;   /* 8 bytes */
int clw_host_cast_layers(const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t K, const void* spheres, uint32_t ns, const void* planes,
                         uint32_t np, const void* lights, uint32_t nl, float* t /* K * n */, uint32_t* id /* K * n */);   /* 1 = done, 0 = refused */
int clw_host_camera_rays(const struct clw_camera* cam, const clw_projection* proj, uint64_t id_begin, uint64_t id_end, clw_ray* out);
/* On the device, against the wrapper's bound scene, with the semantics of the three clw_ext_cast_* calls: the scene is prepared if needed and
 * read staged in LDS, from global memory or through the uniform grid (which only skips tests); the caller's stream is used after
 * clw_ext_set_stream; 0 is returned and nothing launched for what the definition refuses and when no scene is bound; the buffers of the
 * host-array calls are allocated at first use, grown at need and freed by cl_wrap_release.
 * clw_ext_cast_layers takes HOST arrays (n rays; K * n floats; K * n words), waits and returns n.  clw_ext_cast_layers_device takes the caller's
 * DEVICE memory of the same sizes, does not wait and returns n.
 * clw_ext_camera_rays / clw_ext_camera_rays_device write the query rays of the range the next trace launch would cover -- the latched camera
 * under the projection set, work-item i being global id id_offset + i, as clw_ext_render_gbuffer -- into a host array (waits) or the caller's
 * device memory (no wait) of `capacity` records, and return the work-items n.  They need no scene.  0 -- nothing launched -- without a latched
 * camera, with row bands, with a projection that cannot be resolved, and when capacity < n.
 * clw_ext_render_layers: the camera rays, then their K layers, into buffers the feature owns (sized for the range and K) -> work-items, 0 when
 * either half refuses.  clw_ext_read_layers copies what the last render_layers left -- what = 0: K * n floats, 1: K * n id words, layer-major
 * -- and returns the byte count (out = NULL or too small a capacity: the count only); clw_ext_layers_device_ptr is the device address, NULL
 * before the first pass.
 * clw_ext_pick_layers: the same two kernels on the one-pixel range of frame pixel (x, y), one small read-back: out[k] = layer k, k < K -- the
 * pixel's column of clw_ext_render_layers, bit for bit.  1, or 0 as clw_ext_pick (no latched camera, a pixel that is not one of the wrapper's
 * work-items, out = NULL), for refused flags or K, and with row bands.  Neither it nor clw_ext_render_layers restarts an accumulating view.
 * All of these leave alone the framebuffer, the buffers of clw_ext_render_gbuffer, the overlay, the object table, the AO pass and the ray
 * queries, an accumulating view and its count, the tile order and clw_ext_last_trace_flags.  Launches are logged under CLW_TIMING_LAYERS and
 * CLW_TIMING_CAMRAYS in clw_ext_timing_get (a pick's are not, as clw_ext_pick's).
 * Not built: the far side of a sphere as a layer of its own (exits); K > 8; a through-selection in the marquee and an X-ray outline in the
 * overlay (consumers of the planar id layers on the device); a total candidate count -- the grid walk meets a sphere once per cell it is listed
 * in and only the list tells repeats apart. */
uint32_t clw_ext_cast_layers(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t K, float* t, uint32_t* id);     /* host arrays; waits */
uint32_t clw_ext_cast_layers_device(cl_wrap* wrap, const void* d_rays, uint32_t n, uint32_t flags, uint32_t K, void* d_t, void* d_id);   /* no wait */
uint32_t clw_ext_camera_rays(cl_wrap* wrap, clw_ray* out, uint32_t capacity);              /* host array; waits */
uint32_t clw_ext_camera_rays_device(cl_wrap* wrap, void* d_rays, uint32_t capacity);       /* no wait */
uint32_t clw_ext_render_layers(cl_wrap* wrap, uint32_t flags, uint32_t K);
uint32_t clw_ext_read_layers(cl_wrap* wrap, uint32_t what /* 0 = t, 1 = id */, void* out, uint32_t capacity_bytes);
void*    clw_ext_layers_device_ptr(cl_wrap* wrap, uint32_t what);
int      clw_ext_pick_layers(cl_wrap* wrap, uint32_t x, uint32_t y, uint32_t flags, uint32_t K, clw_layer* out /* K */);
#define CLW_TIMING_LAYERS  0x4C415952u
#define CLW_TIMING_CAMRAYS 0x43524159u

/* Path queries: where a ray GOES -- what shows in a mirror, what a glass sphere refracts into view, where a beam ends after four bounces -- in
 * ONE launch, where hits read back, a bounce step and another cast cost a launch per bounce and a caller's own copy of the reference's
 * refraction rule.  clw_host_cast_paths is THE definition; the device pass (wt_cast_paths: csrc/whitted_paths.inc) equals it bit for bit in both
 * builds.  The arithmetic regime is the ray queries': float32, one rounding per operation, never fused, IEEE square root and divide, dot products
 * left to right.  Rays, the kinds that take part, `ignore`, CLW_CAST_OPAQUE and the tests are those of clw_host_cast_rays above.
 * Per ray, a path of up to B = `bounces` (1..8) segments; the path's refractive index n1 starts at 1 (the reference's DEFAULT_N).  Segment k:
 *   - THE HIT of segment k is exactly what clw_host_cast_rays answers for the segment's ray {origin, tmax, dir, ignore}: segment 0 is the
 *     caller's ray as given (its direction NOT normalised, its own `ignore`); every later segment has the path's outgoing ray, the caller's
 *     tmax and ignore = CLW_ID_NONE.  tmax bounds every segment on its own.
 *   - A miss ends the path (reason 1); it is not recorded.  A hit is recorded: count = k + 1.
 *   - A light that is hit (kind 2) ends the path (reason 2).
 *   - The winner's material is read from its 96-byte record: the words transperent, dielectric (u32), n, reflectivity (f32) at byte 64.  Unless
 *     CLW_PATH_ALL_SURFACES is set, a surface with reflectivity == 0 && !dielectric && !transperent ends the path (reason 2): the reference sends
 *     nothing on from it.
 *   - The outgoing ray is the reference's (raytracing.cl:139-179), operation for operation, with N = the hit's normal, D = the segment's
 *     direction and P = point + N * EPSILON per component (EPSILON = 0.001f; the product, then the sum -- the point shading uses):
 *       reflect(D, N) = D + N * (2 * c), c = -(N.D) -- every path continues so unless it is transmitted: origin = P, dir = reflect(D, N).
 *       With CLW_PATH_TRANSMIT and transperent != 0: n2 = (n1 == 1) ? material n : 1; if n1 < n2 the origin is P - N * (2 * EPSILON) (inside
 *       the surface), otherwise N is negated and the origin stays P; with e = n1 / n2, c = -(N.D), s = e * e * (1 - c * c): s > 1 gives a NaN
 *       direction, else dir = D * e + N * (e * c - sqrtf(1 - s)); the path's n1 becomes n2.  A direction whose x is NaN (total internal
 *       reflection) falls back to the reflected ray from P with n1 unchanged: that is where the reference's light goes.
 *     refract assumes a UNIT direction, as in the reference; nothing here normalises one.
 *   - After segment B - 1 the path ends with reason 0.
 * Output: hits[k * n + i] = the hit of segment k of ray i (layer-major as the layered query); entries from `count` on hold the miss record of
 * clw_host_cast_rays {+inf, CLW_ID_NONE, 0, 0}.  status[i] = count | reason << 4 (CLW_PATH_COUNT / CLW_PATH_REASON).  next (optional, n
 * records): after reason 0 the outgoing ray of the last hit, after reason 1 the ray that missed (its `ignore` included) -- a caller can look the
 * sky up --, after reason 2 {P of the last hit, tmax, dir = 0, CLW_ID_NONE}: a zero direction meets nothing.
 * Refused (0 returned, nothing written): whatever clw_host_cast_rays refuses for flags & (CLW_CAST_KINDS | CLW_CAST_OPAQUE); a flag bit beside
 * those and the two below; bounces == 0 or > 8; a NULL hits or status. */
#define CLW_PATH_TRANSMIT     16u   /* a transparent surface is passed through (refracted), not reflected off */
#define CLW_PATH_ALL_SURFACES 32u   /* a diffuse surface reflects the path on instead of ending it */
#define CLW_PATH_MAX_BOUNCES  8u
#define CLW_PATH_REASON_BOUNCES 0u  /* `bounces` segments recorded */
#define CLW_PATH_REASON_MISSED  1u  /* the last segment met nothing */
#define CLW_PATH_REASON_ENDED   2u  /* the last hit was a light, or a surface that sends nothing on */
#define CLW_PATH_COUNT(status)  ((status) & 15u)
#define CLW_PATH_REASON(status) ((status) >> 4)
int clw_host_cast_paths(const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t bounces, const void* spheres, uint32_t ns, const void* planes,
                        uint32_t np, const void* lights, uint32_t nl, clw_hit* hits /* bounces * n */, uint8_t* status /* n */,
                        clw_ray* next /* n, or NULL */);   /* 1 = done, 0 = refused */
/* On the device, against the wrapper's bound scene, with the conventions of the clw_ext_cast_layers* calls: the scene is prepared if needed and
 * read staged in LDS, from global memory or through the uniform grid as wt_plan_cast decides for the ray queries; the materials are read from
 * the bound sphere and plane arrays themselves; 0 is returned and nothing launched for what the definition refuses and when no scene is bound.
 * clw_ext_cast_paths takes HOST arrays (n rays; bounces * n hits; n bytes; n rays or NULL), waits and returns n; its staging buffers are
 * allocated at first use, grown at need and freed by cl_wrap_release.  clw_ext_cast_paths_device takes the caller's DEVICE memory of the same
 * sizes (d_next may be NULL), launches on the wrapper's stream -- the caller's after clw_ext_set_stream --, does not wait and returns n.
 * clw_ext_pick_path: the camera-ray kernel on the one-pixel range of frame pixel (x, y) under the wrapper's camera model, then the path of that
 * ray; out_hits[k], k < bounces, and *out_status as above.  1, or 0 as clw_ext_pick_layers (no latched camera, a pixel that is not one of the
 * wrapper's work-items, row bands, a NULL output, refused flags or bounces, no scene bound).  It does not restart an accumulating view.
 * All three leave alone the framebuffer, the buffers of clw_ext_render_gbuffer, the overlay, the object table, the AO pass, the ray queries and
 * the layers, an accumulating view and its count, the tile order and clw_ext_last_trace_flags.  Launches are logged under CLW_TIMING_PATHS in
 * clw_ext_timing_get (a pick's are not).
 * Not built: per-ray flags; a bound on the total path length instead of the per-segment tmax; Schlick-weighted branching (a path follows one
 * ray, the reference's trace follows both at a dielectric). */
uint32_t clw_ext_cast_paths(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t bounces, clw_hit* hits, uint8_t* status,
                            clw_ray* next);   /* host arrays; waits */
uint32_t clw_ext_cast_paths_device(cl_wrap* wrap, const void* d_rays, uint32_t n, uint32_t flags, uint32_t bounces, void* d_hits, void* d_status,
                                   void* d_next);   /* no wait */
int      clw_ext_pick_path(cl_wrap* wrap, uint32_t x, uint32_t y, uint32_t bounces, uint32_t flags, clw_hit* out_hits /* bounces */,
                           uint8_t* out_status);
#define CLW_TIMING_PATHS 0x50415448u

/* ---- proximity queries: what lies around a point -- the nearest surface, whether anything is within reach, the K nearest surfaces.  The
 * questions that have no direction: how far is this point from the nearest object and which one is it, does a ball of radius R placed here
 * touch anything, which spheres touch each other.  clw_host_nearest_surface, clw_host_within_reach and clw_host_near_surfaces are THE
 * definition; the device pass (wt_near: csrc/whitted_near.inc) equals them bit for bit in both builds.  The regime is the ray queries': float32,
 * one rounding per operation, never fused, IEEE square root and divide, dot products left to right, the scene read through the prepared words
 * {c, +-r * r}, {n}, {p0} the device reads.  flags are CLW_CAST_SPHERES | PLANES | LIGHTS | OPAQUE with their meaning above; the primitives take
 * part in the same order (spheres, planes, lights, ascending index); a primitive whose id word equals ignore[k] is skipped (`ignore` NULL, or
 * the word CLW_ID_NONE: nothing is); with CLW_CAST_OPAQUE a sphere whose prepared word has its sign bit set is skipped.
 *   Probe k = {p, reach} against
 *   - a sphere or light {c, q}: v = p - c, m = sqrtf(v.v), r = sqrtf(|q|), d = m - r -- signed, negative inside.  Normal N = v / m per
 *     component, nearest point c + N * r per component (the product, then the sum).  At the centre m = 0: N and the point are the NaNs this
 *     computes and d = -r; they are stored as computed.
 *   - a plane {n, p0}: s = (p - p0).n, d = fabsf(s) -- the two-sided sheet the tracer shades.  Nearest point p - n * s per component (the
 *     product, then the difference); normal = the stored n, never flipped and taken for unit.
 *   CANDIDATE iff d <= reach.  So a NaN point or a NaN reach meets nothing, reach = +inf is unlimited, and a negative reach is legal: only
 *   penetrations at least that deep.
 *   - nearest: the smallest key (d, id word) -- a candidate replaces the best iff d < best, so an equal d keeps the earlier primitive -- as a
 *     clw_hit {t = d, id, normal, point}.  No candidate: the miss record of clw_host_cast_rays.  A candidate at d = +inf raises `within` but
 *     keeps the miss record.
 *   - within: within[k] = 1 iff probe k has a candidate, else 0.
 *   - K nearest (1..8): exactly the list rules of clw_host_cast_layers with d for t -- listed iff d < +inf, ordered by (d, id), every
 *     primitive at most once, planar and layer-major d[k * n + i], id[k * n + i], empty entries {+inf, CLW_ID_NONE}.  K is a prefix of K + 1,
 *     and layer 0 is {d, id} of the nearest query wherever that is finite.
 *   Refused (0 returned, nothing written): whatever clw_host_cast_rays refuses for n, flags and NULL arrays; K == 0 or K > 8; a NULL output. */
typedef struct clw_probe { float point[3]; float reach; } clw_probe;   /* 16 bytes */
int clw_host_nearest_surface(const clw_probe* probes, const uint32_t* ignore /* n words, or NULL */, uint32_t n, uint32_t flags,
                             const void* spheres, uint32_t ns, const void* planes, uint32_t np, const void* lights, uint32_t nl,
                             clw_hit* out);                     /* 1 = done, 0 = refused */
int clw_host_within_reach(const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns,
                          const void* planes, uint32_t np, const void* lights, uint32_t nl, uint8_t* within);      /* 0 / 1 per probe */
int clw_host_near_surfaces(const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, const void* spheres, uint32_t ns,
                           const void* planes, uint32_t np, const void* lights, uint32_t nl, uint32_t K, float* d /* K * n */,
                           uint32_t* id /* K * n */);
/* On the device, against the wrapper's bound scene, with the conventions of the clw_ext_cast_* calls: the scene is prepared if needed (a call
 * after clw_ext_invalidate_scene sees the rewritten scene) and read staged in LDS, from global memory or through the uniform grid as
 * wt_plan_near decides -- on the grid a probe tests the spheres listed in the cells of the box its reach spans (csrc/whitted_near.inc states
 * and proves the box); a probe whose box covers more than a cap of cells (CLWRAP_NEAR_BOX_CELLS in the environment overrides the built-in
 * cap) or whose reach is not finite scans every sphere.  Same answer either way.
 * clw_ext_nearest_surface / clw_ext_within_reach / clw_ext_near_surfaces take HOST arrays (n probes; n ignore words or NULL), wait and return
 * n; their staging buffers are allocated at first use, grown at need and freed by cl_wrap_release.  clw_ext_probe_device and
 * clw_ext_near_surfaces_device take the caller's DEVICE memory of the same sizes (d_ignore may be NULL; exactly one of d_hits / d_within is
 * non-NULL), launch on the wrapper's stream -- the caller's after clw_ext_set_stream --, do not wait and return n.
 * 0 is returned and nothing launched for what the definition refuses, when no scene is bound and, for clw_ext_probe_device, when both or
 * neither output is given.  The framebuffer, the buffers of clw_ext_render_gbuffer, the overlay, the object table, the AO pass, the ray,
 * layered and path queries, an accumulating view and its count, the tile order and clw_ext_last_trace_flags are left alone.  Launches are
 * logged under CLW_TIMING_NEAR in clw_ext_timing_get.
 * Not built: swept balls; an expanding search for an unlimited reach on the grid (such a probe scans every sphere); per-probe flags; a
 * clearance view over the primary-hit point channel. */
uint32_t clw_ext_nearest_surface(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, clw_hit* out);     /* host arrays; waits */
uint32_t clw_ext_within_reach(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, uint8_t* within);    /* host arrays; waits */
uint32_t clw_ext_near_surfaces(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, uint32_t K, float* d,
                               uint32_t* id);     /* host arrays; waits */
uint32_t clw_ext_probe_device(cl_wrap* wrap, const void* d_probes, const void* d_ignore, uint32_t n, uint32_t flags, void* d_hits,
                              void* d_within);   /* exactly one output; no wait */
uint32_t clw_ext_near_surfaces_device(cl_wrap* wrap, const void* d_probes, const void* d_ignore, uint32_t n, uint32_t flags, uint32_t K, void* d_d,
                                      void* d_id);   /* no wait */
#define CLW_TIMING_NEAR 0x4E454152u

/* Work counters of the trace kernel.  enable=1 selects the counting build of the kernel
 * for subsequent launches (slower); read returns and clears
 *   out[0] path segments  out[1] shadow rays  out[2] light probes  out[3] skybox fetches
 *   out[4] texel fetches  out[5] refraction pushes  out[6] lane-iterations  out[7] wave-iterations*64
 * (rays = out[0] + out[1]; out[6]/out[7] = SIMD lane utilisation). */
void clw_ext_enable_counters(cl_wrap* wrap, int enable);
void clw_ext_read_counters(cl_wrap* wrap, uint64_t out[8]);
/* The same with the later words: out[8] = shadow rays really TRACED.  out[1] counts every shadow ray the reference
 * would cast; those of a surface whose specular and diffuse coefficients are both zero (glass)
 * contribute exactly +0, so the kernel draws their random numbers but does not trace them -- out[8] leaves them
 * out.  n <= 32 words are returned (the rest reads 0), and the device block is cleared.  Words 16.. are
 * only written by the diagnostic stamp build of the kernel (tools/stamp_phases.py). */
void clw_ext_read_counters_ex(cl_wrap* wrap, uint64_t* out, uint32_t n);

/* The factor a transparent sphere applies to a shadow ray that passes through it: 0.8f by default, the reference's
 * TRANSPERENT_THROUGH (primitives.cl:7, :419).  A knob because the reference's only committed output, out/scene.png, was rendered by
 * a version of its kernels without that attenuation: with 1.0 the unchanged raypng.c driver reproduces that image (tests/
 * test_gpu_reference_fixture.py); also CLWRAP_THROUGH=<float> in the environment of cl_wrap_init. */
void clw_ext_set_shadow_through(cl_wrap* wrap, float factor);

/* Uniform grid over the spheres (default on; built for scenes with more than 256 spheres): rays test only the
 * spheres registered in the cells they cross instead of all of them.  Same arithmetic per test, same nearest
 * hit and same shadow factor as the reference's linear scan; 0 forces the linear scan. */
void clw_ext_set_grid(cl_wrap* wrap, int on);
/* The grid of the scene as last prepared (the first trace, G-buffer or unit-scene launch after the scene changed prepares it).  `built` 0: the
 * scene has no grid -- at most 256 spheres, a sphere that is not finite, or more cell-list entries than the shim allows -- and runs the linear
 * scan; every other field is then 0.  `pair` 1: the two soft-shadow samples of a light share one walk along the ray to its centre
 * (wt_grid_shadow_pair) and every sphere is listed `reg_pad` beyond its box; 0: every shadow ray walks on its own (wt_grid_shadow), which is
 * also what the tree-parallel tail always does.  The shim pairs when the largest light radius is at most 0.3 of the smallest cell side and
 * the padded lists fit.  res / cell / gmin: cells per axis, their sides, the low corner of the bounds; ncells = res[0] * res[1] * res[2];
 * pairs = (cell, sphere) entries = start[ncells].  Returns 1, or 0 (and writes nothing) while no scene is prepared.  For tests. */
typedef struct {
    int32_t built, pair;
    int32_t res[3];
    uint32_t ncells;
    uint64_t pairs;
    float cell[3], gmin[3], reg_pad;
} clw_grid_info;
int clw_ext_get_grid(const cl_wrap* wrap, clw_grid_info* out);
/* Which shadow walk a grid scene takes: -1 the default (pairing unless env CLWRAP_GRID_PAIR=0), 0 never pair, 1 pair wherever the rule above
 * allows it, whatever the environment says (clw_ext_get_grid reports what came of it).  Same image either way.  Takes effect at the next scene
 * preparation and forces one, as a changed scene does.  Errors (print + exit(1)): a value outside [-1, 1]. */
void clw_ext_set_grid_pair(cl_wrap* wrap, int on);

/* Cost-sorted tile dispatch (default on): every 8x8 tile reports its cost, and the next frame serves each
 * XCD's tiles heaviest-first, so the expensive refraction tiles no longer end up in the tail of the launch.
 * Pure scheduling: the image is bit-identical either way. */
void clw_ext_set_tile_sched(cl_wrap* wrap, int on);

/* The per-tile cost table of the last tiled launch (row-major 8x8 tiles; cost = loop iterations of the tile's most expensive
 * pixel, +3 per shaded hit; for scenes on the uniform grid: the lifetime of the tile's wavefront in units of 256 cycles).  Returns the number of tiles; copies them if `capacity` suffices. */
uint32_t clw_ext_read_tile_costs(cl_wrap* wrap, uint32_t* out, uint32_t capacity);

/* Runs ONE device helper of the trace kernel over `n` input rows (host arrays; rows of `stride_in` / `stride_out`
 * floats) in the current arithmetic mode -- function-level parity tests against the reference's own functions.
 * op: 0 intersect_sphere {o,d,c,r -> hit,t}  1 intersect_plane {o,d,n,p0 -> hit,t}  2 reflect {i,n -> r}
 *     3 refract {n1,n2,i,n -> ok,r}  4 compute_schlick {n1,n2,i,n -> f}  5 map_to_cube {dir -> u,v bits; aux = face}
 *     6 xorshift32 {state bits -> state bits, value}  7 euclidean_modulo {a,b bits -> m bits}
 *     8 sin/cos of the sampling angle {u -> s,c of fl32(2 pi u) (aux 1) or fl32(pi u) (aux 0)}  9 pow {x,y -> x^y}  10 normalize {v -> unit, length}. */
void clw_ext_unit(cl_wrap* wrap, int op, const float* in, uint32_t stride_in, float* out, uint32_t stride_out,
                  uint32_t n, uint32_t aux);

/* Runs the dispatch-order builder (wt_sched_build, csrc/whitted_trace.inc) ONCE on a caller's cost table -- `cost` = trows x tpr words, row-major
 * 8x8 tiles, as clw_ext_read_tile_costs returns them -- with exactly the arguments the shim gives it, per_share = ceil(trows / 8) * tpr:
 *   clamp_outliers 0 / 1 (1 = the scale of the 256 bins stops at 16x the share's mean: grid builds), per_share_cap >= per_share = entries per
 *   XCD share, split_slots (0 = no tile is split), min_quota, max_lg in 0..4 (a tile is served by at most 2^max_lg wavefronts).
 * The order is order[8 * pos + k] = entry `pos` of share k (the tiles of tile rows = k mod 8), heaviest first; an entry is
 *   tile column | tile row << 12 | lg << 24 | part << 27, or 0xFFFFFFFF = none.
 * The device buffer is allocated for the worst case, 8 * (per_share << max_lg) + 8 * per_share_cap words, pre-filled with CLW_SCHED_SENTINEL
 * (neither an entry nor 0xFFFFFFFF) and returned WHOLE: a builder that writes beyond its 8 * per_share_cap words shows as overwritten sentinels,
 * never as an access outside an allocation.  Returns that number of words; copies them if `out_words` suffices (else nothing is launched).
 * Errors (print + exit(1)): an empty table, more than 4095 tiles either way, max_lg > 4, per_share_cap < per_share.  For tests. */
#define CLW_SCHED_SENTINEL 0xA5A5A5A5u
uint32_t clw_ext_unit_sched(cl_wrap* wrap, const uint32_t* cost, uint32_t tpr, uint32_t trows, int clamp_outliers, uint32_t per_share_cap,
                            uint32_t split_slots, uint32_t min_quota, uint32_t max_lg, uint32_t* out, uint32_t out_words);
/* The order buffer the LAST tiled launch of a whole range (not a strip of the pipelined read-back) actually read, 8 * per_share_cap words laid
 * out as above -> their count, and per_share_cap through the pointer (may be NULL); 0 = that launch ran in the default order (no order built
 * yet, tile order off, variant 4) or there was none.  Copies the words if `capacity` suffices.  Waits for the launch and for a build behind it.
 * The shim remembers WHICH of its two buffers the launch read; a launch that also rebuilds (its camera, depth or scene changed) may have that
 * buffer rewritten behind it, so pair the call with a still view: the order is then the one built from the first frame's costs.  For tests. */
uint32_t clw_ext_read_tile_order(cl_wrap* wrap, uint32_t* out, uint32_t capacity, uint32_t* per_share_cap);
/* How heavy tiles of deep launches are split: the quota of a share is its total cost over `slots` wavefronts (default 512, at least 1; env
 * CLWRAP_SPLIT_SLOTS), and at least `min_quota` (default 1500; 0 = no tile is split; env CLWRAP_SPLIT_MIN_QUOTA).  A negative argument keeps the
 * current value.  Same image whatever the settings.  The orders built so far are dropped, as by clw_ext_set_tile_sched: the next launch runs in
 * the default order and the one after it in an order built with the new values. */
void clw_ext_set_split(cl_wrap* wrap, int slots, int min_quota);
/* The values in effect, and how many entries a share's list has beyond its tiles in a launch that may split (any pointer may be NULL). */
void clw_ext_get_split(const cl_wrap* wrap, uint32_t* slots, uint32_t* min_quota, uint32_t* extra_per_share);

/* The same for the helpers that need the SCENE: runs on the scene bound to raytracer kernel `kernel_id` (its args 1-6,
 * 8, 9), through the code the trace kernel itself runs (its hit phase and its batched shadow traversal).
 * op: 0 hit phase {o,d -> lit, light rgb[3], solid hit, point[3], normal[3], material rgb[3], ambient, diffuse, specular,
 *       shininess, transparent, dielectric, n, reflectivity}  (findLightIntersection + findSolidIntersection,
 *       reference primitives.cl:262-318, 322-394; 22 floats out)
 *     1 testShadowPath {to, from -> factor}  (primitives.cl:396-442)
 *     2 plane_texture_pixel {b0[3], scale, b1[3], texture id bits, p[3] -> rgb}  (primitives.cl:217-259; the first eight
 *       floats are the plane's prepared basis row; stride_in must be a multiple of 4). */
void clw_ext_unit_scene(cl_wrap* wrap, cl_uint kernel_id, int op, const float* in, uint32_t stride_in, float* out,
                        uint32_t stride_out, uint32_t n);

/* Kernel build variant for A/B measurements and equivalence tests (same image in every variant); 0 = default.  Bits:
 * 1 geometry from global memory instead of LDS, 2 linear work-item ids instead of 8x8 tiles, 4 no cost-sorted tile
 * order, 8 no uniform grid, 16 no tree-parallel tail (deep launches run their per-lane loop to the end), 64 never the high-occupancy flavour of the deep build,
 * 128 no light / plane side table (every shadow ray tests every plane), 256 no visibility classes (every needed shadow ray is traced),
 * 4096 heavy tiles of deep launches are not split over several wavefronts,
 * 8192 small scenes of the shallow fast build run the generic trace kernel instead of the one with the scene's counts compiled in,
 * 16384 the trace loop runs the Fresnel / reflection block on a path's last level too, where nothing reads its results, and the tile cost is
 * reduced over the wave by the shuffle butterfly instead of DPP row operations (the kernel as it was before both were trimmed),
 * 32768 no primary-ray cull table: the first loop iteration of every tile tests every sphere and every light (clw_host_primary_cull below),
 * 2048 deep launches always carry the full-depth (31-parent) scratch stack instead of one sized for their depth,
 * 1024 (with clw_ext_enable_counters) VERIFICATION of the visibility classes: lights are classified AND traced, counter word 9 =
 * lights classified, word 28 = lights whose traced factors differ from their class's (must read 0),
 * 512 DIAGNOSTIC builds only (-DWT_TIMELINE=1, tools/timeline.py): the tile-cost buffer receives when each tile's wave ran inside the launch
 * (CLWRAP_TIMELINE_SHIFT = tick of 10 ns << shift; CLWRAP_TIMELINE_EDGES = 1 / 2: its prologue and epilogue instead); no effect otherwise. */
void clw_ext_set_variant(cl_wrap* wrap, int variant);
/* The kernel flavour of the latest trace launch: its WT_F_* flags (csrc/whitted_params.h; bit 256 = the scene's counts compiled in,
 * ns | np << 3 | nl << 5 in bits 9..16), -1 before the first launch.  For tests and A/B runs. */
int clw_ext_last_trace_flags(cl_wrap* wrap);

/* The primary-ray cull table.  The first loop iteration of a tile's wavefront traces 64 rays of the pinhole camera from one origin; where no
 * ray of the tile can pass the line test of a sphere (the discriminant D >= 0 of intersect_sphere, primitives.cl:170-195), the test is the same
 * failure in every lane and skipping it changes no bit of the image.  The table holds one byte per 8x8 tile of a launch's rows:
 *   bit 0  no primary ray of the tile has D >= 0 for ANY scene sphere       bit 1  the same for every light sphere
 * and the trace kernel skips the nearest-hit sphere loop / the light probe of a tile's first iteration when the bit is set.
 * clw_host_primary_cull is THE definition (csrc/primary_cull_host.h states the rule and justifies its margin): the tile's directions are bounded
 * by a cone -- the axis through the tile centre, the half-angle the largest angle to its four corner pixels -- and a sphere is clear of the tile
 * when the angle between the axis and the LINE through the origin and the sphere's centre (a sphere behind the camera fails the line test too)
 * exceeds half-angle + asin(r / distance) by 3e-3 rad, both sines first enlarged by 1e-3.  Conservative: a set bit implies D < 0 for every
 * pixel of the tile as the kernel computes it in float32, never the converse.  No bit of a group is set when the origin lies inside or on one
 * of its spheres; none at all when a camera term is not finite.  An empty group has its bit set.
 *   cam: the raygen arguments (its width is the frame's; its height is not read); the launch covers `rows` rows from global row `row_offset`, or
 *   -- band_stride > 1 -- the interleaved 8-row bands of clw_ext_set_row_bands (local row y = global row ((y / 8) band_stride + band_phase) 8 + y % 8);
 *   spheres / lights: the 96-byte rsphere and 48-byte rlight arrays of the raytracer's arguments 1 and 3.
 * Writes ceil(rows / 8) * ceil(width / 8) bytes, row-major tiles, and returns that count; 0 = refused (a NULL pointer, no tiles, band_phase >=
 * band_stride), nothing written.
 * On the device the shim builds the same table (wt_primary_cull_build, the same arithmetic compiled for the device: bit for bit this one) on the
 * launch stream ahead of a trace, only when the camera, the frame width, the row range or the scene changed since it was built, and then for
 * the SECOND launch in a row of the new view: a still view builds once, behind its first frame (which tests everything), a camera that moves
 * every frame never builds and never reads a table (the builder's launch costs a frame more than the table saves it).  Only shallow
 * (depth <= 4), tiled, fused 1-sample launches of the pinhole camera over a scene without a uniform grid read a table; a launch from a ray
 * buffer (a projection's included), sample cameras (lens, shutter), moving spheres, every supersampled, adaptive-refine or deep launch and
 * variant 32768 run with none.
 * clw_ext_read_primary_cull: the table the LAST whole-range trace launch was given -> its tile count, the bytes copied if `capacity` suffices;
 * 0 = that launch had no table (or there was none).  `builds` (may be NULL) receives how often the builder has run for whole-range launches.
 * Waits for the launch.  For tests and A/B runs. */
struct clw_camera;      /* (below) */
uint32_t clw_host_primary_cull(const struct clw_camera* cam, uint32_t row_offset, uint32_t rows, uint32_t band_stride, uint32_t band_phase, const void* spheres,
                               uint32_t ns, const void* lights, uint32_t nl, uint8_t* out);
uint32_t clw_ext_read_primary_cull(cl_wrap* wrap, uint8_t* out, uint32_t capacity, uint64_t* builds);

/* The bounce cull table: a second byte per tile, one segment further.  Where bit 0 of the primary byte is set and ONE plane is the first hit of
 * every primary ray of the tile (decided at the four corner pixels and the centre: between two planes "nearer" is linear in the unnormalised
 * direction; a tile in which two planes meet, a grazing view or a normal that is not unit to 1e-6 carries nothing), the shading points of the
 * tile lie in a ball around the four corner hits, and
 *   bits 0-3  bit k: no line through that ball and a light sphere (any light) passes the line test of a scene sphere i with i mod 4 = k -- the
 *             shadow batch of the tile's FIRST shade skips those spheres (an empty class has its bit set)
 *   bit 4     no ray of the tile's SECOND loop iteration passes the line test of any scene sphere     bit 5  the same for every light sphere
 *             -- the plane's material is not transparent and depth >= 2, so those rays are the primary rays' mirror images and leave a
 *             virtual pinhole, the camera origin mirrored in the plane: the primary table's cone rule from there, every radius enlarged by
 *             the kernel's offset of the hit point.
 * clw_host_bounce_cull is THE definition (csrc/bounce_cull_host.h states the rule and justifies its margins); the arguments are
 * clw_host_primary_cull's, with the 96-byte rplane array, the launch depth and `parts` (1 = bits 0-3, 2 = bits 4-5, 3 = both; other bits of the
 * byte are 0).  Conservative like the primary table: a set bit implies D < 0 in the kernel's float32 for every test it stands for.
 * The device builder writes both bytes of a tile (one 16-bit entry, which the trace kernel loads where it loaded the primary byte) under the
 * primary table's when-to-build rule; a change of the launch depth or of the parts also builds again.
 * clw_ext_read_bounce_cull: the bounce bytes of the table the LAST whole-range trace launch was given, as clw_ext_read_primary_cull reads the
 * primary ones.  clw_ext_set_bounce_cull: the parts that tables built from now on carry (default 3, or CLWRAP_BOUNCE_CULL); same image whatever
 * the parts; the next launch of a still view builds its table again.  For tests and A/B runs. */
uint32_t clw_host_bounce_cull(const struct clw_camera* cam, uint32_t row_offset, uint32_t rows, uint32_t band_stride, uint32_t band_phase, const void* spheres,
                              uint32_t ns, const void* planes, uint32_t np, const void* lights, uint32_t nl, uint32_t depth, uint32_t parts, uint8_t* out);
uint32_t clw_ext_read_bounce_cull(cl_wrap* wrap, uint8_t* out, uint32_t capacity);
void clw_ext_set_bounce_cull(cl_wrap* wrap, int parts);

/* The tree-parallel tail of deep launches (depth > 4; csrc/whitted_tpt.inc): once at most `max_lanes` lanes of a tile's wavefront are
 * alive and they hold at least `min_paths` pending paths (current segments + continuations on their stacks), the rest of the tile is
 * traced by the whole wavefront as one pool of segments kept in a slot of a device pool of `pool_mb` MiB (8 192 slots).
 * Same image whatever the settings (the per-lane loop and the tail do the same arithmetic and add in the same order); max_lanes 64 sends
 * everything through the tail, 0 switches it off; a negative argument keeps the current value.  Defaults 40 / 4 / 8192, or
 * CLWRAP_TPT_MAX / CLWRAP_TPT_MIN / CLWRAP_TPT_POOL_MB.  Counting build: counter words 29 / 30 / 31 = tiles the tail gave up on (slice
 * full: finished by the per-lane loop) / tiles it finished / nodes it traced. */
void clw_ext_set_tpt(cl_wrap* wrap, int max_lanes, int min_paths, int pool_mb);
/* The values in effect (any pointer may be NULL). */
void clw_ext_get_tpt(const cl_wrap* wrap, uint32_t* max_lanes, uint32_t* min_paths, uint32_t* pool_mb);

/* Host helper: camera -> the eight by-value raygen arguments, with the reference's exact
 * mixed float/double arithmetic (rinit_camera + rgen_perspective, src/cpu_ray.c:8-35, 42-106).
 * `look` need not be normalised.  Returns 0 for the cameras the reference rejects
 * (fov ~ 180, fov <= eps, look == +Y; cpu_ray.c:58-63), else 1. */
typedef struct clw_camera {
    float im_corner[3], origin[3], up[3], right[3];
    float w_factor, h_factor;
    uint32_t width, height;
} clw_camera;
int clw_host_perspective(const float origin[3], const float look[3], float fov, float focal,
                         uint32_t width, uint32_t height, clw_camera* out);

/* Host helper: THE definition of the lens table, n in {2, 4, 8}; returns 0 on bad arguments (n, aperture < 0 or not finite,
 * focus <= 0 or not finite, a camera whose image plane passes through its origin), else 1 and n * n entries in sy * n + sx order.
 *   image-plane centre (im_corner is relative to the origin)  c = im_corner + right (w_factor W / 2) - up (h_factor H / 2),
 *   focal = |c|, q = focal / focus                                      [double; q rounded to float]
 *   sample k = sy n + sx takes lens cell j = k with its 2 log2 n bits reversed, cell (j mod n, j div n); the cell's centre in
 *   [-1, 1]^2 goes to the unit disk by the concentric (Shirley-Chiu) map -> (lx, ly)          [double; lx, ly rounded to float]
 *   delta = right (aperture lx) + up (aperture ly);  origin_k = origin + delta;  im_corner_k = im_corner - delta q;  up, right unchanged
 *                                                                       [float32, one rounding per operation, no contraction]
 * Every camera sees a point of the plane at axial distance `focus` at the same virtual pixel position.  aperture 0 returns n * n
 * copies of the base camera, bit for bit. */
int clw_host_lens_cameras(const clw_camera* base, float aperture, float focus, uint32_t n, clw_sample_camera* out);
/* Host helper: an open shutter between two cameras (camera motion blur; set the result with clw_ext_set_sample_cameras).  Sample k
 * looks through the camera at time t = (j + 1/2) / n^2, j as above, each of the four vectors a + (b - a) t in float32 (a where
 * a == b).  Returns 0 when n is not 2, 4 or 8 or the two cameras differ in width, height, w_factor or h_factor. */
int clw_host_shutter_cameras(const clw_camera* open, const clw_camera* close, uint32_t n, clw_sample_camera* out);
/* Host helper: the default sample times of moving spheres, the ones clw_host_shutter_cameras uses: t[k] = (j + 1/2) / n^2, j = k with its
 * 2 log2 n bits reversed (exact in float32).  Returns 0 when n is not 2, 4 or 8, else 1 and n * n times in sy * n + sx order. */
int clw_host_sample_times(uint32_t n, float* out);
/* Host helper: THE definition of the moved scene S(t): copies the ns 96-byte rsphere records to `out` and replaces each centre (the
 * first three floats) by fmaf(t, disp[3 i + a], c[a]); every other byte -- radius, material, padding -- is copied as it is.  `out` may
 * be `rspheres` itself.  Returns 0 on a NULL argument (with ns > 0), else 1. */
int clw_host_spheres_at(const void* rspheres, uint32_t ns, const float* disp, float t, void* out);

/* Host helpers: THE definition of what makes frame f of an accumulated view its own (clw_ext_set_accumulate).
 *   clw_host_frame_seed(f) = f * 0x9E3779B1 mod 2^32: 0 for frame 0; the multiplier is odd, so the frames of a run get distinct offsets.
 *   clw_host_jitter_camera(base, f, n), n in {1, 2, 4, 8}: f = 0 copies `base` byte for byte; for f >= 1
 *     jx = radical inverse of f in base 2, less 1/2;  jy = radical inverse of f in base 3, less 1/2     [double, the digit loop; rounded to float]
 *     ax = (w_factor / n) jx;  ay = (h_factor / n) jy;  im_corner[i] = (im_corner[i] + right[i] ax) - up[i] ay
 *                                                                       [float32, one rounding per operation, no contraction]
 *   and everything else copied: an offset of at most half a sample cell either way, so the running mean is a box filter over the cell of a pixel
 *   (of a sub-sample when n > 1).  Returns 0 on a NULL pointer or an n that is not 1, 2, 4 or 8, else 1.  `out` may be `base`. */
uint32_t clw_host_frame_seed(uint32_t f);
int clw_host_jitter_camera(const clw_camera* base, uint32_t f, uint32_t n, clw_camera* out);

/* Host helper: THE definition of the refine mask of adaptive supersampling (steps 2 and 3 of clw_ext_set_adaptive): `xrgb` = width x rows packed
 * pixels (the top byte is ignored), n in {2, 4, 8}, threshold in [0, 256]; writes one byte (0 / 1) per block of b x b pixels, b = 8 / n, row-major,
 * ceil(rows / b) x ceil(width / b) of them.  Returns 0 on bad arguments (n, threshold, a NULL pointer, an empty frame), else 1. */
int clw_host_refine_mask(const uint32_t* xrgb, uint32_t width, uint32_t rows, uint32_t n, int threshold, uint8_t* out);

/* Host helpers: PNG files without libpng (reference png_dump, src/cpu_ray.c:108-165, and the
 * decode step of cl_wrap_load_images).  Return 0 on success. */
int clw_host_write_png(const char* path, const uint32_t* xrgb, uint32_t width, uint32_t height);
int clw_host_write_png_rgba(const char* path, const uint8_t* rgba, uint32_t width, uint32_t height);
int clw_host_read_png(const char* path, uint32_t* width, uint32_t* height, uint8_t** rgba_malloced);
void clw_host_free(void* p);

/* Library build info, e.g. "opencl_wrap_hip gfx950 fast+strict". */
const char* clw_ext_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HIP_WRAP_EXT_H */
