/*
 * launch_plan.h -- the decision half of a trace launch (launch_plan.c): everything hip_wrap.cpp decides before it touches the device,
 * as pure C99 over plain structs -- the launch range and tile grid, the virtual frame of a supersampled launch, the per-lane camera
 * and time tables, the tail's pool arithmetic, the split of heavy tiles, the flag word (which compiled kernel runs) and every refusal
 * with its message.  No HIP, no exit: hip_wrap.cpp turns a refusal into its "ERROR:" line and a plan into device work.
 *
 * The wt_* functions declared here are exported from the library as a TEST SEAM (tests/plan_common.py mirrors the two structs and
 * holds the mirror to wt_plan_sizes); they are not part of the public interface of include/hip_wrap_ext.h.
 */
#ifndef LAUNCH_PLAN_H
#define LAUNCH_PLAN_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/hip_wrap_ext.h"
#include "whitted_params.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bits of clw_ext_set_variant / CLWRAP_VARIANT (documented in hip_wrap_ext.h) */
enum { WT_V_GEOM_GLOBAL = 1, WT_V_LINEAR_IDS = 2, WT_V_NO_TILE_ORDER = 4, WT_V_NO_GRID = 8, WT_V_NO_TAIL = 16, WT_V_NO_OCC = 64,
       WT_V_NO_LPT = 128, WT_V_NO_VIS = 256, WT_V_TIMELINE = 512, WT_V_VIS_VERIFY = 1024, WT_V_FULL_STACK = 2048, WT_V_NO_SPLIT = 4096,
       WT_V_NO_SHAPE = 8192, WT_V_UNTRIMMED = 16384, WT_V_NO_CULL = 32768 };

/* limits and thresholds of the plan (the defaults of the knobs below are the measured optima) */
enum {
    WT_LAUNCH_ROUND = 256,          /* the reference's launch rounding unit: CL_KERNEL_WORK_GROUP_SIZE on AMD (opencl_wrap.c:359-374) */
    WT_GEOM_LDS_MAX_F4 = 1024,      /* <= 16 KiB of prepared geometry is staged in LDS */
    WT_SHALLOW_LEVELS = 3,          /* DFS levels the shallow builds provide (LDS + scratch): depth <= WT_SHALLOW_LEVELS + 1 */
    WT_GRID_MIN_SPHERES = 256,      /* scenes beyond the reference's one-byte counts get the uniform grid (at 64 spheres it only
                                       wins when the cells happen to align with the spheres: 9.2-15 ms vs 10.9 ms linear) */
    /* deep launches of at least OCC_TILES_PER_DEPTH x depth wavefronts take the high-occupancy flavour: the serial tail of
     * the deepest refraction trees grows with the depth, the throughput part with the tile count (tools/occ_sweep.py on
     * render.map: wins 12-14 % at 2560x1440 depth 6 and 3840x2160 depth 6-8, loses 2-5 % at 1920x1080 and at depth 15) */
    WT_OCC_TILES_PER_DEPTH = 9000,
    /* tree-parallel tail (whitted_tpt.inc): a deep launch enters it with at most TPT_MAX_LANES live lanes holding at least TPT_MIN_PATHS
     * pending paths; the pool holds TPT_SLOTS_PER_XCC slots per XCD (more than an XCD's CUs hold wavefronts) of at most TPT_SLICE_WORDS_MAX
     * words, TPT_POOL_MB in all (below TPT_MIN_CAP nodes per slot -- hundreds of lights -- the launch runs without the tail) */
    WT_TPT_MAX_LANES = 40, WT_TPT_MIN_PATHS = 4, WT_TPT_POOL_MB = 8192, WT_TPT_MIN_CAP = 160, WT_TPT_SLOTS_PER_XCC = 1024,
    WT_TPT_SLICE_WORDS_MAX = 1 << 18,
    /* heavy tiles of such a launch are served by up to 16 wavefronts each (wt_sched_build): up to SPLIT_EXTRA_PER_SHARE more dispatch entries
     * per XCD share; a tile is split while its parts stay above SPLIT_MIN_QUOTA cost units (a part enters the tail at once and pays its
     * fixed costs: 800x600 depth 15 0.267 ms at 3 000, 0.208 at 750-1 500); the quota is the share's total cost over SPLIT_SLOTS wavefronts (384 / 512 / 640: 1920x1080 depth 15 0.370 / 0.332 / 0.322 ms, glass field 2048^2 depth 8 3.19 / 2.95 / 3.33) */
    WT_SPLIT_EXTRA_PER_SHARE = 1024, WT_SPLIT_MIN_QUOTA = 1500, WT_SPLIT_SLOTS = 512,
    WT_TILE_LIST_MAX = 0xFFF        /* a tile order / tile list packs (tile column | row << 12 | parts): 4095 tiles each way */
};

/* snapshot of the eight by-value raygen arguments + the launch range: what a ray buffer "holds" after a fused raygen launch */
typedef struct {
    float corner[3], origin[3], up[3], right[3];
    float w_factor, h_factor;
    uint32_t width, height;
    uint64_t id_offset;
    uint32_t n_items;
    uint32_t band_stride, band_phase;
} wt_raygen;

/* what a trace launch is: the whole thing, or one of the two passes of an adaptive launch -- its 1-sample base pass, which is the factor-1
 * launch in everything (scheduling state included), or its refine pass, the supersampled launch served from the classifier's list */
enum { WT_PASS_PLAIN = 0, WT_PASS_BASE = 1, WT_PASS_REFINE = 2 };

typedef struct {
    /* the knobs */
    int32_t depth, strict, fuse, counting, stamps, tpt_clock, variant;
    int32_t supersample;            /* 1, 2, 4 or 8 */
    int32_t adaptive;               /* contrast threshold, -1 = off (the mode check only) */
    uint32_t seed_offset;
    int32_t acc_frame, acc_jitter;  /* the frame of an accumulated view this launch folds in, -1 = not an accumulated launch */
    float aperture, focus, through;
    uint32_t tpt_max, tpt_pool_mb, tpt_min, split_min_quota, occ_tiles_per_depth;
    int32_t sched;                  /* cost-sorted tile dispatch on */
    uint32_t diag;                  /* whitted_params.diag of a WT_V_TIMELINE launch (read from the environment by the shim) */
    uint64_t id_offset;             /* the wrapper's id offset and row bands: what a launch from a caller's ray buffer falls back to */
    uint32_t band_stride;
    /* the scene as prepared: counts, float4s of prepared geometry, side table built, uniform grid built and switched on */
    int32_t scene_ok;               /* arguments 1-6, 8, 9 are bound and well formed */
    uint32_t ns, np, nl, geom_f4;
    int32_t have_lpt, grid_usable;
    /* the ray buffer of argument 0 */
    int32_t args_ok;                /* the ray handle resolves, `total` and the framebuffer are bound */
    /* rays_generated: 0 = the caller's rays; else the rays of a raygen launch of this library, 1 + the CLW_PROJ_* camera model they are generated
     * under -- 1 = the pinhole, 2 = the orthographic view, 3 = the panorama (wt_plan_projection).  A projected launch is never fused: its records
     * are generated into the ray buffer (wt_raygen_proj) and traced as a ray buffer is. */
    int32_t rays_generated, rays_exposed;
    wt_raygen gen;
    uint64_t rays_size;
    /* the range */
    uint64_t array_size, out_size;  /* the launch's size argument; bytes of the framebuffer */
    uint32_t total;
    /* one strip of a pipelined read-back: rows [row0, row0 + rows) of the range (the caller checked: whole rows, no bands) */
    int32_t has_strip;
    uint32_t strip_row0, strip_rows;
    int32_t pass;
    /* the caller's tables (NULL / 0 = none): sample cameras, sy * n + sx order; explicit sample times; 3 displacement floats per sphere */
    const clw_sample_camera* cams;
    const float* times;
    const float* disp;
    uint32_t n_cams, n_times, n_disp;
    int32_t explicit_times;
} wt_plan_in;

enum { WT_PLAN_LAUNCH = 0, WT_PLAN_NONE = 1 /* an empty range: no launch */, WT_PLAN_REFUSED = 2 };

typedef struct {
    int32_t status;
    int32_t flags;                  /* WT_F_*: the compiled kernel */
    uint32_t grid, dyn_lds;         /* workgroups, bytes of dynamic LDS */
    whitted_params P;               /* every scalar field; the shim adds the device pointers (and takes the tail's words back when it has no pool) */
    uint64_t out_offset;            /* the launch writes from this pixel of the framebuffer on (a strip) */
    uint32_t out_pixels;            /* output pixels of the launch: what an accumulation buffer is sized for */
    int32_t fused;                  /* primary rays are generated in the kernel; else read from the ray buffer */
    int32_t need_counters;          /* the launch gets the counter block */
    int32_t ss;                     /* the factor of this pass */
    /* tile geometry: tile rows, tiles per row, dispatch entries per XCD share without and with the split's extra ones */
    uint32_t trows, tpr, per_share, per_share_cap;
    int32_t use_order;              /* a tiled launch that writes tile costs and reads a cost-sorted order */
    int32_t split;                  /* heavy tiles are split ... */
    uint32_t split_max_lg;          /* ... into at most 1 << split_max_lg parts */
    int32_t tail_wanted;            /* the tree-parallel tail: a pool slot of tpt_slice words holds tpt_cap nodes */
    uint32_t tpt_slice, tpt_cap, tpt_nslots;
    wt_raygen sig;                  /* the scheduling signature's camera: the (virtual) frame the tile costs belong to */
    int32_t samples_decided;        /* the plan got as far as the tables: n_cams / n_times below are what the launch uses (0 = none) */
    uint32_t n_cams, n_times;
    uint32_t motion_floats;         /* floats of motion_table in use: whole wt_cam_tables, 0 = the scene stands still */
    char message[200];              /* WT_PLAN_REFUSED: the text of the error */
    /* written when the launch uses them, and only then: the cameras and times used (sy * n + sx order) and the two device-layout tables --
     * 12 floats per lane; 64 per-lane times, then a float4 per sphere */
    clw_sample_camera cams_used[64];
    float times_used[64];
    wt_cam_table cam_table;
    float motion_table[2 * WT_CAM_TABLE_FLOATS];
} wt_plan_out;

/* The plan of one trace launch -> its status (also out->status).  Writes the head of `out` (up to and including `message`) always, the
 * tables behind it only when the launch uses them. */
int wt_plan(const wt_plan_in* in, wt_plan_out* out);
/* What the modes do not combine with, before any launch of a trace call: `accumulating` = frame accumulation is on, else in->adaptive says
 * whether the call is adaptive.  -> 0, or WT_PLAN_REFUSED and the text in message[200]. */
int wt_plan_mode_check(const wt_plan_in* in, int accumulating, char* message);
/* the camera model of the launch's generated rays (CLW_PROJ_*; 0 = the pinhole, and what a caller's rays have) */
int wt_plan_projection(const wt_plan_in* in);
/* work-items of a launch: the size argument rounded as the reference rounds it, guarded by `total` and the framebuffer */
uint64_t wt_plan_range(uint64_t array_size, uint32_t total, uint64_t out_size);
/* a tile's lane (lane & 7, lane >> 3) traces sub-sample (sx, sy) = both mod n -> sy * n + sx */
uint32_t wt_plan_lane_sample(uint32_t lane, uint32_t n);
/* workgroups: tiled, the tile rows dealt to the 8 XCDs -- 8 * ceil(trows / 8) * tpr; linear, ceil(n_items / WT_BLOCK) */
uint32_t wt_plan_grid(const whitted_params* P);
/* the range words of a launch that generates its primary rays: camera, frame, id range, bands, tiled / rows / row_offset, unit_dirs (P->ns is set) */
void wt_plan_fused_range(const wt_raygen* g, uint32_t n_items, whitted_params* P);
/* how the kernels read the scene: the uniform grid (WT_F_GRID), geometry staged in LDS (WT_F_GEOM_LDS and its bytes) or from global memory;
 * with it the side table and the visibility classes of the lights */
typedef struct { int32_t flags; uint32_t dyn_lds, lpt, vis; } wt_geom_class;
wt_geom_class wt_plan_geometry(int strict, int variant, uint32_t ns, uint32_t np, uint32_t geom_f4, int have_lpt, int grid_usable);
/* how a ray query (whitted_cast.inc: wt_cast) of `n` rays reads the scene and how it is launched.  The geometry class is the primary-hit
 * pass's, by the same rules: the uniform grid when it is built and on (not WT_V_NO_GRID), else the scene staged in LDS when it fits
 * WT_GEOM_LDS_MAX_F4 float4 (and not WT_V_GEOM_GLOBAL), else global memory.  A workgroup is one wave that serves `batches` consecutive batches
 * of 64 rays: WT_CAST_BATCHES_LDS where the scene is staged (the staging is paid once per workgroup), 1 elsewhere; `batches_req` > 0 overrides
 * it (the tuning knob CLWRAP_CAST_BATCHES; capped at WT_CAST_BATCHES_MAX).  groups = 0: n is not a count the queries accept.
 * WT_CAST_BATCHES_LDS = 1 is the measured optimum (tools/cast_times.py --batches, 2 M rays: 1 / 2 / 4 / 8 / 16 batches cost 0.0235 / 0.0238 /
 * 0.0244 / 0.0271 / 0.0335 ms on the demo scene and 0.256 / 0.268 / 0.297 / 0.368 / 0.534 ms on 256 spheres): at most 4.2 KiB are ever staged
 * (more than 256 spheres are not), four loads per lane against hundreds of tests, while every further batch takes a wave's worth of parallelism
 * away from the machine. */
enum { WT_CAST_BATCHES_LDS = 1, WT_CAST_BATCHES_MAX = 64 };
typedef struct { int32_t flags; uint32_t dyn_lds, groups, batches; } wt_cast_class;
wt_cast_class wt_plan_cast(int variant, uint32_t ns, uint32_t geom_f4, int grid_usable, uint32_t n, uint32_t batches_req);
/* how a proximity query (whitted_near.inc: wt_near) of `n` probes reads the scene and how it is launched: the geometry class by wt_plan_cast's
 * rules, one wave per workgroup, one batch of 64 probes each (groups = 0: n is not a count the queries accept).  `grid_usable` here also asks
 * that every prepared r * r word is finite (the box proof of whitted_near.inc needs it; the shim checks when it builds the grid).
 * box_cells: on the grid, the most cells a probe's box may cover before the probe scans every sphere instead -- `box_cells_req` >= 0
 * overrides it (the tuning knob CLWRAP_NEAR_BOX_CELLS; 0 = every probe scans), else WT_NEAR_BOX_CELLS.  A probe with a box of c cells pays c
 * cell-range fetches and the tests of the spheres listed there; one that scans pays ns tests.  At about 1.6 spheres per cell and 2-3 cells
 * per sphere, c cells hold about 4 c entries, so the two meet near c = ns / 4; below a cap, a wave waits for its largest box, above it for
 * the scan.  WT_NEAR_BOX_CELLS is a provisional constant of that order for the scenes that get a grid at all (more than 256 spheres); the sweep
 * that should choose it (tools/near_times.py --cap-sweep) has not been run yet. */
enum { WT_NEAR_BOX_CELLS = 512 };
typedef struct { int32_t flags; uint32_t dyn_lds, groups, box_cells; } wt_near_class;
wt_near_class wt_plan_near(int variant, uint32_t ns, uint32_t geom_f4, int grid_usable, uint32_t n, int32_t box_cells_req);

/* Which tile order a tiled launch reads and which builds it must wait for (hip_wrap.cpp: Impl::Sched).  Trace k writes its tile costs into
 * cost[wr]; when the signature changed, order[wr] is built from them on a side stream behind it, while trace k + 1 already runs with the
 * order built two frames earlier. */
typedef struct {
    int32_t have[2];                /* order[i] holds / will hold a schedule */
    int32_t wr;                     /* cost buffer the next trace writes */
    int32_t newest;                 /* the order built last */
    int32_t sig_valid, sig_age;     /* the newest order was built for a known signature; launches since (saturating) */
    uint64_t frame, newest_frame;   /* tiled launches so far; the one the newest order was built behind */
} wt_order_state;
typedef struct { int32_t rd /* order the launch reads, -1 = the default order */, wait_wr, wait_rd /* builds to wait for first */; } wt_order_choice;
wt_order_choice wt_order_choose(wt_order_state* s);
/* whether the costs of this launch are sorted behind it: the signature changed, or a grid build refines its first order once */
int wt_order_rebuild(wt_order_state* s, int sig_changed, int grid_build);
/* the launch is enqueued: note the build behind it (if any) and swap the buffers */
void wt_order_launched(wt_order_state* s, int rebuilt);

/* Whether a planned launch reads a primary-ray cull table (whitted_params.h: whitted_kargs; primary_cull_host.h): a shallow, tiled, fused
 * 1-sample launch of the pinhole camera over a linearly scanned scene, unless variant 32768.  Everything else -- a grid scene, a launch from a
 * ray buffer (a projection's included), sample cameras, moving spheres, any supersampled or deep launch -- gets a null table.  The table is
 * indexed like the tile costs and keyed by the launch's camera, range and scene (hip_wrap.cpp: bind_primary_cull). */
int wt_plan_cull(const wt_plan_in* in, const wt_plan_out* out);

/* whether the fast / strict build compiled a trace kernel for a flag word (whitted_launch.inc) */
int wt_fast_has_trace(int flags);
int wt_strict_has_trace(int flags);
/* sizeof(wt_plan_in), sizeof(wt_plan_out) and offsetof(wt_plan_out, message), for the tests' mirror */
void wt_plan_sizes(uint32_t out[3]);
/* status and flag word of n plans (the mode check first, accumulating = acc_frame >= 0): for walks over many launches */
void wt_plan_many(const wt_plan_in* in, size_t n, int32_t* status, int32_t* flags);

#ifdef __cplusplus
}
#endif
#endif
