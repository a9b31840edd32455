/*
 * whitted_params.h -- launch parameters shared by the host shim and the HIP kernels.
 *
 * "Prepared geometry": one float4 stream per scene, built once on the host from the raw
 * wire structs (scene_prep.c) so the intersection loops read 16 B per sphere instead of
 * the 96-B rsphere the reference copies per test (reference primitives.cl:295,338,409):
 *
 *   geom[0 .. ns)                 sphere i : { cx, cy, cz, +-r*r }   sign bit set = transparent
 *   geom[ns + 2p], geom[ns+2p+1]  plane p  : { nx, ny, nz, has_texture ? 1 : 0 }, { px, py, pz, 0 }
 *   geom[ns + 2np + 2l], [..+1]   light l  : { ox, oy, oz, r*r }, { lr, lg, lb, radius }
 *                                            with l* = (rgb * intensity) * (1/pi)
 *   geom[ns + 2np + 2nl + c*np + p]  (only if lpt != 0) light chunk c, plane p: { mu0, mu1, mu2, 1/|n| } -- the signed
 *                                            distance of the three lights of the chunk from the plane, less radius and
 *                                            slack (scene_prep.c): lets a wave skip plane tests no shadow ray can fail
 *   (LDS copy only) [geom_f4 + i] sphere i : { dx, dy, dz, 0 } of a moving launch's displacement table (ss_disp below), staged behind the stream
 *   ptex[2p], ptex[2p+1]          plane p  : { b0x, b0y, b0z, texture_scale }, { b1x, b1y, b1z, bits(texture_id) }
 *                                            (tangent basis of reference primitives.cl:226-236)
 * Materials stay in the raw arrays and are gathered for the winning primitive only.
 */
#ifndef WHITTED_PARAMS_H
#define WHITTED_PARAMS_H
#include <stdint.h>

#define CLW_MAX_DEPTH 32 /* deepest supported trace depth (hip_wrap_ext.h) */
#define CLW_NUM_COUNTERS 32
#define CLW_STAMP_SHARDS 1024 /* diagnostic stamp build: 16-word shards behind the counter block, summed into words 16.. on read */ /* words of the device counter block (hip_wrap_ext.h: clw_ext_read_counters_ex); 16.. = phase stamps of the diagnostic build */

/* ---- the launch vocabulary: which compiled trace kernel a launch runs (the FLAGS of wt_trace<FLAGS>; clw_ext_last_trace_flags) -------- */
#define WT_BLOCK 64                  /* one wavefront = one 8x8 tile = one workgroup: a finished tile frees its
                                        LDS and wave slot at once instead of waiting for three neighbours      */
#ifndef WT_VIS_MAX_SPHERES
#define WT_VIS_MAX_SPHERES 16        /* the light visibility classes (wt_light_vis) cost one pass over the spheres per light chunk: small scenes only */
#endif
enum { WT_F_COUNT = 1, WT_F_DEEP = 2, WT_F_GEOM_LDS = 4, WT_F_RAYS = 8, WT_F_GRID = 16,
       WT_F_OCC = 32 /* deep builds only: the high-occupancy flavour (see WT_LDS_LEVELS of whitted_trace.inc) */,
       WT_F_D8 = 64, WT_F_D16 = 128 /* deep builds only: the launch's depth is <= 8 / <= 16, so the DFS stack holds at most 7 / 15 parents and the
                                       part of it kept in scratch is sized for that instead of for CLW_MAX_DEPTH */,
       WT_F_SHAPE = 256 /* shallow fast LDS-geometry build only: the scene's counts are compiled in (wt_shape) */,
       WT_F_SS = 1 << 17 /* n x n supersampling, fused tiled launches only (bits 9-16: the counts of WT_SHAPE_FLAGS) */,
       WT_F_MOVE = 1 << 18 /* on top of WT_F_SS, not the grid builds: moving spheres (wt_sphere_at) -- a flavour of its own, so that the plain
                              supersampled kernels are the code they were */,
       WT_F_LIST = 1 << 19 /* on top of WT_F_SS, not with WT_F_MOVE: the refine pass of an adaptive launch -- a wave first asks the device-side length of
                              its list (list_count below) whether it has a tile at all; again a flavour of its own */,
       WT_F_ACC = 1 << 20 /* the seed offset and progressive accumulation (seed_offset, acc_sum below) are one more scalar word and a wave-uniform
                              run-time branch of the epilogue in every flavour but the few whose register allocation they disturbed (wt_acc_flagged:
                              the strict build's shallow counting and grid kernels, which sit on their 128-VGPR cap): those read neither unless
                              they are this twin, so that they are the code they were; the planner asks for the twin when the launch has a seed
                              offset or accumulates */ };
/* the shaped flavour (wt_shape of whitted_trace.inc) carries the scene's counts in bits 9-11, 12-13 and 14-16; exactly these counts are
 * compiled (whitted_launch.inc) and asked for (launch_plan.c): 1..WT_SHAPE_MAX_SPHERES spheres, 0..WT_SHAPE_MAX_PLANES planes, WT_SHAPE_LIGHTS lights */
#define WT_SHAPE_FLAGS(ns, np, nl) (WT_F_GEOM_LDS | WT_F_SHAPE | ((ns) << 9) | ((np) << 12) | ((nl) << 14))
enum { WT_SHAPE_MAX_SPHERES = 4, WT_SHAPE_MAX_PLANES = 2, WT_SHAPE_LIGHTS = 3 };

typedef struct {
    /* camera: the eight by-value raygen arguments (reference raygen.cl:5-8) */
    float corner[3], origin[3], up[3], right[3];
    float w_factor, h_factor;
    uint32_t width, height;
    /* work range: work-item i <-> global id id_offset + i, i in [0, n_items) */
    uint64_t id_offset;
    uint32_t n_items;
    uint32_t tiled;        /* 1: range is whole rows -> 8x8 pixel tile per wavefront */
    uint32_t rows;         /* tiled: number of rows in the range                      */
    uint32_t row_offset;   /* tiled: global row of the range's first row (= id_offset / width) */
    /* interleaved 8-row bands (multi-GPU load balance): local row y is global row
     * ((y/8)*band_stride + band_phase)*8 + y%8; band_stride <= 1 = contiguous range        */
    uint32_t band_stride, band_phase;
    /* cost-sorted tile dispatch (tiled mode; both nullable): tile_order[b] = tile served by workgroup b
     * (packed: tile column | tile row << 12 | log2(parts) << 24 | part << 27; 0xFFFFFFFF = none), heaviest tiles of the previous frame first, one list per
     * XCD interleaved as order[8*j + k]; tile_cost[tile] receives this frame's cost of every tile.  */
    const uint32_t* tile_order;
    uint32_t* tile_cost;
    /* the tree-parallel tail of deep launches (whitted_tpt.inc): once at most tpt_max lanes of a tile's wave are alive and they hold at
     * least tpt_min pending paths, the rest of the tile is traced by the whole wave as one pool of segments whose nodes live in a slot
     * of tpt_pool: 8 x tpt_slots slots (tpt_slots per XCD) of tpt_slice_words words, room for tpt_cap nodes each; tpt_flags[8 * tpt_slots]:
     * 1 = slot taken (tpt_cap 0 = no tail: the per-lane loop runs to the end) */
    uint32_t* tpt_pool;
    uint32_t* tpt_flags;
    const uint32_t* tpt_jump;   /* [7][32]: the GF(2) matrices M^(2^i), M = the xorshift steps of one shaded hit (4 x lights), as columns */
    uint32_t tpt_slice_words, tpt_cap, tpt_slots, tpt_max, tpt_min;
    uint32_t tpt_clock;    /* DIAGNOSTIC: 1 = the tail books its phases' durations into counter words 10-25 (`counters` must be set) */
    uint32_t cost_sum;     /* 1: a tile's cost is the SUM over its lanes (and over the wavefronts that share the tile), added atomically to a zeroed tile_cost; 0: the maximum over its lanes, stored */
    int32_t depth;         /* reference MAX_DEPTH                                     */
    uint32_t untrimmed;    /* A/B and equivalence tests (variant 16384): 1 = the bounce block also runs on a path's last level and the tile cost is
                              reduced by the shuffle butterfly, as before both were trimmed (whitted_bounce.inc, wt_wave_reduce); same image, same costs */
    /* scene */
    const float* geom;     /* float4 stream, layout above                             */
    const float* ptex;     /* float4 x 2 per plane                                    */
    const uint8_t* spheres_raw; /* 96-B rsphere array (materials)                     */
    const uint8_t* planes_raw;  /* 96-B rplane array                                  */
    uint32_t ns, np, nl;
    float through;         /* factor a transparent sphere applies to a shadow ray: 0.8f = reference primitives.cl:7 (clw_ext_set_shadow_through) */
    uint32_t geom_f4;      /* number of float4 in geom                                */
    uint32_t unit_dirs;    /* 1: ray directions are unit (this library's own rays) and the scene is small: the fast build takes a = d.d = 1 */
    uint32_t lpt;          /* 1: the light / plane side table follows the lights in geom */
    uint32_t vis;          /* strict build, small scenes: 1: lights are sorted into visibility classes (wt_light_vis) and only the samples of
                              undecided ones are traced; 2 (counting build): classify AND trace, count disagreements in counter word 28 */
    uint32_t diag;         /* DIAGNOSTIC builds (-DWT_TIMELINE=1) only: 1 + s = tile_cost receives (start << 16 | end) in ticks of 10 ns << s, not costs */
    /* uniform grid over the spheres (big scenes only; see scene_prep.c wprep_grid_*): cell c holds
     * grid_items[grid_start[c] .. grid_start[c+1]) = sphere indices in ascending order; grid_box[2i], [2i+1] =
     * sphere i's inclusive cell box, 10 bits per axis: lo = x0 | y0<<10 | z0<<20, hi likewise               */
    const uint32_t* grid_start;
    const uint32_t* grid_items;
    const uint32_t* grid_box;
    const float* grid_geom;   /* float4 per cell-list entry: geom[grid_items[k]], so a test costs one load, not two dependent ones */
    float grid_min[3], grid_inv[3], grid_cell[3];
    uint32_t grid_pair;      /* 1: spheres are listed a light radius beyond their boxes: the two samples of a light share one walk (wt_grid_shadow_pair) */
    int32_t grid_res[3];
    /* images: RGBA8 layer stacks */
    const uint32_t* tex; int32_t tex_w, tex_h, tex_layers;
    const uint32_t* sky; int32_t sky_w, sky_h;
    /* I/O */
    const float* rays;     /* unfused path: 64-B rray records, else NULL              */
    uint32_t* out;         /* packed 0x00RRGGBB per work-item                         */
    float* out_rgb;        /* optional float radiance, 3 per work-item                */
    unsigned long long* counters; /* counting build only: CLW_NUM_COUNTERS words          */
    /* n x n supersampling, n = 1 << ss_lg (tiled launches; 0 = off): the camera, width, rows, row_offset, id_offset, n_items and the tile
     * buffers above describe the VIRTUAL frame of n x as many columns and rows; the n x n samples of an output pixel sit in adjacent lanes
     * of one wavefront and are resolved in registers (wt_ss_resolve); out / out_rgb hold one entry per OUTPUT pixel, width >> ss_lg per row */
    uint32_t ss_lg;
    /* sample cameras of a supersampled launch (NULL = every sample looks through the launch camera above): WT_CAM_TABLE_FLOATS floats,
     * 12 per LANE of a tile's wavefront -- { im_corner, origin, up, right } of the camera of sub-sample ((lane & 7) mod n, (lane >> 3) mod n);
     * w_factor, h_factor, width, height stay the launch's (16-byte aligned) */
    const float* ss_cams;
    /* moving spheres of a supersampled launch (NULL = the scene stands still): ss_disp = float4 { dx, dy, dz, 0 } per sphere, the movement of
     * its centre while the shutter is open; ss_times = 64 floats, the scene time of the sub-sample each LANE of a tile's wavefront traces (laid
     * out like ss_cams).  A lane sees sphere i at fmaf(t_lane, d_i, c_i) per component (wt_sphere_at); radius, planes and lights stand still.
     * Small non-grid scenes only (ns <= 256); LDS-geometry kernels stage the table behind the prepared stream (geom_f4 + ns <= 1024 float4) */
    const float* ss_disp;
    const float* ss_times;
    /* the refine pass of an adaptive supersampled launch (the WT_F_LIST flavours; wt_refine_classify wrote both): tile_order holds eight lists
     * interleaved as order[8 * j + k], list k -- the refined tiles of the tile rows r = 8m + k -- being list_count[WT_LIST_COUNT_STRIDE * k]
     * entries long (a cache line per counter); the grid is sized for full lists, and workgroup b leaves at once unless b / 8 is below the
     * length of list b % 8 */
    const uint32_t* list_count;
    /* progressive frame accumulation (NULL = off; hip_wrap_ext.h: clw_ext_set_accumulate): acc_sum holds 3 floats per OUTPUT pixel, indexed like
     * out -- the running sum of the clamped (1 sample) or resolved (supersampled) value the plain launch would pack; the lane that packs a pixel
     * stores its value (acc_scale == 1.0f: the first frame, a store with no read) or adds it, and packs fminf(sum * acc_scale, 1.0f), acc_scale
     * = 1 / frames, correctly rounded by the host; out_rgb, when bound, receives that mean */
    float* acc_sum;
    float acc_scale;
    /* added mod 2^32 to the global id that seeds a work-item's xorshift state (clw_ext_set_seed_offset; an accumulated frame adds its own);
     * nothing else reads it: pixel positions, buffers and guards keep the id */
    uint32_t seed_offset;
} whitted_params;

/* What wt_trace_cull receives, the twin of wt_trace that a launch WITH a primary-ray cull table runs (a launch without one runs wt_trace on the
 * whitted_params alone): the parameters, and behind them the table: TWO bytes per tile, indexed like tile_cost.  The first is the primary byte
 * (primary_cull_host.h): bit 0 = no primary ray of the tile can meet the line test of any sphere, bit 1 = of any light sphere; the first loop
 * iteration of the tile's wave skips the group (whitted_hit.inc).  The second is the bounce byte (bounce_cull_host.h): the sphere classes the
 * first shade's shadow batch skips, and the two groups again for the second iteration.  Read as whole words: the allocation is a multiple of
 * four bytes.  The pointer travels BEHIND whitted_params, not inside it: the struct is embedded in the planner's wt_plan_out, whose
 * layout the planner's tests mirror field by field, and the planner has nothing to say about a device pointer.  Only shallow fused tiled
 * launches of the pinhole camera without sample cameras, moving spheres, supersampling or a grid get a table (launch_plan.h: wt_plan_cull). */
typedef struct {
    whitted_params P;
    const uint8_t* tile_cull;
} whitted_kargs;

#define WT_LIST_COUNT_STRIDE 32
#define WT_CAM_TABLE_FLOATS (64 * 12)
typedef struct { float v[WT_CAM_TABLE_FLOATS]; } wt_cam_table;   /* the table as a by-value kernel argument (wt_cams_store) */

typedef struct {
    float corner[3], origin[3], up[3], right[3];
    float w_factor, h_factor;
    uint32_t width, height;
    uint64_t id_offset;
    uint32_t n_items;
    uint32_t band_stride, band_phase;
    float* rays;           /* 16 floats per work-item                                 */
} raygen_params;

#endif
