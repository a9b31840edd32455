/* whitted_launch.inc -- instantiates the kernels of whitted_trace.inc (and the primary-hit pass of whitted_gbuffer.inc, built from its
 * pieces, the camera models of whitted_projection.inc, the queries' shared scan of whitted_query.inc, the ambient occlusion pass of
 * whitted_ao.inc, the ray queries of whitted_cast.inc, the layered ray queries of whitted_layers.inc, the proximity queries of whitted_near.inc, the path queries of whitted_paths.inc, the selection overlay of
 * whitted_overlay.inc, the visible-object table of whitted_objects.inc and the builder of the primary-ray cull table of whitted_cull.inc) in
 * namespace WT_NS and exports the C launchers the shim calls. */
#include "bounce_cull_host.h"      /* (and through it primary_cull_host.h) */
#include "ref_tests.h"             /* the reference arithmetic of the passes beside the trace launch: one text, host and device */
namespace WT_NS {
#include "whitted_trace.inc"
#include "whitted_gbuffer.inc"
#include "whitted_projection.inc"
#include "whitted_query.inc"
#include "whitted_ao.inc"
#include "whitted_cast.inc"
#include "whitted_layers.inc"
#include "whitted_near.inc"
#include "whitted_paths.inc"
#include "whitted_overlay.inc"
#include "whitted_objects.inc"
#include "whitted_cull.inc"
}

template <int FLAGS>
static hipError_t wt_launch_one(const whitted_params* P, const unsigned char* tile_cull, unsigned grid, size_t dyn_lds, hipStream_t s) {
    /* a launch with a cull table runs the twin that reads it; every other launch runs wt_trace, which knows nothing of tables */
    if constexpr (WT_NS::wt_cull_flavour(FLAGS)) {
        if (tile_cull) {
            const whitted_kargs K = {*P, tile_cull};
            hipLaunchKernelGGL(WT_NS::wt_trace_cull<FLAGS>, dim3(grid), dim3(WT_BLOCK), dyn_lds, s, K);
            return hipGetLastError();
        }
    } else if (tile_cull) return hipErrorInvalidValue;      /* (launch_plan.c: wt_plan_cull gives such a flavour no table) */
    hipLaunchKernelGGL(WT_NS::wt_trace<FLAGS>, dim3(grid), dim3(WT_BLOCK), dyn_lds, s, *P);
    return hipGetLastError();
}

/* the compiled trace kernel of a flag word, or null: the shaped flavours by their exact word, the others by the bits that select a kernel */
typedef hipError_t (*wt_trace_launcher)(const whitted_params*, const unsigned char*, unsigned, size_t, hipStream_t);
static wt_trace_launcher wt_find_trace(int flags) {
#if !WT_STRICT
    if (flags & WT_F_SHAPE) {
        /* the shaped flavour (wt_shape): exactly these counts are compiled -- 1..4 spheres, 0..2 planes, 3 lights; the planner asks for no other */
        switch (flags) {
#define WT_SHAPE_CASE(ns, np) case WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS): return wt_launch_one<WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS)>; \
                              case WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS) | WT_F_SS: return wt_launch_one<WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS) | WT_F_SS>; \
                              case WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS) | WT_F_SS | WT_F_LIST: return wt_launch_one<WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS) | WT_F_SS | WT_F_LIST>; \
                              case WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS) | WT_F_SS | WT_F_MOVE: return wt_launch_one<WT_SHAPE_FLAGS(ns, np, WT_SHAPE_LIGHTS) | WT_F_SS | WT_F_MOVE>;
#define WT_SHAPE_CASES(ns) WT_SHAPE_CASE(ns, 0) WT_SHAPE_CASE(ns, 1) WT_SHAPE_CASE(ns, 2)
            WT_SHAPE_CASES(1) WT_SHAPE_CASES(2) WT_SHAPE_CASES(3) WT_SHAPE_CASES(4)
#undef WT_SHAPE_CASES
#undef WT_SHAPE_CASE
        }
        return nullptr;
    }
#endif
    switch (flags & (255 | WT_F_SS | WT_F_MOVE | WT_F_LIST | WT_F_ACC)) {
#define WT_CASE(F) case F: return wt_launch_one<F>;
/* F, its supersampled twin (fused launches only: no twin for the ray-buffer flavours, bit 3) and the twin's list-driven flavour (adaptive launches) */
#define WT_CASE2(F) WT_CASE(F) WT_CASE((F) | WT_F_SS) WT_CASE((F) | WT_F_SS | WT_F_LIST)
/* ... and the twin's moving-spheres flavour (not the grid builds) */
#define WT_CASE3(F) WT_CASE2(F) WT_CASE((F) | WT_F_SS | WT_F_MOVE)
        WT_CASE3(0) WT_CASE3(1) WT_CASE3(2) WT_CASE3(3) WT_CASE3(4) WT_CASE3(5) WT_CASE3(6) WT_CASE3(7)
        WT_CASE(8) WT_CASE(9) WT_CASE(10) WT_CASE(11) WT_CASE(12) WT_CASE(13) WT_CASE(14) WT_CASE(15)
        /* grid builds: geometry from global memory only (bit 2 clear) */
        WT_CASE2(16) WT_CASE2(17) WT_CASE2(18) WT_CASE2(19) WT_CASE(24) WT_CASE(25) WT_CASE(26) WT_CASE(27)
        /* deep builds whose depth is <= 8 (bit 6) / <= 16 (bit 7): a smaller scratch part of the DFS stack (not the counting builds) */
        WT_CASE3(66) WT_CASE3(70) WT_CASE(74) WT_CASE(78) WT_CASE2(82) WT_CASE(90)
        WT_CASE3(130) WT_CASE3(134) WT_CASE(138) WT_CASE(142) WT_CASE2(146) WT_CASE(154)
#if WT_STRICT
        /* the shallow counting and grid kernels (wt_acc_flagged): their twins that read the seed offset and accumulate */
        WT_CASE3(1 | WT_F_ACC) WT_CASE3(5 | WT_F_ACC) WT_CASE(9 | WT_F_ACC) WT_CASE(13 | WT_F_ACC)
        WT_CASE2(16 | WT_F_ACC) WT_CASE2(17 | WT_F_ACC) WT_CASE(24 | WT_F_ACC) WT_CASE(25 | WT_F_ACC)
#endif
#if !WT_STRICT
        WT_CASE3(98) WT_CASE3(102) WT_CASE(106) WT_CASE(110) WT_CASE2(114) WT_CASE(122)
        WT_CASE3(162) WT_CASE3(166) WT_CASE(170) WT_CASE(174) WT_CASE2(178) WT_CASE(186)
        /* deep builds, high-occupancy flavour (bit 5 on top of bit 1) */
        WT_CASE3(34) WT_CASE3(35) WT_CASE3(38) WT_CASE3(39) WT_CASE(42) WT_CASE(43) WT_CASE(46) WT_CASE(47)
        WT_CASE2(50) WT_CASE2(51) WT_CASE(58) WT_CASE(59)
#endif
#undef WT_CASE3
#undef WT_CASE2
#undef WT_CASE
    }
    return nullptr;
}

/* `tile_cull`: the primary-ray cull table of the launch (whitted_params.h: whitted_kargs), or null = every test runs */
WT_LAUNCHER(trace)(const whitted_params* P, const unsigned char* tile_cull, int flags, unsigned grid, size_t dyn_lds,
                                      hipStream_t s) {
    const wt_trace_launcher run = wt_find_trace(flags);
    return run ? run(P, tile_cull, grid, dyn_lds, s) : hipErrorInvalidValue;
}

#if !WT_STRICT   /* double-precision work that is the same in both builds: one copy, in the fast unit */
/* the cull table (whitted_cull.inc) of the tiled launch `P` describes, into `table`: two bytes per tile -- the primary byte, the bounce byte with
 * the parts `parts` (WT_BC_PART_*) --, trows x tpr of them */
WT_LAUNCHER(cull)(const whitted_params* P, unsigned parts, unsigned char* table, hipStream_t s) {
    const unsigned long long tpr = (P->width + 7ull) / 8ull, trows = (P->rows + 7ull) / 8ull;
    if (!P->tiled || P->width == 0u || P->rows == 0u || tpr * trows >= (1ull << 30) || !table || !P->geom) return hipErrorInvalidValue;
    WT_NS::wt_cull_args A = {};
    for (int a = 0; a < 3; a++) { A.V.corner[a] = P->corner[a]; A.V.origin[a] = P->origin[a]; A.V.up[a] = P->up[a]; A.V.right[a] = P->right[a]; }
    A.V.w_factor = P->w_factor; A.V.h_factor = P->h_factor;
    A.V.width = P->width; A.V.rows = P->rows; A.V.row_offset = P->row_offset; A.V.band_stride = P->band_stride; A.V.band_phase = P->band_phase;
    A.S.spheres = P->geom; A.S.planes = P->geom + 4 * (size_t)P->ns; A.S.lights = P->geom + 4 * ((size_t)P->ns + 2 * (size_t)P->np);
    A.S.planes_raw = (const uint32_t*)P->planes_raw;
    A.S.ns = P->ns; A.S.np = P->np; A.S.nl = P->nl; A.S.depth = P->depth > 0 ? (unsigned)P->depth : 0u;
    if (A.S.np > 0u && !A.S.planes_raw) parts = 0u;      /* (no raw records to read the planes' materials from: the primary byte alone) */
    A.tiles = (unsigned)(tpr * trows); A.tpr = (unsigned)tpr; A.parts = parts; A.table = table;
    hipLaunchKernelGGL(WT_NS::wt_primary_cull_build, dim3((A.tiles + 255u) / 256u), dim3(256), 0, s, A);
    return hipGetLastError();
}
#endif

/* whether this build compiled a trace kernel for the flag word (csrc/launch_plan.h: the planner's tests hold every word it returns to it) */
extern "C" int WT_NAME(has_trace)(int flags) { return wt_find_trace(flags) != nullptr; }

WT_LAUNCHER(raygen)(const raygen_params* P, hipStream_t s) {
    unsigned grid = (P->n_items + WT_RG_BLOCK - 1) / WT_RG_BLOCK;
    hipLaunchKernelGGL(WT_NS::wt_raygen, dim3(grid), dim3(WT_RG_BLOCK), 0, s, *P);
    return hipGetLastError();
}

WT_LAUNCHER(sched)(const unsigned* cost, unsigned* order, unsigned tpr, unsigned trows,
                                      unsigned per_share, unsigned clamp_outliers, unsigned per_share_cap, unsigned split_slots,
                                      unsigned min_quota, unsigned max_lg, hipStream_t s) {
    hipLaunchKernelGGL(WT_NS::wt_sched_build, dim3(8), dim3(256), 0, s, cost, order, tpr, trows, per_share, clamp_outliers, per_share_cap,
                       split_slots, min_quota, max_lg);
    return hipGetLastError();
}

#if !WT_STRICT   /* integer work: one copy, in the fast unit, serves both builds */
WT_LAUNCHER(classify)(const unsigned* frame, unsigned width, unsigned rows, unsigned lgb, unsigned threshold,
                                         unsigned char* mask, unsigned* order, unsigned* count, unsigned cap, hipStream_t s) {
    const unsigned b = 1u << lgb, nbc = (width + b - 1u) / b, nbr = (rows + b - 1u) / b;
    const unsigned per_wave = 64u >> (2u * lgb), wpr = (nbc + per_wave - 1u) / per_wave;      /* blocks a wave owns; waves per block row */
    const unsigned long long waves = (unsigned long long)nbr * wpr;
    if (lgb > 2u || waves == 0ull || waves > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(WT_NS::wt_refine_classify, dim3((unsigned)((waves + 3ull) / 4ull)), dim3(256), 0, s, frame, width, rows, lgb, threshold, nbc, nbr,
                       wpr, mask, order, count, cap);
    return hipGetLastError();
}
#endif

WT_LAUNCHER(cams)(const wt_cam_table* T, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(WT_NS::wt_cams_store, dim3(1), dim3(64), 0, s, *T, (float4*)dst);
    return hipGetLastError();
}

WT_LAUNCHER(unit)(int op, const float* in, float* out, unsigned n, unsigned stride_in,
                                     unsigned stride_out, unsigned aux, hipStream_t s) {
    hipLaunchKernelGGL(WT_NS::wt_unit, dim3((n + 63) / 64), dim3(64), 0, s, op, in, out, n, stride_in, stride_out, aux);
    return hipGetLastError();
}

/* The geometry-flavour ladder, written once: KERNEL<GEOM_LDS, GRID TAIL> as bind_scene chose the geometry -- WT_F_GRID the uniform grid, else
 * WT_F_GEOM_LDS the scene staged in LDS, else read from global memory.  TAIL = WT_TAIL(the kernel's further template arguments), or empty.
 * Each flavour gets the dynamic LDS bytes its launcher names for it; what follows `s` are the kernel's arguments. */
#define WT_TAIL(...) , __VA_ARGS__
#define WT_LAUNCH_FLAVOUR(KERNEL, TAIL, flags, g, block, lds_grid, lds_staged, lds_global, s, ...) \
    do { \
        if ((flags) & WT_F_GRID) hipLaunchKernelGGL((WT_NS::KERNEL<false, true TAIL>), g, block, lds_grid, s, __VA_ARGS__); \
        else if ((flags) & WT_F_GEOM_LDS) hipLaunchKernelGGL((WT_NS::KERNEL<true, false TAIL>), g, block, lds_staged, s, __VA_ARGS__); \
        else hipLaunchKernelGGL((WT_NS::KERNEL<false, false TAIL>), g, block, lds_global, s, __VA_ARGS__); \
    } while (0)

WT_LAUNCHER(unit_scene)(const whitted_params* P, int flags, int op, const float* in, float* out, unsigned n,
                                           unsigned stride_in, unsigned stride_out, size_t dyn_lds, hipStream_t s) {
    const dim3 grid((n + 63) / 64), block(64);
    WT_LAUNCH_FLAVOUR(wt_unit_scene, /* no tail */, flags, grid, block, 0, dyn_lds, 0, s, *P, op, in, out, n, stride_in, stride_out);
    return hipGetLastError();
}

/* the primary-hit pass (whitted_gbuffer.inc): geometry as bind_scene chose it -- WT_F_GRID the uniform grid, WT_F_GEOM_LDS the scene staged in LDS, else
 * read from global memory; the five channel pointers in CLW_GB_* bit order, NULL = not written; `T` = the camera model (model 0: the pinhole) */
WT_LAUNCHER(gbuffer)(const whitted_params* P, int flags, unsigned grid, size_t dyn_lds, float* depth, unsigned* id,
                                        float* normal, float* point, float* albedo, const wt_projection* T, hipStream_t s) {
    const WT_NS::wt_gbuffer_out G = {depth, id, normal, point, albedo};
    const dim3 g(grid), block(WT_BLOCK);
    if (T->model != CLW_PROJ_PERSPECTIVE) WT_LAUNCH_FLAVOUR(wt_gbuffer, WT_TAIL(true), flags, g, block, 0, dyn_lds, 0, s, *P, G, *T);      /* (calls wt_proj_ray) */
    else WT_LAUNCH_FLAVOUR(wt_gbuffer, WT_TAIL(false), flags, g, block, 0, dyn_lds, 0, s, *P, G, *T);
    return hipGetLastError();
}

/* the raygen of the camera models beside the pinhole (whitted_projection.inc): wt_raygen's launch shape; `T` carries the model's terms and, for
 * the panorama, the device addresses of its two tables (width and height float4) */
WT_LAUNCHER(raygen_proj)(const raygen_params* P, const wt_projection* T, hipStream_t s) {
    if (P->n_items == 0u || P->width == 0u || (T->model != CLW_PROJ_ORTHO && T->model != CLW_PROJ_EQUIRECT) ||
        (T->model == CLW_PROJ_EQUIRECT && (!T->col || !T->row || T->width != P->width || T->height != P->height)))
        return hipErrorInvalidValue;
    unsigned grid = (P->n_items + WT_RG_BLOCK - 1) / WT_RG_BLOCK;
    hipLaunchKernelGGL(WT_NS::wt_raygen_proj, dim3(grid), dim3(WT_RG_BLOCK), 0, s, *P, *T);
    return hipGetLastError();
}

/* the selection overlay (whitted_overlay.inc) over a width x rows range: one workgroup per tile of 32 x 8 pixels, the kernel compiled for the
 * flag word (CLW_OV_* bits, 1..7); `style` = radius, outline_rgb, fill_rgb, fill_alpha, edge_rgb; the caller has checked style and selection
 * (csrc/overlay_host.h: wt_overlay_check) */
WT_LAUNCHER(overlay)(const unsigned* frame, const unsigned* ids, unsigned* out, unsigned width, unsigned rows, unsigned flags,
                                        const unsigned style[5], const unsigned* sel, unsigned count, hipStream_t s) {
    const unsigned long long tpr = (width + (WT_OV_TILE_W - 1ull)) / WT_OV_TILE_W, trows = (rows + (WT_OV_TILE_H - 1ull)) / WT_OV_TILE_H;
    if (width == 0u || rows == 0u || width > 0x7FFFFFFFu || tpr * trows > 0x7FFFFFFFull || count > 64u || flags < 1u || flags > 7u ||
        ((flags & WT_OV_OUTLINE) && (style[0] < 1u || style[0] > 4u)))
        return hipErrorInvalidValue;
    WT_NS::wt_overlay_args A = {};
    A.frame = frame; A.ids = ids; A.out = out; A.width = width; A.rows = rows; A.tiles_per_row = (unsigned)tpr;
    A.radius = style[0]; A.outline_rgb = style[1] & 0x00FFFFFFu; A.fill_rgb = style[2] & 0x00FFFFFFu; A.fill_alpha = style[3];
    A.edge_rgb = style[4] & 0x00FFFFFFu; A.count = count;
    for (unsigned k = 0; k < count; k++) A.sel[k] = sel[k];
    const dim3 g((unsigned)(tpr * trows)), block(WT_OV_TILE_W * WT_OV_TILE_H);
    switch (flags) {
#define WT_OV_CASE(F) case F: hipLaunchKernelGGL(WT_NS::wt_overlay<F>, g, block, 0, s, A); break;
        WT_OV_CASE(1) WT_OV_CASE(2) WT_OV_CASE(3) WT_OV_CASE(4) WT_OV_CASE(5) WT_OV_CASE(6) WT_OV_CASE(7)
#undef WT_OV_CASE
    }
    return hipGetLastError();
}

/* the visible-object table (whitted_objects.inc) of a width x rows range whose first row is row `first_row` of the frame: clears `table` (16
 * bytes of counters, then a 48-byte slot per possible id: counts[0] + counts[1] + counts[2] + 1 of them), reduces the pixels of the clipped
 * rectangle `clip` = {first column, first row of the range, columns, rows} (columns 0 = it misses the range: nothing to reduce) into it, in
 * tiles of 32 x 8 pixels dealt to at most WT_OBJ_MAX_GROUPS workgroups, and compacts the occupied slots into `result` (the 16-byte summary, then the records, room for one
 * per slot).  `depth` = the depth channel's bit patterns, or null.  The caller has checked the arguments (csrc/objects_host.h:
 * wt_objects_check, wt_objects_clip) */
WT_LAUNCHER(objects)(const unsigned* ids, const unsigned* depth, unsigned width, unsigned rows, unsigned first_row,
                                        const unsigned clip[4], const unsigned counts[3], void* table, void* result, hipStream_t s) {
    const unsigned long long nslots = (unsigned long long)counts[0] + counts[1] + counts[2] + 1ull;
    const unsigned long long tpr = (clip[2] + (WT_OBJ_TILE_W - 1ull)) / WT_OBJ_TILE_W, trows = (clip[3] + (WT_OBJ_TILE_H - 1ull)) / WT_OBJ_TILE_H;
    if (width == 0u || rows == 0u || (unsigned long long)width * rows >= (1ull << 30) || nslots > (1ull << 24) || !ids || !table || !result ||
        (unsigned long long)clip[0] + clip[2] > width || (unsigned long long)clip[1] + clip[3] > rows || (unsigned long long)first_row + rows > (1ull << 32))
        return hipErrorInvalidValue;
    WT_NS::wt_obj_head* head = (WT_NS::wt_obj_head*)table;
    WT_NS::wt_obj_slot* slots = (WT_NS::wt_obj_slot*)(head + 1);
    hipError_t e = hipMemsetAsync(table, 0, sizeof(WT_NS::wt_obj_head) + (size_t)nslots * sizeof(WT_NS::wt_obj_slot), s);
    if (e != hipSuccess) return e;
    if (clip[2] != 0u && clip[3] != 0u) {
        WT_NS::wt_objects_args A = {};
        A.ids = ids; A.depth = depth; A.head = head; A.slots = slots; A.width = width; A.first_row = first_row;
        A.cx = clip[0]; A.cy = clip[1]; A.cw = clip[2]; A.ch = clip[3]; A.tiles_per_row = (unsigned)tpr;
        A.c0 = counts[0]; A.c1 = counts[1]; A.c2 = counts[2];
        /* at most WT_OBJ_MAX_GROUPS workgroups, each a run of consecutive tiles (tiles <= pixels < 2^30) */
        const unsigned tiles = (unsigned)(tpr * trows), wanted = tiles < WT_OBJ_MAX_GROUPS ? tiles : WT_OBJ_MAX_GROUPS;
        A.tiles = tiles; A.tiles_per_group = (tiles + wanted - 1u) / wanted;
        const unsigned groups = (tiles + A.tiles_per_group - 1u) / A.tiles_per_group;
        hipLaunchKernelGGL(WT_NS::wt_objects_reduce, dim3(groups), dim3(WT_OBJ_TILE_W * WT_OBJ_TILE_H), 0, s, A);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    unsigned* summary = (unsigned*)result;
    hipLaunchKernelGGL(WT_NS::wt_objects_compact, dim3(1), dim3(WT_OBJ_CHUNK), 0, s, head, slots, (unsigned)nslots, counts[0], counts[1], counts[2],
                       depth ? 1u : 0u, summary, (WT_NS::wt_obj_record*)(summary + 4));
    return hipGetLastError();
}

/* ambient occlusion (whitted_ao.inc).  wt_ao_trace over the planar point / normal / id channels of a width x rows range whose first row is row
 * `first_row` of the frame: one workgroup of one wave per 8 x 8 tile, geometry as bind_scene chose it (flags as the gbuffer launcher), `dirs` = the
 * 16 x K float4 of clw_host_ao_dirs on the device, staged in LDS behind the geometry; `open` receives a byte per pixel.  The caller has checked
 * K, radius and the range (csrc/ao_host.h: wt_ao_check, wt_ao_range_ok) */
WT_LAUNCHER(ao_trace)(const whitted_params* P, int flags, const float* point, const float* normal, const unsigned* ids,
                                         const float* dirs, unsigned char* open, unsigned width, unsigned rows, unsigned first_row, unsigned K,
                                         float radius, hipStream_t s) {
    const unsigned long long tpr = (width + 7ull) / 8ull, trows = (rows + 7ull) / 8ull;
    if (width == 0u || rows == 0u || (unsigned long long)width * rows >= (1ull << 30) || K < 1u || K > 32u || !(radius > 0.0f) || !point || !normal ||
        !ids || !dirs || !open)
        return hipErrorInvalidValue;
    const bool lds = !(flags & WT_F_GRID) && (flags & WT_F_GEOM_LDS);
    const size_t dyn_lds = ((lds ? (size_t)P->geom_f4 : 0u) + 16u * (size_t)K) * sizeof(float4);
    if (dyn_lds > 48u * 1024u) return hipErrorInvalidValue;
    WT_NS::wt_ao_args A = {};
    A.point = point; A.normal = normal; A.ids = ids; A.dirs = (const float4*)dirs; A.open = open;
    A.width = width; A.rows = rows; A.first_row = first_row; A.tiles_per_row = (unsigned)tpr; A.K = K; A.radius = radius;
    const dim3 g((unsigned)(tpr * trows)), block(WT_BLOCK);
    WT_LAUNCH_FLAVOUR(wt_ao_trace, /* no tail */, flags, g, block, dyn_lds, dyn_lds, dyn_lds, s, *P, A);      /* (the table in every flavour) */
    return hipGetLastError();
}

/* wt_ao_resolve over a width x rows range: one workgroup per tile of 32 x 8 pixels; ao_flags = CLW_AO_* bits (`frame` is read with COMPOSE only) */
WT_LAUNCHER(ao_resolve)(const unsigned char* open, const unsigned* ids, const unsigned* frame, unsigned* out, unsigned width,
                                           unsigned rows, unsigned ao_flags, unsigned K, unsigned strength, hipStream_t s) {
    const unsigned long long tpr = (width + (WT_AO_TILE_W - 1ull)) / WT_AO_TILE_W, trows = (rows + (WT_AO_TILE_H - 1ull)) / WT_AO_TILE_H;
    if (width == 0u || rows == 0u || (unsigned long long)width * rows >= (1ull << 30) || K < 1u || K > 32u || strength > 256u || (ao_flags & ~3u) ||
        !open || !ids || !out || ((ao_flags & WT_AO_COMPOSE) && !frame))
        return hipErrorInvalidValue;
    WT_NS::wt_ao_resolve_args A = {};
    A.open = open; A.ids = ids; A.frame = frame; A.out = out; A.width = width; A.rows = rows; A.tiles_per_row = (unsigned)tpr;
    A.K = K; A.strength = strength; A.compose = (ao_flags & WT_AO_COMPOSE) ? 1u : 0u;
    const dim3 g((unsigned)(tpr * trows)), block(WT_AO_TILE_W * WT_AO_TILE_H);
    if (ao_flags & WT_AO_FILTER) hipLaunchKernelGGL(WT_NS::wt_ao_resolve<true>, g, block, 0, s, A);
    else hipLaunchKernelGGL(WT_NS::wt_ao_resolve<false>, g, block, 0, s, A);
    return hipGetLastError();
}

/* ray queries (whitted_cast.inc): wt_cast over `n` rays (2 float4 each) on the device, geometry as the caller's plan chose it (launch_plan.c:
 * wt_plan_cast -- flags as the gbuffer launcher, `groups` workgroups of one wave serving `batches` batches of 64 rays each).  Exactly one of
 * `hits` (nearest: 2 float4 per ray) and `blocked` (any: a byte per ray) is given.  The caller has checked n and cast_flags (csrc/cast_host.h:
 * wt_cast_check) */
WT_LAUNCHER(cast)(const whitted_params* P, int flags, unsigned groups, unsigned batches, size_t dyn_lds, const void* rays,
                                     unsigned n, unsigned cast_flags, void* hits, unsigned char* blocked, hipStream_t s) {
    if (n == 0u || n >= (1u << 30) || !(cast_flags & 7u) || (cast_flags & ~15u) || !rays || (hits != nullptr) == (blocked != nullptr) || batches == 0u ||
        groups == 0u || (unsigned long long)groups * batches * 64ull < n || (unsigned long long)groups * batches * 64ull >= (1ull << 31) ||
        dyn_lds > 48u * 1024u)
        return hipErrorInvalidValue;
    WT_NS::wt_cast_args A = {};
    A.rays = (const float4*)rays; A.hits = (float4*)hits; A.blocked = blocked; A.n = n; A.flags = cast_flags; A.batches = batches;
    const dim3 g(groups), block(WT_BLOCK);
    if (hits) WT_LAUNCH_FLAVOUR(wt_cast, WT_TAIL(false), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    else WT_LAUNCH_FLAVOUR(wt_cast, WT_TAIL(true), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    return hipGetLastError();
}

/* layered ray queries (whitted_layers.inc): wt_cast_layers over `n` rays (2 float4 each) on the device, one workgroup of one wave per 64 rays,
 * geometry as the caller's plan chose it (launch_plan.c: wt_plan_cast -- flags as the gbuffer launcher).  `t` and `id` receive K * n words each,
 * layer-major.  `capacity`: the compiled list capacity to run, 4 or 8 (>= K), or 0 = the smallest that holds K.  The caller has checked n,
 * cast_flags and K (csrc/layers_host.h: wt_layers_check) */
WT_LAUNCHER(cast_layers)(const whitted_params* P, int flags, size_t dyn_lds, const void* rays, unsigned n, unsigned cast_flags, unsigned K,
                         unsigned capacity, float* t, unsigned* id, hipStream_t s) {
    if (capacity == 0u) capacity = K <= 4u ? 4u : 8u;
    if (n == 0u || n >= (1u << 30) || !(cast_flags & 7u) || (cast_flags & ~15u) || K == 0u || K > capacity || (capacity != 4u && capacity != 8u) || !rays ||
        !t || !id || dyn_lds > 48u * 1024u)
        return hipErrorInvalidValue;
    WT_NS::wt_layers_args A = {};
    A.rays = (const float4*)rays; A.t = t; A.id = id; A.n = n; A.flags = cast_flags; A.K = K;
    const dim3 g((n + 63u) / 64u), block(WT_BLOCK);
    if (capacity == 4u) WT_LAUNCH_FLAVOUR(wt_cast_layers, WT_TAIL(4), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    else WT_LAUNCH_FLAVOUR(wt_cast_layers, WT_TAIL(8), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    return hipGetLastError();
}

/* proximity queries (whitted_near.inc): wt_near over `n` probes (1 float4 each; `ignore` a word each, or null) on the device, one workgroup of
 * one wave per 64 probes, geometry as the caller's plan chose it (launch_plan.c: wt_plan_near -- flags as the gbuffer launcher, `box_cells` the
 * cap on a probe's box on the grid).  Exactly one output is given: `hits` (the nearest: 2 float4 per probe), `within` (a byte per probe), or
 * `d` and `id` together with K in 1..8 (K * n words each, layer-major; the list capacity run is the smallest of 4 and 8 that holds K).  The
 * caller has checked n, cast_flags and K (csrc/near_host.h: wt_near_check, wt_near_list_check) */
WT_LAUNCHER(near)(const whitted_params* P, int flags, size_t dyn_lds, unsigned box_cells, const void* probes, const unsigned* ignore, unsigned n,
                  unsigned cast_flags, unsigned K, void* hits, unsigned char* within, float* d, unsigned* id, hipStream_t s) {
    const int outputs = (hits != nullptr) + (within != nullptr) + (d != nullptr || id != nullptr);
    if (n == 0u || n >= (1u << 30) || !(cast_flags & 7u) || (cast_flags & ~15u) || !probes || outputs != 1 || ((d != nullptr) != (id != nullptr)) ||
        (d && (K == 0u || K > 8u)) || dyn_lds > 48u * 1024u)
        return hipErrorInvalidValue;
    WT_NS::wt_near_args A = {};
    A.probes = (const float4*)probes; A.ignore = ignore; A.hits = (float4*)hits; A.within = within; A.d = d; A.id = id;
    A.n = n; A.flags = cast_flags; A.K = K; A.box_cells = box_cells;
    const dim3 g((n + 63u) / 64u), block(WT_BLOCK);
    if (hits) WT_LAUNCH_FLAVOUR(wt_near, WT_TAIL(0), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    else if (within) WT_LAUNCH_FLAVOUR(wt_near, WT_TAIL(1), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    else if (K <= 4u) WT_LAUNCH_FLAVOUR(wt_near, WT_TAIL(4), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    else WT_LAUNCH_FLAVOUR(wt_near, WT_TAIL(8), flags, g, block, 0, dyn_lds, 0, s, *P, A);
    return hipGetLastError();
}

/* path queries (whitted_paths.inc): wt_cast_paths over `n` rays (2 float4 each) on the device, one workgroup of one wave per 64 rays, geometry
 * as the caller's plan chose it (launch_plan.c: wt_plan_cast -- flags as the gbuffer launcher); P carries the bound sphere and plane arrays
 * (spheres_raw, planes_raw) the materials are read from.  `hits` receives bounces * n records of 2 float4, segment-major, `status` n bytes,
 * `next` (may be null) n rays.  The caller has checked n, path_flags and bounces (csrc/paths_host.h: wt_paths_check) */
WT_LAUNCHER(cast_paths)(const whitted_params* P, int flags, size_t dyn_lds, const void* rays, unsigned n, unsigned path_flags, unsigned bounces,
                        void* hits, unsigned char* status, void* next, hipStream_t s) {
    if (n == 0u || n >= (1u << 30) || !(path_flags & 7u) || (path_flags & ~63u) || bounces == 0u || bounces > 8u || !rays || !hits || !status ||
        (P->ns > 0u && !P->spheres_raw) || (P->np > 0u && !P->planes_raw) || dyn_lds > 48u * 1024u)
        return hipErrorInvalidValue;
    WT_NS::wt_paths_args A = {};
    A.rays = (const float4*)rays; A.hits = (float4*)hits; A.status = status; A.next = (float4*)next; A.n = n; A.flags = path_flags; A.bounces = bounces;
    const dim3 g((n + 63u) / 64u), block(WT_BLOCK);
    WT_LAUNCH_FLAVOUR(wt_cast_paths, /* no tail */, flags, g, block, 0, dyn_lds, 0, s, *P, A);
    return hipGetLastError();
}

/* the launch camera's rays as query rays (whitted_layers.inc: wt_camera_rays): the `P->n_items` work-items of the linear range that starts at
 * global id `P->id_offset` of the camera `P` carries (wt_plan_fused_range), 2 float4 each into `rays`; `T` = the camera model (model 0: the
 * pinhole; the panorama's tables sized for the frame, as the raygen_proj launcher asks) */
WT_LAUNCHER(camera_rays)(const whitted_params* P, const wt_projection* T, void* rays, hipStream_t s) {
    const bool proj = T->model != CLW_PROJ_PERSPECTIVE;
    if (P->n_items == 0u || P->n_items >= (1u << 30) || P->width == 0u || P->band_stride > 1u || P->id_offset + P->n_items > (1ull << 32) || !rays ||
        (proj && T->model != CLW_PROJ_ORTHO && T->model != CLW_PROJ_EQUIRECT) ||
        (T->model == CLW_PROJ_EQUIRECT && (!T->col || !T->row || T->width != P->width || T->height != P->height)))
        return hipErrorInvalidValue;
    WT_NS::wt_camrays_args A = {};
    for (int a = 0; a < 3; a++) { A.corner[a] = P->corner[a]; A.right[a] = P->right[a]; A.up[a] = P->up[a]; A.origin[a] = P->origin[a]; }
    A.w_factor = P->w_factor; A.h_factor = P->h_factor; A.width = P->width; A.n = P->n_items; A.id_offset = P->id_offset; A.rays = (float4*)rays;
    const dim3 g((A.n + 255u) / 256u), block(256);
    if (proj) hipLaunchKernelGGL(WT_NS::wt_camera_rays<true>, g, block, 0, s, A, *T);
    else hipLaunchKernelGGL(WT_NS::wt_camera_rays<false>, g, block, 0, s, A, *T);
    return hipGetLastError();
}
