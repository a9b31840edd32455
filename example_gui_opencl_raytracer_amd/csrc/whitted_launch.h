/* whitted_launch.h -- THE prototypes of the C launchers the device units export (whitted_launch.inc) and the shim calls.  Each is written once,
 * here; a unit defines its copy as `WT_LAUNCHER(name)(parameters) { ... }`, so the compiler holds every definition against its declaration (C
 * linkage: another parameter list is a conflicting declaration, not an overload), and the shim picks the build's copy with WT_LAUNCH. */
#ifndef WHITTED_LAUNCH_H
#define WHITTED_LAUNCH_H
#include <hip/hip_runtime.h>
#include "projection_host.h"
#include "whitted_params.h"

/* in both units / in the fast unit only (integer work that serves both builds) */
#define WT_BOTH(ret, name, args) extern "C" ret wt_fast_##name args; extern "C" ret wt_strict_##name args;
#define WT_FAST_ONLY(ret, name, args) extern "C" ret wt_fast_##name args;

WT_BOTH(hipError_t, launch_trace, (const whitted_params* P, const unsigned char* tile_cull, int flags, unsigned grid, size_t dyn_lds, hipStream_t s))
WT_FAST_ONLY(hipError_t, launch_cull, (const whitted_params* P, unsigned parts, unsigned char* table, hipStream_t s))
WT_BOTH(int, has_trace, (int flags))
WT_BOTH(hipError_t, launch_raygen, (const raygen_params* P, hipStream_t s))
WT_BOTH(hipError_t, launch_raygen_proj, (const raygen_params* P, const wt_projection* T, hipStream_t s))
WT_BOTH(hipError_t, launch_sched, (const unsigned* cost, unsigned* order, unsigned tpr, unsigned trows, unsigned per_share, unsigned clamp_outliers,
                                   unsigned per_share_cap, unsigned split_slots, unsigned min_quota, unsigned max_lg, hipStream_t s))
WT_FAST_ONLY(hipError_t, launch_classify, (const unsigned* frame, unsigned width, unsigned rows, unsigned lgb, unsigned threshold, unsigned char* mask,
                                           unsigned* order, unsigned* count, unsigned cap, hipStream_t s))
WT_BOTH(hipError_t, launch_cams, (const wt_cam_table* T, float* dst, hipStream_t s))
WT_BOTH(hipError_t, launch_unit, (int op, const float* in, float* out, unsigned n, unsigned stride_in, unsigned stride_out, unsigned aux, hipStream_t s))
WT_BOTH(hipError_t, launch_unit_scene, (const whitted_params* P, int flags, int op, const float* in, float* out, unsigned n, unsigned stride_in,
                                        unsigned stride_out, size_t dyn_lds, hipStream_t s))
WT_BOTH(hipError_t, launch_gbuffer, (const whitted_params* P, int flags, unsigned grid, size_t dyn_lds, float* depth, unsigned* id, float* normal,
                                     float* point, float* albedo, const wt_projection* T, hipStream_t s))
WT_BOTH(hipError_t, launch_overlay, (const unsigned* frame, const unsigned* ids, unsigned* out, unsigned width, unsigned rows, unsigned flags,
                                     const unsigned style[5], const unsigned* sel, unsigned count, hipStream_t s))
WT_BOTH(hipError_t, launch_objects, (const unsigned* ids, const unsigned* depth, unsigned width, unsigned rows, unsigned first_row,
                                     const unsigned clip[4], const unsigned counts[3], void* table, void* result, hipStream_t s))
WT_BOTH(hipError_t, launch_ao_trace, (const whitted_params* P, int flags, const float* point, const float* normal, const unsigned* ids,
                                      const float* dirs, unsigned char* open, unsigned width, unsigned rows, unsigned first_row, unsigned K,
                                      float radius, hipStream_t s))
WT_BOTH(hipError_t, launch_ao_resolve, (const unsigned char* open, const unsigned* ids, const unsigned* frame, unsigned* out, unsigned width,
                                        unsigned rows, unsigned ao_flags, unsigned K, unsigned strength, hipStream_t s))
WT_BOTH(hipError_t, launch_cast, (const whitted_params* P, int flags, unsigned groups, unsigned batches, size_t dyn_lds, const void* rays, unsigned n,
                                  unsigned cast_flags, void* hits, unsigned char* blocked, hipStream_t s))
WT_BOTH(hipError_t, launch_cast_layers, (const whitted_params* P, int flags, size_t dyn_lds, const void* rays, unsigned n, unsigned cast_flags, unsigned K,
                                         unsigned capacity, float* t, unsigned* id, hipStream_t s))
WT_BOTH(hipError_t, launch_near, (const whitted_params* P, int flags, size_t dyn_lds, unsigned box_cells, const void* probes, const unsigned* ignore,
                                  unsigned n, unsigned cast_flags, unsigned K, void* hits, unsigned char* within, float* d, unsigned* id, hipStream_t s))
WT_BOTH(hipError_t, launch_cast_paths, (const whitted_params* P, int flags, size_t dyn_lds, const void* rays, unsigned n, unsigned path_flags,
                                        unsigned bounces, void* hits, unsigned char* status, void* next, hipStream_t s))
WT_BOTH(hipError_t, launch_camera_rays, (const whitted_params* P, const wt_projection* T, void* rays, hipStream_t s))
#undef WT_BOTH
#undef WT_FAST_ONLY

#ifdef WT_STRICT      /* a device unit.  Its definition of a launcher: WT_LAUNCHER(trace)(the parameters above) { ... } */
#if WT_STRICT
#define WT_NAME(name) wt_strict_##name
#else
#define WT_NAME(name) wt_fast_##name
#endif
#define WT_LAUNCHER(name) extern "C" hipError_t WT_NAME(launch_##name)
#else                 /* the shim.  The build in use launches its own copy: WT_LAUNCH(I, trace)(arguments) */
#define WT_LAUNCH(I, name) ((I)->strict ? wt_strict_launch_##name : wt_fast_launch_##name)
#endif
#endif
