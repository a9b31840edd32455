/*
 * hip_wrap_impl.h -- what the translation units of the C-ABI shim share: the wrapper's state (Impl, Buffer, Kernel), the failure convention
 * (die, HIP_OK), the launch helpers (LaunchTimer, finish, use_device, impl_of), the scoped device temporary of the unit entry points and the
 * scene side of a launch (prepare_scene, bind_scene, bind_geometry, find_rays, resolve_projection).  hip_wrap.cpp: the reference's entry
 * points, the trace path and the knobs; hip_wrap_passes.cpp: the passes beside the trace launch.
 */
#ifndef HIP_WRAP_IMPL_H
#define HIP_WRAP_IMPL_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hip_wrap_ext.h"
#include "ao_host.h"
#include "cast_host.h"
#include "layers_host.h"
#include "near_host.h"
#include "paths_host.h"
#include "launch_plan.h"
#include "objects_host.h"
#include "overlay_host.h"
#include "png_codec.h"
#include "bounce_cull_host.h"
#include "primary_cull_host.h"
#include "projection_host.h"
#include "scene_prep.h"
#include "whitted_launch.h"
#include "whitted_params.h"

namespace clw {

[[noreturn]] void die(const char* fmt, ...);      /* prints "ERROR:\t<message>" on stdout and calls exit(1) */

#define HIP_OK(call, what)                                                        \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) die("%s (%s)", what, hipGetErrorString(e_));        \
    } while (0)

enum KernelKind { K_RAYGEN = 0, K_RAYTRACER = 1 };

typedef wt_raygen RaygenArgs;   /* snapshot of the eight by-value raygen arguments + the launch range (launch_plan.h) */

struct Buffer {
    void* dptr = nullptr;
    size_t size = 0;
    bool owned = true;       /* freed by release */
    bool lazy = false;       /* created with data == NULL: allocated on first real use */
    bool image = false;
    uint32_t w = 0, h = 0, layers = 0;
    std::vector<uint8_t> shadow;   /* host copy of uploaded data (scene arrays are re-read by scene prep) */
    bool gen_valid = false;        /* holds rays "generated" by a fused raygen launch */
    bool exposed = false;          /* its device pointer was handed out (clw_ext_device_ptr) since the rays were generated: a caller may have
                                      rewritten them in place, so they are no longer known to be this library's own unit vectors */
    bool gen_materialised = false;
    RaygenArgs gen{};
    clw_projection gen_proj{};     /* the camera model the materialised rays were generated with (all zero = the pinhole) */
};

struct ArgValue {
    bool set = false;
    size_t size = 0;
    uint8_t bytes[32] = {0};
};

struct Kernel {
    KernelKind kind;
    std::string name;
    ArgValue values[__MAX_BUFFERS];
};

struct TimingEntry { hipEvent_t start, stop; cl_uint kernel; };

/* A device staging buffer that only grows: freed and allocated again when a call needs more than it holds, kept otherwise.  Its owner's calls
 * wait for their own work, so nothing is in flight on it when it is replaced. */
struct DeviceGrow {
    void* p = nullptr;
    size_t cap = 0;                 /* bytes p holds */
    void* reserve(size_t bytes) {
        if (cap < bytes) {
            release();
            HIP_OK(hipMalloc(&p, bytes), "Couldn't allocate device memory");
            cap = bytes;
        }
        return p;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Impl {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::vector<Kernel> kernels;
    std::vector<Buffer*> live;      /* every buffer handed out as a cl_mem handle */
    /* knobs */
    int depth = 15;
    int strict = 0;
    int fuse = 1;
    int async = 0;
    int variant = 0;
    int last_trace_flags = -1;    /* the kernel flavour (WT_F_* flags) of the latest trace launch; -1 = none yet */
    int counting = 0;
    float through = 0.8f;  /* primitives.cl:7 TRANSPERENT_THROUGH; CLWRAP_THROUGH / clw_ext_set_shadow_through */
    int stamps = 0;        /* CLWRAP_STAMPS=1: hand the counter block to the (diagnostic) stamp build of the kernel */
    uint64_t id_offset = 0;
    uint32_t band_stride = 1, band_phase = 0;
    int supersample = 1;   /* n x n samples per pixel, resolved in the trace kernel (clw_ext_set_supersample / CLWRAP_SUPERSAMPLE): 1, 2, 4 or 8 */
    float* debug_rgb = nullptr;
    /* adaptive supersampling (clw_ext_set_adaptive / CLWRAP_ADAPTIVE): a trace launch becomes a 1-sample base pass, the classifier
     * (wt_refine_classify) and a supersampled pass over the blocks it listed, all three on the launch stream and none waited for.  The
     * buffers follow the launch range and the factor; a change of stream fences them like the camera table (tables_fence). */
    int adaptive = -1;            /* contrast threshold, 0..256; -1 = off */
    struct Adaptive {
        uint8_t* mask = nullptr; uint32_t* order = nullptr; uint32_t* count = nullptr;
        uint32_t w = 0, rows = 0; int ss = 0;     /* output pixels of the range the buffers were sized for, and the factor */
        uint32_t blocks = 0;                      /* blocks of the LAST trace launch when it was adaptive, else 0 (clw_ext_read_refine_mask) */
        void free_all() {
            for (void* q : {(void*)mask, (void*)order, (void*)count}) if (q) (void)hipFree(q);
            mask = nullptr; order = nullptr; count = nullptr; w = rows = 0; ss = 0;
        }
    } adapt;
    /* per-sample cameras of supersampled launches (clw_ext_set_sample_cameras / clw_ext_set_lens: alternatives, the later call clears the
     * other).  The device copy is laid out per lane of a tile's wavefront (whitted_params.h: ss_cams) and is rewritten, only when it changed,
     * by a small kernel on the launch stream that carries the table as its argument: stream order keeps it behind every queued launch that
     * reads the previous table, and no host memory has to outlive the call.  A change of stream (clw_ext_set_stream) records tables_fence on
     * the old stream, which the next launch with a table waits for on the new one. */
    std::vector<clw_sample_camera> cams;         /* the explicit table, sy * n + sx order; empty = none */
    float aperture = 0.0f, focus = 1.0f;         /* thin lens: the table is derived at every launch from the latched camera; aperture 0 = pinhole */
    std::vector<clw_sample_camera> cams_used;    /* the table of the latest trace launch (clw_ext_get_sample_cameras) */
    float* d_cams = nullptr;
    wt_cam_table cams_dev{}; bool cams_dev_valid = false;   /* what d_cams holds once the stream gets there */
    hipEvent_t tables_fence = nullptr; bool tables_fence_pending = false, tables_in_flight = false;   /* one fence for every device table written and read in stream order: sample cameras, moving spheres, an adaptive launch's mask / list / counters */
    /* moving spheres of supersampled launches (clw_ext_set_sphere_motion).  The device copy -- 64 per-lane times, then a float4 per sphere
     * (whitted_params.h: ss_times, ss_disp) -- is written like the camera table: only when it changed, in pieces of one wt_cam_table by the
     * same small kernel on the launch stream, and behind the same fence when the stream changes. */
    std::vector<float> motion_disp;              /* 3 per sphere; empty = the scene stands still (an all-zero table is stored as none) */
    std::vector<float> motion_times;             /* explicit sample times, sy * n + sx order (only when motion_explicit_times) */
    bool motion_explicit_times = false;          /* the caller gave times (of any count: the launch checks it); false = the shutter times of the launch's factor */
    std::vector<float> times_used;               /* the times of the latest trace launch (clw_ext_get_sample_times) */
    float* d_motion = nullptr;
    std::vector<float> motion_dev;               /* what d_motion holds once the stream gets there; empty = nothing yet */
    /* the seed offset of every trace launch (clw_ext_set_seed_offset / CLWRAP_SEED_OFFSET): a work-item's xorshift state starts at id + seed_offset */
    uint32_t seed_offset = 0;
    /* progressive frame accumulation (clw_ext_set_accumulate / CLWRAP_ACCUMULATE, CLWRAP_ACC_JITTER): frame f = K of a still view is traced with
     * seed offset seed_offset + clw_host_frame_seed(f) through clw_host_jitter_camera(latched camera, f, n) and folded into `sum` by the trace
     * kernel's epilogue (whitted_params.h: acc_sum); the key is everything that defines the image -- a launch whose key differs from the previous
     * one's starts again at frame 0.  `sum` follows the launch range and is fenced across a change of stream like the tables (tables_fence). */
    int acc_max = 0, acc_jitter = 1;          /* frames a still view accumulates (0 = the mode is off); per-frame sub-pixel offset on / off */
    struct AccKey {
        RaygenArgs gen{}; uint64_t n_out = 0; uint32_t total = 0;
        int depth = 0, strict = 0, fuse = 0, ss = 0, max_frames = 0, jitter = 0;
        float through = 0.0f; uint32_t seed = 0;
        const Buffer* buf[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   /* rays, spheres, planes, lights, textures, skybox, framebuffer */
        const void* dptr[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; size_t size[7] = {0, 0, 0, 0, 0, 0, 0};
        uint32_t counts[3] = {0, 0, 0}, img[5] = {0, 0, 0, 0, 0};
        uint64_t epoch = 0;
    };
    struct Accum {
        float* sum = nullptr; size_t pixels = 0;      /* 3 floats per output pixel of the launch range */
        uint32_t K = 0;                               /* frames in the sum */
        int frame = -1;                               /* the frame the trace launch under way folds in; -1 = not an accumulated launch */
        uint64_t epoch = 0;                           /* bumped by whatever changes the image behind the key's back (uploads, invalidate, reset) */
        bool key_valid = false; AccKey key;
    } acc;
    /* the camera model beside the pinhole (clw_ext_set_projection / CLWRAP_PROJECTION; whitted_projection.inc): model 0 = none.  The two tables
     * of a panorama (width and height float4) are the wrapper's: `tab_col` / `tab_row` are what the device copies hold, and they are written
     * again -- behind a wait for the launches that read them -- only when a launch resolves to other values. */
    clw_projection proj{};
    struct ProjTables {
        float* d_col = nullptr; float* d_row = nullptr;
        uint32_t cap_w = 0, cap_h = 0;               /* float4s the device buffers hold */
        std::vector<float> tab_col, tab_row;         /* the tables on the device (4 floats per column / row) */
        void free_all() { if (d_col) (void)hipFree(d_col); if (d_row) (void)hipFree(d_row); d_col = d_row = nullptr; cap_w = cap_h = 0; tab_col.clear(); tab_row.clear(); }
    } ptab;
    /* What the passes that leave range-sized results on the device share (range_resize, range_mark_done, range_read below): `done` is recorded
     * behind every pass on the stream it ran on, so a read-back waits for the pass whatever the launch stream is by then */
    struct RangePass {
        uint32_t n = 0;                 /* work-items the buffers are sized for */
        uint32_t written = 0;           /* what the last pass left to read: the G-buffer's channels, else 1 */
        hipEvent_t done = nullptr;
        void drop_done() { if (done) (void)hipEventDestroy(done); done = nullptr; }
    };
    /* the primary-hit pass (clw_ext_render_gbuffer / clw_ext_pick; whitted_gbuffer.inc): planar channel buffers indexed like the framebuffer, one per
     * CLW_GB_* bit, allocated when a pass first asks for them and sized for the pass's range */
    struct GBuffer : RangePass {
        void* chan[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   /* depth, id, normal, point, albedo */
        uint32_t* pick = nullptr;       /* the 11 words of one clw_pick: a pick is the pass on a one-pixel range, its channels laid out as the struct */
        void alloc_buffers(uint32_t) {}      /* (per channel, when a pass first asks for it) */
        void free_buffers() { for (void*& q : chan) { if (q) (void)hipFree(q); q = nullptr; } n = 0; written = 0; }
        void release() { free_buffers(); if (pick) (void)hipFree(pick); pick = nullptr; drop_done(); }
    } gb;
    /* the selection overlay (clw_ext_render_overlay; whitted_overlay.inc): its own id buffer -- the primary-hit pass writes it, `gb` is not touched --
     * and the composed frame, both sized for the pass's range */
    struct Overlay : RangePass {
        uint32_t* ids = nullptr; uint32_t* frame = nullptr;
        void alloc_buffers(uint32_t items) {
            HIP_OK(hipMalloc((void**)&ids, (size_t)items * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&frame, (size_t)items * 4), "Couldn't allocate device memory");
        }
        void free_buffers() { if (ids) (void)hipFree(ids); if (frame) (void)hipFree(frame); ids = frame = nullptr; n = 0; written = 0; }
        void release() { free_buffers(); drop_done(); }
    } ov;
    /* the visible-object table (clw_ext_object_stats; whitted_objects.inc): its own id and depth buffers -- the primary-hit pass writes them, `gb`
     * and `ov` are not touched -- sized for the pass's range, and the slot table (16 bytes of counters + 48 per slot) and the result (the 16-byte
     * summary + room for a 48-byte record per slot), sized for the scene's counts.  Every call waits for its own work, so nothing is ever in flight
     * on these buffers between calls: no `done`. */
    struct Objects {
        uint32_t* ids = nullptr; float* depth = nullptr;
        uint32_t n = 0;                 /* work-items ids and depth are sized for */
        void* table = nullptr; void* result = nullptr;
        uint32_t slots = 0;             /* slots table and result are sized for */
        void alloc_buffers(uint32_t items) {
            HIP_OK(hipMalloc((void**)&ids, (size_t)items * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&depth, (size_t)items * 4), "Couldn't allocate device memory");
        }
        void free_buffers() { if (ids) (void)hipFree(ids); if (depth) (void)hipFree(depth); ids = nullptr; depth = nullptr; n = 0; }
        void size_table(uint32_t count) {
            if (slots == count) return;
            free_table();
            HIP_OK(hipMalloc(&table, 16 + (size_t)count * sizeof(clw_object_stat)), "Couldn't allocate device memory");
            HIP_OK(hipMalloc(&result, sizeof(clw_object_summary) + (size_t)count * sizeof(clw_object_stat)), "Couldn't allocate device memory");
            slots = count;
        }
        void free_table() { if (table) (void)hipFree(table); if (result) (void)hipFree(result); table = result = nullptr; slots = 0; }
        void release() { free_buffers(); free_table(); }
    } obj;
    /* ambient occlusion (clw_ext_render_ao; whitted_ao.inc): its own point, normal and id buffers -- the primary-hit pass writes them, `gb`, `ov`
     * and `obj` are not touched --, the open-ray counts and the resolved frame, all sized for the pass's range.  The direction table (16 x K
     * float4, room for K = 32) is written only when K changes, behind a wait for the passes that read the old one. */
    struct AO : RangePass {
        float* point = nullptr; float* normal = nullptr; uint32_t* ids = nullptr; uint8_t* open = nullptr; uint32_t* frame = nullptr;
        float* dirs = nullptr; uint32_t dirs_K = 0;      /* the table on the device and the K it was built for (0 = none yet) */
        void alloc_buffers(uint32_t items) {
            HIP_OK(hipMalloc((void**)&point, (size_t)items * 12), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&normal, (size_t)items * 12), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&ids, (size_t)items * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&open, (size_t)items), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&frame, (size_t)items * 4), "Couldn't allocate device memory");
        }
        void free_buffers() {
            for (void* q : {(void*)point, (void*)normal, (void*)ids, (void*)open, (void*)frame}) if (q) (void)hipFree(q);
            point = normal = nullptr; ids = nullptr; open = nullptr; frame = nullptr; n = 0; written = 0;
        }
        void release() { free_buffers(); if (dirs) (void)hipFree(dirs); dirs = nullptr; drop_done(); }
    } ao;
    /* ray queries (clw_ext_cast_rays / clw_ext_occluded_rays; whitted_cast.inc): the buffers of the host-array entry points -- the rays as uploaded,
     * the hits, the blocked bytes -- each grown to the largest n so far (DeviceGrow).  Those calls wait for their own work, so nothing is in flight on them between
     * calls; clw_ext_cast_rays_device works on the caller's memory and owns nothing. */
    struct Cast {
        DeviceGrow rays, hits, blocked;
        void free_buffers() { rays.release(); hits.release(); blocked.release(); }
    } cast;
    /* layered ray queries (clw_ext_cast_layers / clw_ext_render_layers / clw_ext_pick_layers / clw_ext_camera_rays; whitted_layers.inc).  The
     * range part -- the camera rays of a render_layers and its K planar layers of t and id, sized for the pass's range and its K -- is read back
     * like every range pass (`done`).  The host-array entry points have buffers of their own, grown to the largest n and K * n so far (DeviceGrow); those
     * calls wait for their own work.  A pick is both kernels on a one-pixel range into `pick`: the ray, then 8 t and 8 id words.  The device
     * entry points work on the caller's memory and own nothing. */
    struct Layers : RangePass {
        void* rays = nullptr; float* t = nullptr; uint32_t* id = nullptr;
        uint32_t K = 0;                 /* layers the range buffers hold per work-item */
        DeviceGrow h_rays, h_t, h_id;   /* (h_rays also holds the camera rays of clw_ext_camera_rays) */
        uint32_t* pick = nullptr;
        void free_range() {
            for (void* q : {rays, (void*)t, (void*)id}) if (q) (void)hipFree(q);
            rays = nullptr; t = nullptr; id = nullptr; n = 0; K = 0; written = 0;
        }
        void release() { free_range(); h_rays.release(); h_t.release(); h_id.release(); if (pick) (void)hipFree(pick); pick = nullptr; drop_done(); }
    } layers;
    /* path queries (clw_ext_cast_paths / clw_ext_pick_path; whitted_paths.inc): the buffers of the host-array entry point -- the rays as uploaded,
     * the hits, the status bytes, the outgoing rays -- each grown to the largest size so far (DeviceGrow); that call waits for its own work.  A
     * pick is the camera-ray kernel and the path kernel on a one-pixel range into `pick`: the ray, then 8 hits, the outgoing ray and the status
     * byte's word.  The device entry point works on the caller's memory and owns nothing. */
    struct Paths {
        DeviceGrow rays, hits, status, next;
        uint32_t* pick = nullptr;
        void release() { rays.release(); hits.release(); status.release(); next.release(); if (pick) (void)hipFree(pick); pick = nullptr; }
    } paths;
    /* proximity queries (clw_ext_nearest_surface / clw_ext_within_reach / clw_ext_near_surfaces; whitted_near.inc): the buffers of the host-array
     * entry points -- the probes and the ignore words as uploaded, the hits or the within bytes, the K planar layers of d and id -- each grown to
     * the largest size so far (DeviceGrow); those calls wait for their own work.  The device entry points work on the caller's memory and own
     * nothing. */
    struct Near {
        DeviceGrow probes, ignore, out, d, id;
        void release() { probes.release(); ignore.release(); out.release(); d.release(); id.release(); }
    } near;
    /* prepared scene cache */
    const Buffer *prep_s = nullptr, *prep_p = nullptr, *prep_l = nullptr;
    uint32_t prep_ns = 0, prep_np = 0, prep_nl = 0;
    float* d_geom = nullptr; size_t geom_f4 = 0;
    float* d_ptex = nullptr;
    bool have_lpt = false;    /* the light / plane side table follows the lights in d_geom */
    uint64_t scene_generation = 0;   /* bumped every time the prepared scene is rebuilt (device pointers can be reused) */
    uint32_t *d_grid_start = nullptr, *d_grid_items = nullptr, *d_grid_box = nullptr;
    float* d_grid_geom = nullptr;
    wprep_grid grid{}; bool grid_ok = false, grid_pair = false, near_grid_ok = false; int use_grid = 1;
    size_t grid_pairs = 0;                       /* cell-list entries of the grid built (clw_ext_get_grid) */
    int grid_pair_req = -1;                      /* clw_ext_set_grid_pair: -1 = env CLWRAP_GRID_PAIR (default on), 0 / 1 */
    unsigned long long* d_counters = nullptr;
    /* cost-sorted tile dispatch: costs written by frame n order the tiles of frame n+1 */
    int sched = 1;
    /* Double-buffered: trace k writes its tile costs into cost[k & 1]; when the camera / depth / scene changed, the
     * order for those costs is built on a SIDE stream behind trace k (order[k & 1], 15 us, 8 workgroups) while trace
     * k+1 already runs with the order built two frames earlier -- so a moving camera (the interactive loop of
     * rayinteractive.c:183-197) never waits for the sort.  Any order built for the same tile grid is a valid
     * permutation, so a stale one only costs balance, never pixels. */
    struct Sched {
        unsigned* cost[2] = {nullptr, nullptr}; unsigned* order[2] = {nullptr, nullptr};
        hipEvent_t built[2] = {nullptr, nullptr};    /* order[i] complete (recorded on the sched stream) */
        wt_order_state o{};                           /* which order holds a schedule, which cost buffer the next trace writes, what the newest order was
                                                         built for and how long ago: plain words, stepped by wt_order_* (launch_plan.c) */
        hipEvent_t traced = nullptr;
        uint32_t w = 0, rows = 0, cap = 0;           /* frame the buffers were sized for (the virtual frame of a supersampled launch); dispatch entries per XCD share */
        int ss = 1;                                   /* supersampling factor its orders were built for: it caps how far a tile is split */
        int last_rd = -1;                             /* order[] the last tiled launch read; -1 = it ran in the default order (clw_ext_read_tile_order) */
        /* the signature the newest order was built for: camera, depth, scene, and the sample cameras and moving spheres' device tables (empty = none) */
        RaygenArgs sig{}; int sig_depth = 0; uint64_t sig_scene = 0;
        wt_cam_table sig_cams{}; bool sig_has_cams = false;
        std::vector<float> sig_motion;
        void reset() { o.have[0] = o.have[1] = 0; o.sig_valid = 0; o.newest = 0; last_rd = -1; }
        void free_all() {
            for (int i = 0; i < 2; i++) {
                if (cost[i]) (void)hipFree(cost[i]);
                if (order[i]) (void)hipFree(order[i]);
                if (built[i]) (void)hipEventDestroy(built[i]);
                cost[i] = order[i] = nullptr; built[i] = nullptr;
            }
            if (traced) { (void)hipEventDestroy(traced); traced = nullptr; }
            reset();
        }
    };
    hipStream_t sched_stream = nullptr;
    static constexpr int MAX_CHUNKS = 4;
    Sched scheds[1 + MAX_CHUNKS];   /* [0]: whole-range launches; [1 + c]: strip c of a pipelined read-back */
    /* The primary-ray cull table (primary_cull_host.h; launch_plan.h: wt_plan_cull), one per scheduling slot: built on the launch stream ahead of
     * the trace that reads it, and only when its key -- the camera terms, frame width and row range, and the prepared scene -- changed and has
     * now come twice in a row, so a still view pays for it once and a camera that moves every frame never.  It is written and read in stream
     * order (the tables fence covers a change of stream). */
    struct Cull {
        unsigned char* table = nullptr; size_t bytes = 0;   /* two bytes per tile (primary, bounce: bounce_cull_host.h), rounded up to whole words */
        bool valid = false;                                  /* `table` holds the table of `view`, `scene`, `depth` and `parts` */
        wt_cull_view view{}; uint64_t scene = 0;
        uint32_t tiles = 0;
        int32_t depth = 0; uint32_t parts = 0;               /* what the bounce bytes were built for: the launch depth, WT_BC_PART_* */
        bool seen = false;                                   /* the key of the slot's last launch that could read a table: a view is built for when it comes twice in a row */
        wt_cull_view seen_view{}; uint64_t seen_scene = 0; uint32_t seen_tiles = 0;
        uint64_t builds = 0;                                 /* builder launches so far (clw_ext_read_primary_cull) */
        bool last_used = false;                              /* the slot's last trace launch was given the table */
        void free_all() { if (table) (void)hipFree(table); table = nullptr; bytes = 0; valid = false; last_used = false; tiles = 0; }
    };
    Cull culls[1 + MAX_CHUNKS];
    uint32_t bounce_parts = WT_BC_PART_SHADOW | WT_BC_PART_REFL;   /* CLWRAP_BOUNCE_CULL, clw_ext_set_bounce_cull: the parts of the bounce byte that tables carry */
    /* pipelined read-back (cl_wrap_output of a large frame): strips rendered back to back, each copied to the host
     * while the next one renders */
    int pipeline = 1;
    hipStream_t copy_stream = nullptr;
    hipEvent_t chunk_done[MAX_CHUNKS] = {nullptr, nullptr, nullptr, nullptr};
    /* timing log */
    std::vector<TimingEntry> timing;
    unsigned occ_tiles_per_depth = WT_OCC_TILES_PER_DEPTH;   /* CLWRAP_OCC_TILES_PER_DEPTH: tuning knob */
    /* the tree-parallel tail of deep launches (whitted_tpt.inc): one slice of node storage per workgroup of the launch */
    uint32_t* d_tpt_pool = nullptr; uint32_t* d_tpt_flags = nullptr; size_t tpt_pool_bytes = 0;
    uint32_t* d_tpt_jump = nullptr;              /* 7 x 32 words: M^(2^i), M = one hit's worth of xorshift steps (xorshift_jump_matrices) */
    unsigned tpt_max = WT_TPT_MAX_LANES, tpt_min = WT_TPT_MIN_PATHS, tpt_pool_mb = WT_TPT_POOL_MB;   /* CLWRAP_TPT_MAX / _MIN / _POOL_MB, clw_ext_set_tpt */
    int tpt_clock = 0;                                    /* CLWRAP_TPT_CLOCK=1: DIAGNOSTIC phase clock of the tail (counter words 10-25) */
    unsigned split_slots = WT_SPLIT_SLOTS;                   /* CLWRAP_SPLIT_SLOTS: the quota is a share's total cost over this many wavefronts */
    unsigned split_min_quota = WT_SPLIT_MIN_QUOTA;           /* CLWRAP_SPLIT_MIN_QUOTA; 0 = heavy tiles are not split */
    bool timing_on = false;                       /* switched on by the first clw_ext_timing_reset / set_timing_every */
    uint32_t timing_every = 1, timing_tick = 0;   /* events around every n-th launch only */
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
};

inline Impl* impl_of(const cl_wrap* w) {
    if (!w || !w->impl) die("cl_wrap is not initialised");
    return (Impl*)w->impl;
}

inline void use_device(Impl* I) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != I->device) HIP_OK(hipSetDevice(I->device), "Cannot select the HIP device");
}

inline bool is_registered(const cl_wrap* w, cl_uint kernel_id, cl_uint arg_id) {
    for (cl_uint i = 0; i < w->buffers_num[kernel_id]; i++)
        if (w->buffers_ids[kernel_id][i] == arg_id) return true;
    return false;
}

inline Buffer* lookup_handle(Impl* I, const void* handle) {
    for (Buffer* b : I->live)
        if ((const void*)b == handle) return b;
    return nullptr;
}

inline void ensure_allocated(Impl* I, Buffer* b) {
    (void)I;
    if (b->dptr || b->size == 0) return;
    HIP_OK(hipMalloc(&b->dptr, b->size), "Couldn't allocate device memory");
    b->lazy = false;
}

/* ---- launch helpers -------------------------------------------------------------------- */
inline std::pair<hipEvent_t, hipEvent_t> take_events(Impl* I) {
    if (!I->free_events.empty()) {
        auto p = I->free_events.back();
        I->free_events.pop_back();
        return p;
    }
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a), "Couldn't create a timing event");
    HIP_OK(hipEventCreate(&b), "Couldn't create a timing event");
    return {a, b};
}

struct LaunchTimer {
    Impl* I; cl_uint kernel; bool on; std::pair<hipEvent_t, hipEvent_t> ev;
    LaunchTimer(Impl* I_, cl_uint k, bool wanted = true) : I(I_), kernel(k), on(wanted && I_->timing_on && I_->timing.size() < 16384 && (I_->timing_tick++ % I_->timing_every) == 0) {
        if (on) { ev = take_events(I); HIP_OK(hipEventRecord(ev.first, I->stream), "Couldn't run the kernel"); }
    }
    void done() {
        if (on) { HIP_OK(hipEventRecord(ev.second, I->stream), "Couldn't run the kernel"); I->timing.push_back({ev.first, ev.second, kernel}); }
    }
};

inline void finish(Impl* I) {
    hipError_t e = hipStreamSynchronize(I->stream);
    if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
}

/* A device temporary of a unit entry point: allocated -- and, given a host array, filled from it -- here, freed when it goes out of scope.  A
 * null optional input stays a null device pointer. */
template <class T> struct DeviceTemp {
    T* p = nullptr;
    explicit DeviceTemp(size_t bytes) { HIP_OK(hipMalloc((void**)&p, bytes), "Couldn't allocate device memory"); }
    DeviceTemp(const void* host, size_t bytes) {
        if (!host) return;
        HIP_OK(hipMalloc((void**)&p, bytes), "Couldn't allocate device memory");
        HIP_OK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    }
    ~DeviceTemp() { if (p) (void)hipFree(p); }
    DeviceTemp(const DeviceTemp&) = delete;
    DeviceTemp& operator=(const DeviceTemp&) = delete;
    void read(void* host, size_t bytes) const { HIP_OK(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost), "Failed to transfer device memory to host"); }
    operator T*() const { return p; }
};

inline uint32_t read_count(const Kernel& k, cl_uint arg) {
    const ArgValue& v = k.values[arg];
    if (!v.set) die("Couldn't run the kernel");
    switch (v.size) { /* uchar in the reference (raytracing.cl:17); 2/4 bytes = wide-count extension */
        case 1: return v.bytes[0];
        case 2: { uint16_t x; memcpy(&x, v.bytes, 2); return x; }
        case 4: { uint32_t x; memcpy(&x, v.bytes, 4); return x; }
        default: die("Couldn't run the kernel");
    }
}

inline int env_int(const char* name, int dflt) {
    const char* s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}

/* arg 0 of the raytracer: the ray buffer, passed by value as the 8 bytes of a handle (raypng.c:61) or bound as a buffer; null = neither */
inline Buffer* find_rays(const cl_wrap* w, Impl* I, cl_uint kid) {
    if (is_registered(w, kid, 0)) return (Buffer*)w->buffers[kid][0];
    const ArgValue& v = I->kernels[kid].values[0];
    if (!v.set || v.size != sizeof(cl_mem)) return nullptr;
    void* h; memcpy(&h, v.bytes, sizeof h);
    return lookup_handle(I, h);
}

/* arg 7 of the raytracer: the guard `total_size` (raytracing.cl:24) */
inline bool find_total(const Kernel& k, uint32_t& total) {
    if (!k.values[7].set || k.values[7].size != 4) return false;
    memcpy(&total, k.values[7].bytes, 4);
    return true;
}

/* The prepared geometry (prepare_scene) as a launch sees it: the scene words, the prepared arrays and -- for a launch over the uniform grid
 * (flags: WT_F_GRID) -- the grid.  The one place that knows these fields: every launch over a bound scene and the ray queries come here. */
inline void bind_geometry(const Impl* I, whitted_params& P, int flags) {
    P.ns = I->prep_ns; P.np = I->prep_np; P.nl = I->prep_nl; P.geom_f4 = (uint32_t)I->geom_f4;
    P.geom = I->d_geom; P.ptex = I->d_ptex;
    if (flags & WT_F_GRID) {
        P.grid_pair = I->grid_pair ? 1u : 0u;
        P.grid_start = I->d_grid_start; P.grid_items = I->d_grid_items; P.grid_box = I->d_grid_box; P.grid_geom = I->d_grid_geom;
        for (int a = 0; a < 3; a++) {
            P.grid_min[a] = I->grid.gmin[a]; P.grid_inv[a] = I->grid.inv[a]; P.grid_cell[a] = I->grid.cell[a]; P.grid_res[a] = I->grid.res[a];
        }
    }
}

/* defined in hip_wrap.cpp */
bool resolve_projection(Impl* I, const RaygenArgs& g, wt_projection& T);
void prepare_scene(Impl* I, Buffer* s, uint32_t ns, Buffer* p, uint32_t np, Buffer* l, uint32_t nl);
void bind_scene(cl_wrap* w, Impl* I, cl_uint kid, whitted_params& P, int& flags, size_t& dyn_lds);

} /* namespace clw */
#endif
