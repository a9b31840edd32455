/*
 * hip_wrap.cpp -- the C-ABI shim: the reference's six cl_wrap_* entry points
 * (reference src/opencl_wrap.h:29-42, src/opencl_wrap.c:11-416) implemented over the HIP
 * runtime and the precompiled gfx950 kernels of whitted_{fast,strict}.hip, plus the
 * extension entry points of include/hip_wrap_ext.h.
 *
 * Same conventions as the reference: every failure prints "ERROR:\t<message>" on stdout
 * and calls exit(1); every call returns with its work complete (unless the caller opted
 * into async mode); single host thread.
 *
 * There is NO CPU fallback: without a HIP device cl_wrap_init fails exactly as the
 * reference fails without an OpenCL GPU (opencl_wrap.c:31-34).
 */
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
#include "launch_plan.h"
#include "objects_host.h"
#include "overlay_host.h"
#include "png_codec.h"
#include "projection_host.h"
#include "scene_prep.h"
#include "whitted_params.h"

extern "C" hipError_t wt_fast_launch_trace(const whitted_params*, int, unsigned, size_t, hipStream_t);
extern "C" hipError_t wt_fast_launch_raygen(const raygen_params*, hipStream_t);
extern "C" hipError_t wt_strict_launch_trace(const whitted_params*, int, unsigned, size_t, hipStream_t);
extern "C" hipError_t wt_strict_launch_raygen(const raygen_params*, hipStream_t);
extern "C" hipError_t wt_fast_launch_unit(int, const float*, float*, unsigned, unsigned, unsigned, unsigned, hipStream_t);
extern "C" hipError_t wt_strict_launch_unit(int, const float*, float*, unsigned, unsigned, unsigned, unsigned, hipStream_t);
extern "C" hipError_t wt_fast_launch_unit_scene(const whitted_params*, int, int, const float*, float*, unsigned, unsigned, unsigned, size_t, hipStream_t);
extern "C" hipError_t wt_strict_launch_unit_scene(const whitted_params*, int, int, const float*, float*, unsigned, unsigned, unsigned, size_t, hipStream_t);
extern "C" hipError_t wt_fast_launch_gbuffer(const whitted_params*, int, unsigned, size_t, float*, unsigned*, float*, float*, float*, const wt_projection*, hipStream_t);
extern "C" hipError_t wt_strict_launch_gbuffer(const whitted_params*, int, unsigned, size_t, float*, unsigned*, float*, float*, float*, const wt_projection*, hipStream_t);
extern "C" hipError_t wt_fast_launch_raygen_proj(const raygen_params*, const wt_projection*, hipStream_t);
extern "C" hipError_t wt_strict_launch_raygen_proj(const raygen_params*, const wt_projection*, hipStream_t);
extern "C" hipError_t wt_fast_launch_overlay(const unsigned*, const unsigned*, unsigned*, unsigned, unsigned, unsigned, const unsigned*, const unsigned*, unsigned, hipStream_t);
extern "C" hipError_t wt_strict_launch_overlay(const unsigned*, const unsigned*, unsigned*, unsigned, unsigned, unsigned, const unsigned*, const unsigned*, unsigned, hipStream_t);
extern "C" hipError_t wt_fast_launch_objects(const unsigned*, const unsigned*, unsigned, unsigned, unsigned, const unsigned*, const unsigned*, void*, void*, hipStream_t);
extern "C" hipError_t wt_strict_launch_objects(const unsigned*, const unsigned*, unsigned, unsigned, unsigned, const unsigned*, const unsigned*, void*, void*, hipStream_t);
extern "C" hipError_t wt_fast_launch_ao_trace(const whitted_params*, int, const float*, const float*, const unsigned*, const float*, unsigned char*, unsigned, unsigned, unsigned, unsigned, float, hipStream_t);
extern "C" hipError_t wt_strict_launch_ao_trace(const whitted_params*, int, const float*, const float*, const unsigned*, const float*, unsigned char*, unsigned, unsigned, unsigned, unsigned, float, hipStream_t);
extern "C" hipError_t wt_fast_launch_ao_resolve(const unsigned char*, const unsigned*, const unsigned*, unsigned*, unsigned, unsigned, unsigned, unsigned, unsigned, hipStream_t);
extern "C" hipError_t wt_strict_launch_ao_resolve(const unsigned char*, const unsigned*, const unsigned*, unsigned*, unsigned, unsigned, unsigned, unsigned, unsigned, hipStream_t);
extern "C" hipError_t wt_fast_launch_cast(const whitted_params*, int, unsigned, unsigned, size_t, const void*, unsigned, unsigned, void*, unsigned char*, hipStream_t);
extern "C" hipError_t wt_strict_launch_cast(const whitted_params*, int, unsigned, unsigned, size_t, const void*, unsigned, unsigned, void*, unsigned char*, hipStream_t);
extern "C" hipError_t wt_fast_launch_cams(const wt_cam_table*, float*, hipStream_t);
extern "C" hipError_t wt_fast_launch_classify(const unsigned*, unsigned, unsigned, unsigned, unsigned, unsigned char*, unsigned*, unsigned*, unsigned, hipStream_t);
extern "C" hipError_t wt_fast_launch_sched(const unsigned*, unsigned*, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, hipStream_t);

namespace {

constexpr size_t COUNTER_WORDS = CLW_NUM_COUNTERS + 16 * (size_t)CLW_STAMP_SHARDS;
constexpr size_t GRID_MAX_PAIRS = (size_t)1 << 25;   /* 20 B per cell-list entry */

[[noreturn]] void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("ERROR:\t");
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
    fflush(stdout);
    exit(1);
}

/* the same floats bit for bit (+0 and -0 differ, a NaN equals itself): "the device table is unchanged" is decided on what it holds */
bool same_bits(const std::vector<float>& a, const float* b, size_t n) {
    return a.size() == n && (n == 0 || !memcmp(a.data(), b, n * sizeof(float)));
}

#define HIP_OK(call, what)                                                        \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) die("%s (%s)", what, hipGetErrorString(e_));        \
    } while (0)

enum KernelKind { K_RAYGEN = 0, K_RAYTRACER = 1 };

typedef wt_raygen RaygenArgs;   /* snapshot of the eight by-value raygen arguments + the launch range (launch_plan.h) */
/* field by field (the struct has tail padding, which a memcmp would also compare); floats by bit pattern */
bool same_raygen(const RaygenArgs& a, const RaygenArgs& b) {
    return !memcmp(a.corner, b.corner, 12) && !memcmp(a.origin, b.origin, 12) && !memcmp(a.up, b.up, 12) &&
           !memcmp(a.right, b.right, 12) && !memcmp(&a.w_factor, &b.w_factor, 4) && !memcmp(&a.h_factor, &b.h_factor, 4) &&
           a.width == b.width && a.height == b.height && a.id_offset == b.id_offset && a.n_items == b.n_items &&
           a.band_stride == b.band_stride && a.band_phase == b.band_phase;
}

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
    /* the primary-hit pass (clw_ext_render_gbuffer / clw_ext_pick; whitted_gbuffer.inc): planar channel buffers indexed like the framebuffer, one per
     * CLW_GB_* bit, allocated when a pass first asks for them and sized for the pass's range; `done` is recorded behind every pass on the stream it
     * ran on, so a read-back waits for the pass whatever the launch stream is by then */
    struct GBuffer {
        void* chan[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   /* depth, id, normal, point, albedo */
        uint32_t n = 0;                 /* work-items the buffers are sized for */
        uint32_t written = 0;           /* the channels of the last pass */
        uint32_t* pick = nullptr;       /* the 11 words of one clw_pick: a pick is the pass on a one-pixel range, its channels laid out as the struct */
        hipEvent_t done = nullptr;
        void free_channels() { for (void*& q : chan) { if (q) (void)hipFree(q); q = nullptr; } n = 0; written = 0; }
    } gb;
    /* the selection overlay (clw_ext_render_overlay; whitted_overlay.inc): its own id buffer -- the primary-hit pass writes it, `gb` is not touched --
     * and the composed frame, both sized for the pass's range; `done` as above */
    struct Overlay {
        uint32_t* ids = nullptr; uint32_t* frame = nullptr;
        uint32_t n = 0;                 /* work-items the buffers are sized for */
        bool written = false;           /* a pass has composed `frame` */
        hipEvent_t done = nullptr;
        void free_buffers() { if (ids) (void)hipFree(ids); if (frame) (void)hipFree(frame); ids = frame = nullptr; n = 0; written = false; }
    } ov;
    /* the visible-object table (clw_ext_object_stats; whitted_objects.inc): its own id and depth buffers -- the primary-hit pass writes them, `gb`
     * and `ov` are not touched -- sized for the pass's range, and the slot table (16 bytes of counters + 48 per slot) and the result (the 16-byte
     * summary + room for a 48-byte record per slot), sized for the scene's counts.  Every call waits for its own work, so nothing is ever in flight
     * on these buffers between calls. */
    struct Objects {
        uint32_t* ids = nullptr; float* depth = nullptr;
        uint32_t n = 0;                 /* work-items ids and depth are sized for */
        void* table = nullptr; void* result = nullptr;
        uint32_t slots = 0;             /* slots table and result are sized for */
        void size_range(uint32_t items) {
            if (n == items) return;
            if (ids) (void)hipFree(ids);
            if (depth) (void)hipFree(depth);
            ids = nullptr; depth = nullptr; n = 0;
            HIP_OK(hipMalloc((void**)&ids, (size_t)items * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&depth, (size_t)items * 4), "Couldn't allocate device memory");
            n = items;
        }
        void size_table(uint32_t count) {
            if (slots == count) return;
            if (table) (void)hipFree(table);
            if (result) (void)hipFree(result);
            table = result = nullptr; slots = 0;
            HIP_OK(hipMalloc(&table, 16 + (size_t)count * sizeof(clw_object_stat)), "Couldn't allocate device memory");
            HIP_OK(hipMalloc(&result, sizeof(clw_object_summary) + (size_t)count * sizeof(clw_object_stat)), "Couldn't allocate device memory");
            slots = count;
        }
        void free_buffers() {
            for (void* q : {(void*)ids, (void*)depth, table, result}) if (q) (void)hipFree(q);
            ids = nullptr; depth = nullptr; table = result = nullptr; n = 0; slots = 0;
        }
    } obj;
    /* ambient occlusion (clw_ext_render_ao; whitted_ao.inc): its own point, normal and id buffers -- the primary-hit pass writes them, `gb`, `ov`
     * and `obj` are not touched --, the open-ray counts and the resolved frame, all sized for the pass's range; `done` as above.  The direction
     * table (16 x K float4, room for K = 32) is written only when K changes, behind a wait for the passes that read the old one. */
    struct AO {
        float* point = nullptr; float* normal = nullptr; uint32_t* ids = nullptr; uint8_t* open = nullptr; uint32_t* frame = nullptr;
        uint32_t n = 0;                 /* work-items the buffers are sized for */
        bool written = false;           /* a pass has filled `open` and `frame` */
        float* dirs = nullptr; uint32_t dirs_K = 0;      /* the table on the device and the K it was built for (0 = none yet) */
        hipEvent_t done = nullptr;
        void free_buffers() {
            for (void* q : {(void*)point, (void*)normal, (void*)ids, (void*)open, (void*)frame}) if (q) (void)hipFree(q);
            point = normal = nullptr; ids = nullptr; open = nullptr; frame = nullptr; n = 0; written = false;
        }
    } ao;
    /* ray queries (clw_ext_cast_rays / clw_ext_occluded_rays; whitted_cast.inc): the buffers of the host-array entry points -- the rays as uploaded,
     * the hits, the blocked bytes -- sized for the largest n so far.  Those calls wait for their own work, so nothing is in flight on them between
     * calls; clw_ext_cast_rays_device works on the caller's memory and owns nothing. */
    struct Cast {
        void* rays = nullptr; void* hits = nullptr; uint8_t* blocked = nullptr;
        uint32_t cap = 0;               /* rays the buffers hold */
        void free_buffers() {
            for (void* q : {rays, hits, (void*)blocked}) if (q) (void)hipFree(q);
            rays = hits = nullptr; blocked = nullptr; cap = 0;
        }
    } cast;
    /* prepared scene cache */
    const Buffer *prep_s = nullptr, *prep_p = nullptr, *prep_l = nullptr;
    uint32_t prep_ns = 0, prep_np = 0, prep_nl = 0;
    float* d_geom = nullptr; size_t geom_f4 = 0;
    float* d_ptex = nullptr;
    bool have_lpt = false;    /* the light / plane side table follows the lights in d_geom */
    uint64_t scene_generation = 0;   /* bumped every time the prepared scene is rebuilt (device pointers can be reused) */
    uint32_t *d_grid_start = nullptr, *d_grid_items = nullptr, *d_grid_box = nullptr;
    float* d_grid_geom = nullptr;
    wprep_grid grid{}; bool grid_ok = false, grid_pair = false; int use_grid = 1;
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

bool same_acc_key(const Impl::AccKey& a, const Impl::AccKey& b) {
    return same_raygen(a.gen, b.gen) && a.n_out == b.n_out && a.total == b.total && a.depth == b.depth && a.strict == b.strict && a.fuse == b.fuse &&
           a.ss == b.ss && a.max_frames == b.max_frames && a.jitter == b.jitter && !memcmp(&a.through, &b.through, 4) && a.seed == b.seed &&
           !memcmp(a.buf, b.buf, sizeof a.buf) && !memcmp(a.dptr, b.dptr, sizeof a.dptr) && !memcmp(a.size, b.size, sizeof a.size) &&
           !memcmp(a.counts, b.counts, sizeof a.counts) && !memcmp(a.img, b.img, sizeof a.img) && a.epoch == b.epoch;
}

Impl* impl_of(const cl_wrap* w) {
    if (!w || !w->impl) die("cl_wrap is not initialised");
    return (Impl*)w->impl;
}

void use_device(Impl* I) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != I->device) HIP_OK(hipSetDevice(I->device), "Cannot select the HIP device");
}

bool is_registered(const cl_wrap* w, cl_uint kernel_id, cl_uint arg_id) {
    for (cl_uint i = 0; i < w->buffers_num[kernel_id]; i++)
        if (w->buffers_ids[kernel_id][i] == arg_id) return true;
    return false;
}

void check_kernel_id(const cl_wrap* w, cl_uint kernel_id) {
    if (kernel_id >= w->kernels_num) die("Wrong kernel ID given");
}

Buffer* new_buffer(Impl* I) {
    Buffer* b = new Buffer();
    I->live.push_back(b);
    return b;
}

Buffer* lookup_handle(Impl* I, const void* handle) {
    for (Buffer* b : I->live)
        if ((const void*)b == handle) return b;
    return nullptr;
}

void ensure_allocated(Impl* I, Buffer* b) {
    (void)I;
    if (b->dptr || b->size == 0) return;
    HIP_OK(hipMalloc(&b->dptr, b->size), "Couldn't allocate device memory");
    b->lazy = false;
}

void register_buffer(cl_wrap* w, cl_uint kernel_id, cl_uint arg_id, Buffer* b) {
    w->buffers[kernel_id][arg_id] = (cl_mem)b;
    w->buffers_ids[kernel_id][w->buffers_num[kernel_id]++] = arg_id;
}

void precheck_buffer_arg(cl_wrap* w, cl_uint kernel_id, cl_uint arg_id) {
    check_kernel_id(w, kernel_id);
    if (arg_id < __MAX_BUFFERS && is_registered(w, kernel_id, arg_id)) die("Given kernel argument already in use");
    if (arg_id >= __MAX_BUFFERS) die("Wrong kernel ID given"); /* the reference's wording (opencl_wrap.c:144) */
}

/* ---- launch helpers -------------------------------------------------------------------- */
std::pair<hipEvent_t, hipEvent_t> take_events(Impl* I) {
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

void finish(Impl* I) {
    hipError_t e = hipStreamSynchronize(I->stream);
    if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
}

const ArgValue& need_value(const Kernel& k, cl_uint arg, size_t min_size, size_t max_size) {
    const ArgValue& v = k.values[arg];
    if (!v.set || v.size < min_size || v.size > max_size) die("Couldn't run the kernel");
    return v;
}

RaygenArgs snapshot_raygen(Impl* I, const Kernel& k, size_t array_size) {
    RaygenArgs g{};
    memcpy(g.corner, need_value(k, 0, 12, 16).bytes, 12);
    memcpy(g.origin, need_value(k, 1, 12, 16).bytes, 12);
    memcpy(g.up, need_value(k, 2, 12, 16).bytes, 12);
    memcpy(g.right, need_value(k, 3, 12, 16).bytes, 12);
    memcpy(&g.w_factor, need_value(k, 4, 4, 4).bytes, 4);
    memcpy(&g.h_factor, need_value(k, 5, 4, 4).bytes, 4);
    memcpy(&g.width, need_value(k, 6, 4, 4).bytes, 4);
    memcpy(&g.height, need_value(k, 7, 4, 4).bytes, 4);
    if (g.width == 0 || g.height == 0) die("Couldn't run the kernel");
    g.id_offset = I->id_offset;
    g.band_stride = I->band_stride; g.band_phase = I->band_phase;
    /* the reference launches ceil(array_size/local)*local items guarded by id < w*h (raygen.cl:11) */
    uint64_t rounded = ((uint64_t)array_size + WT_LAUNCH_ROUND - 1) / WT_LAUNCH_ROUND * WT_LAUNCH_ROUND;
    uint64_t total = (uint64_t)g.width * g.height;
    uint64_t room = total > g.id_offset ? total - g.id_offset : 0;
    if (g.band_stride > 1) {   /* this launch owns every band_stride-th 8-row band of the frame */
        if (g.id_offset != 0 || g.height % (8 * g.band_stride) != 0) die("Row bands need height %% (8*stride) == 0 and no id offset");
        room = total / g.band_stride;
    }
    uint64_t n = rounded < room ? rounded : room;
    if (n > 0xFFFFFFFFull) die("Couldn't run the kernel");
    g.n_items = (uint32_t)n;
    return g;
}

void run_raygen_kernel(Impl* I, const RaygenArgs& g, Buffer* rays, cl_uint kernel_id) {
    ensure_allocated(I, rays);
    size_t cap = rays->size / 64;
    uint32_t n = g.n_items < cap ? g.n_items : (uint32_t)cap; /* never write past the buffer */
    if (n == 0) return;
    raygen_params P{};
    memcpy(P.corner, g.corner, 12); memcpy(P.origin, g.origin, 12);
    memcpy(P.up, g.up, 12); memcpy(P.right, g.right, 12);
    P.w_factor = g.w_factor; P.h_factor = g.h_factor; P.width = g.width; P.height = g.height;
    P.id_offset = g.id_offset; P.n_items = n; P.rays = (float*)rays->dptr;
    P.band_stride = g.band_stride; P.band_phase = g.band_phase;
    LaunchTimer t(I, kernel_id);
    hipError_t e = I->strict ? wt_strict_launch_raygen(&P, I->stream) : wt_fast_launch_raygen(&P, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

void finish(Impl* I);

clw_camera camera_of(const RaygenArgs& g) {
    clw_camera c{};
    memcpy(c.im_corner, g.corner, 12); memcpy(c.origin, g.origin, 12); memcpy(c.up, g.up, 12); memcpy(c.right, g.right, 12);
    c.w_factor = g.w_factor; c.h_factor = g.h_factor; c.width = g.width; c.height = g.height;
    return c;
}

/* The wrapper's projection resolved for a latched camera: the scalar terms and, for the panorama, the device tables -- uploaded only when they
 * differ from what the device holds, behind a wait for the launches that may still read the old ones.  false = the definition refuses this
 * camera / projection pair (projection_host.c). */
bool resolve_projection(Impl* I, const RaygenArgs& g, wt_projection& T) {
    const clw_camera cam = camera_of(g);
    if (!wt_projection_terms(&cam, &I->proj, &T)) return false;
    if (T.model != CLW_PROJ_EQUIRECT) return true;
    Impl::ProjTables& B = I->ptab;
    std::vector<float> col(4 * (size_t)g.width), row(4 * (size_t)g.height);
    if (!clw_host_projection_tables(&cam, &I->proj, col.data(), row.data())) return false;
    if (!same_bits(B.tab_col, col.data(), col.size()) || !same_bits(B.tab_row, row.data(), row.size())) {
        finish(I);
        if (B.cap_w < g.width || B.cap_h < g.height) {
            B.free_all();
            HIP_OK(hipMalloc((void**)&B.d_col, col.size() * sizeof(float)), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&B.d_row, row.size() * sizeof(float)), "Couldn't allocate device memory");
            B.cap_w = g.width; B.cap_h = g.height;
        }
        HIP_OK(hipMemcpy(B.d_col, col.data(), col.size() * sizeof(float), hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
        HIP_OK(hipMemcpy(B.d_row, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
        B.tab_col.swap(col); B.tab_row.swap(row);
    }
    T.col = B.d_col; T.row = B.d_row;
    return true;
}

/* wt_raygen_proj over the range a raygen launch latched: the records of the wrapper's projection, logged under the raygen kernel's id */
void run_raygen_proj_kernel(Impl* I, const RaygenArgs& g, Buffer* rays, cl_uint kernel_id) {
    ensure_allocated(I, rays);
    size_t cap = rays->size / 64;
    uint32_t n = g.n_items < cap ? g.n_items : (uint32_t)cap; /* never write past the buffer */
    if (n == 0) return;
    wt_projection T;
    if (!resolve_projection(I, g, T)) die("The projection (clw_ext_set_projection / CLWRAP_PROJECTION) cannot be resolved for this camera: a zero axis over a camera whose image plane is centred on its origin, or a panorama whose axis is parallel to the camera's right or up");
    raygen_params P{};
    P.width = g.width; P.height = g.height;
    P.id_offset = g.id_offset; P.n_items = n; P.rays = (float*)rays->dptr;
    P.band_stride = g.band_stride; P.band_phase = g.band_phase;
    LaunchTimer t(I, kernel_id);
    hipError_t e = (I->strict ? wt_strict_launch_raygen_proj : wt_fast_launch_raygen_proj)(&P, &T, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

bool same_projection(const clw_projection& a, const clw_projection& b) { return !memcmp(&a, &b, sizeof a); }

/* the records of a generated ray buffer, if they are not there yet -- or were generated under another camera model (a buffer whose pointer was
 * handed out is the caller's: traced as written) */
void materialise_rays(Impl* I, Buffer* b) {
    if (!b->gen_valid) return;
    if (b->gen_materialised && (b->exposed || same_projection(b->gen_proj, I->proj))) return;
    if (I->proj.model != CLW_PROJ_PERSPECTIVE) run_raygen_proj_kernel(I, b->gen, b, 0);
    else run_raygen_kernel(I, b->gen, b, 0);
    b->gen_materialised = true;
    b->gen_proj = I->proj;
}

uint32_t read_count(const Kernel& k, cl_uint arg) {
    const ArgValue& v = k.values[arg];
    if (!v.set) die("Couldn't run the kernel");
    switch (v.size) { /* uchar in the reference (raytracing.cl:17); 2/4 bytes = wide-count extension */
        case 1: return v.bytes[0];
        case 2: { uint16_t x; memcpy(&x, v.bytes, 2); return x; }
        case 4: { uint32_t x; memcpy(&x, v.bytes, 4); return x; }
        default: die("Couldn't run the kernel");
    }
}

const uint8_t* host_view(Impl* I, Buffer* b, size_t need, std::vector<uint8_t>& tmp) {
    if (b->size < need) die("Couldn't run the kernel");
    if (b->shadow.size() >= need) return b->shadow.data();
    ensure_allocated(I, b);
    tmp.resize(need);
    if (need) HIP_OK(hipMemcpy(tmp.data(), b->dptr, need, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    return tmp.data();
}

int env_int(const char* name, int dflt) {
    const char* s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}
/* a float from the environment; anything that is not a number reads as NaN, which every caller refuses */
float env_float(const char* name, float dflt) {
    const char* s = getenv(name);
    if (!s || !*s) return dflt;
    char* end = nullptr;
    const float v = strtof(s, &end);
    return (end == s || *end) ? NAN : v;
}

/* xorshift32 (primitives.cl:116-125) is linear over GF(2): a step is a 32x32 bit matrix T (column b = the step applied to 1 << b), the 4 nl numbers
 * a shaded hit draws are M = T^(4 nl), and the state k hits on is M^k times the state now.  out[i] = M^(2^i), i = 0..6, as columns: the tail's xorshift
 * pass (whitted_tpt.inc, pass C) jumps with them instead of stepping. */
void xorshift_jump_matrices(uint32_t steps, uint32_t out[7][32]) {
    auto apply = [](const uint32_t* A, uint32_t x) { uint32_t r = 0; for (int b = 0; b < 32; b++) if ((x >> b) & 1u) r ^= A[b]; return r; };
    auto mul = [&](const uint32_t* A, const uint32_t* B, uint32_t* C) { uint32_t t[32]; for (int b = 0; b < 32; b++) t[b] = apply(A, B[b]); memcpy(C, t, sizeof t); };
    uint32_t T[32], R[32], Bp[32];
    for (int b = 0; b < 32; b++) { uint32_t x = 1u << b; x ^= x << 13; x ^= x >> 17; x ^= x << 5; T[b] = x; R[b] = 1u << b; }
    memcpy(Bp, T, sizeof T);
    for (uint32_t e = steps; e; e >>= 1) { if (e & 1u) mul(Bp, R, R); mul(Bp, Bp, Bp); }      /* R = T^steps */
    memcpy(out[0], R, sizeof R);
    for (int i = 1; i < 7; i++) mul(out[i - 1], out[i - 1], out[i]);
}

void prepare_scene(Impl* I, Buffer* s, uint32_t ns, Buffer* p, uint32_t np, Buffer* l, uint32_t nl) {
    if (I->d_geom && I->prep_s == s && I->prep_p == p && I->prep_l == l && I->prep_ns == ns &&
        I->prep_np == np && I->prep_nl == nl)
        return;
    std::vector<uint8_t> ts, tp, tl;
    const uint8_t* hs = host_view(I, s, 96 * (size_t)ns, ts);
    const uint8_t* hp = host_view(I, p, 96 * (size_t)np, tp);
    const uint8_t* hl = host_view(I, l, 48 * (size_t)nl, tl);
    const size_t base_f4 = wprep_geom_f4(ns, np, nl), lpt_f4 = wprep_lpt_f4(np, nl);
    size_t f4 = base_f4 + lpt_f4;
    std::vector<float> geom(4 * (f4 ? f4 : 1)), ptex(8 * (size_t)(np ? np : 1));
    wprep_build(hs, ns, hp, np, hl, nl, geom.data(), ptex.data());
    wprep_build_lpt(hp, np, hl, nl, geom.data() + 4 * base_f4);
    I->have_lpt = lpt_f4 != 0;
    {   /* the tail's xorshift jumps for this light count */
        uint32_t jm[7][32];
        xorshift_jump_matrices(4u * nl, jm);
        if (!I->d_tpt_jump) HIP_OK(hipMalloc((void**)&I->d_tpt_jump, sizeof jm), "Couldn't allocate device memory");
        HIP_OK(hipMemcpy(I->d_tpt_jump, jm, sizeof jm, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    }
    if (I->d_geom) { (void)hipFree(I->d_geom); I->d_geom = nullptr; }
    if (I->d_ptex) { (void)hipFree(I->d_ptex); I->d_ptex = nullptr; }
    HIP_OK(hipMalloc((void**)&I->d_geom, geom.size() * 4), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&I->d_ptex, ptex.size() * 4), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(I->d_geom, geom.data(), geom.size() * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemcpy(I->d_ptex, ptex.data(), ptex.size() * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    /* uniform grid over the spheres for big scenes */
    for (uint32_t** q : {&I->d_grid_start, &I->d_grid_items, &I->d_grid_box}) { if (*q) { (void)hipFree(*q); *q = nullptr; } }
    if (I->d_grid_geom) { (void)hipFree(I->d_grid_geom); I->d_grid_geom = nullptr; }
    I->grid_ok = false;
    if (ns > (uint32_t)env_int("CLWRAP_GRID_MIN", (int)WT_GRID_MIN_SPHERES)) {   /* CLWRAP_GRID_MIN: tuning knob */
        const char* dens = getenv("CLWRAP_GRID_DENSITY");   /* tuning knob: average spheres per cell */
        /* the two soft-shadow samples of a light share one walk (wt_grid_shadow_pair) when spheres are listed a light radius beyond their
         * boxes -- worth it while that is a fraction of a cell (CLWRAP_GRID_PAIR=0: every shadow ray walks on its own) */
        float maxr = 0.0f;
        for (uint32_t l = 0; l < nl; l++) { float r; memcpy(&r, hl + 48 * (size_t)l + 16, 4); r = fabsf(r); if (!(r <= maxr)) maxr = r; }
        const float density = dens ? (float)atof(dens) : 1.6f;
        size_t pairs = 0;
        I->grid_pair = false;
        const bool want_pair = I->grid_pair_req < 0 ? env_int("CLWRAP_GRID_PAIR", 1) != 0 : I->grid_pair_req != 0;
        if (want_pair && nl > 0 && maxr > 0.0f && std::isfinite(maxr)) {
            pairs = wprep_grid_plan(hs, ns, density, maxr, &I->grid);
            I->grid_pair = maxr <= 0.3f * std::min(I->grid.cell[0], std::min(I->grid.cell[1], I->grid.cell[2])) && pairs <= GRID_MAX_PAIRS;
        }
        if (!I->grid_pair) pairs = wprep_grid_plan(hs, ns, density, 0.0f, &I->grid);
        if (pairs <= GRID_MAX_PAIRS) {
            std::vector<uint32_t> st((size_t)I->grid.ncells + 1), it(pairs ? pairs : 1), bx(2 * (size_t)ns);
            wprep_grid_fill(hs, ns, &I->grid, st.data(), it.data(), bx.data());
            HIP_OK(hipMalloc((void**)&I->d_grid_start, st.size() * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&I->d_grid_items, it.size() * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&I->d_grid_box, bx.size() * 4), "Couldn't allocate device memory");
            HIP_OK(hipMemcpy(I->d_grid_start, st.data(), st.size() * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
            HIP_OK(hipMemcpy(I->d_grid_items, it.data(), it.size() * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
            HIP_OK(hipMemcpy(I->d_grid_box, bx.data(), bx.size() * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
            /* the prepared sphere of every cell-list entry, next to its index */
            std::vector<float> cg(4 * it.size(), 0.0f);
            for (size_t k = 0; k < pairs; k++) memcpy(&cg[4 * k], &geom[4 * (size_t)it[k]], 16);
            HIP_OK(hipMalloc((void**)&I->d_grid_geom, cg.size() * 4), "Couldn't allocate device memory");
            HIP_OK(hipMemcpy(I->d_grid_geom, cg.data(), cg.size() * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
            I->grid_ok = true;
            I->grid_pairs = pairs;
        }
    }
    I->geom_f4 = f4;
    I->scene_generation++;
    I->prep_s = s; I->prep_p = p; I->prep_l = l; I->prep_ns = ns; I->prep_np = np; I->prep_nl = nl;
}

Buffer* buffer_arg(cl_wrap* w, cl_uint kernel_id, cl_uint arg) {
    if (!is_registered(w, kernel_id, arg)) die("Couldn't run the kernel");
    return (Buffer*)w->buffers[kernel_id][arg];
}

/* arg 0 of the raytracer: the ray buffer, passed by value as the 8 bytes of a handle (raypng.c:61) or bound as a buffer; null = neither */
Buffer* find_rays(const cl_wrap* w, Impl* I, cl_uint kid) {
    if (is_registered(w, kid, 0)) return (Buffer*)w->buffers[kid][0];
    const ArgValue& v = I->kernels[kid].values[0];
    if (!v.set || v.size != sizeof(cl_mem)) return nullptr;
    void* h; memcpy(&h, v.bytes, sizeof h);
    return lookup_handle(I, h);
}
Buffer* rays_of(const cl_wrap* w, Impl* I, cl_uint kid) {
    Buffer* rays = find_rays(w, I, kid);
    if (!rays) die("Couldn't run the kernel");
    return rays;
}
/* arg 7 of the raytracer: the guard `total_size` (raytracing.cl:24) */
bool find_total(const Kernel& k, uint32_t& total) {
    if (!k.values[7].set || k.values[7].size != 4) return false;
    memcpy(&total, k.values[7].bytes, 4);
    return true;
}
uint32_t total_of(const Kernel& k) {
    uint32_t total;
    if (!find_total(k, total)) die("Couldn't run the kernel");
    return total;
}

/* the device tables, an adaptive launch's buffers and the accumulation sum are written and read in stream order: after a change of stream
 * (clw_ext_set_stream) the first launch that touches one waits for the old stream's fence */
void wait_tables_fence(Impl* I) {
    if (!I->tables_fence_pending) return;
    HIP_OK(hipStreamWaitEvent(I->stream, I->tables_fence, 0), "Couldn't run the kernel");
    I->tables_fence_pending = false;
}

/* The scene side of a raytracer launch (args 1-6, 8, 9 of kernel `kid`): checks the bindings and prepares the geometry (once per scene) */
void prepare_bound_scene(cl_wrap* w, Impl* I, cl_uint kid) {
    Kernel& k = I->kernels[kid];
    Buffer* bs = buffer_arg(w, kid, 1);
    Buffer* bp = buffer_arg(w, kid, 2);
    Buffer* bl = buffer_arg(w, kid, 3);
    uint32_t ns = read_count(k, 4), np = read_count(k, 5), nl = read_count(k, 6);
    Buffer* tex = buffer_arg(w, kid, 8);
    Buffer* sky = buffer_arg(w, kid, 9);
    if (!tex->image || !sky->image) die("Couldn't run the kernel");
    prepare_scene(I, bs, ns, bp, np, bl, nl);
    ensure_allocated(I, bs); ensure_allocated(I, bp);
}
/* ... and its device pointers, with the words that describe what they point to (flags: the geometry class, wt_plan_geometry) */
void bind_scene_pointers(const cl_wrap* w, Impl* I, cl_uint kid, whitted_params& P, int flags) {
    const Buffer *bs = (Buffer*)w->buffers[kid][1], *bp = (Buffer*)w->buffers[kid][2], *tex = (Buffer*)w->buffers[kid][8], *sky = (Buffer*)w->buffers[kid][9];
    P.geom = I->d_geom; P.ptex = I->d_ptex;
    P.spheres_raw = (const uint8_t*)bs->dptr; P.planes_raw = (const uint8_t*)bp->dptr;
    P.tex = (const uint32_t*)tex->dptr; P.tex_w = (int)tex->w; P.tex_h = (int)tex->h; P.tex_layers = (int)tex->layers;
    P.sky = (const uint32_t*)sky->dptr; P.sky_w = (int)sky->w; P.sky_h = (int)sky->h;
    if (flags & WT_F_GRID) {
        P.grid_pair = I->grid_pair ? 1u : 0u;
        P.grid_start = I->d_grid_start; P.grid_items = I->d_grid_items; P.grid_box = I->d_grid_box; P.grid_geom = I->d_grid_geom;
        for (int a = 0; a < 3; a++) {
            P.grid_min[a] = I->grid.gmin[a]; P.grid_inv[a] = I->grid.inv[a]; P.grid_cell[a] = I->grid.cell[a]; P.grid_res[a] = I->grid.res[a];
        }
    }
}
/* both, for the launches that are not planned (the primary-hit pass, clw_ext_unit_scene): fills the scene fields of P and chooses between the
 * uniform grid, LDS-staged geometry and geometry read from global memory (flags WT_F_GRID / WT_F_GEOM_LDS, dynamic LDS bytes) */
void bind_scene(cl_wrap* w, Impl* I, cl_uint kid, whitted_params& P, int& flags, size_t& dyn_lds) {
    prepare_bound_scene(w, I, kid);
    const wt_geom_class gc = wt_plan_geometry(I->strict, I->variant, I->prep_ns, I->prep_np, (uint32_t)I->geom_f4, I->have_lpt, I->grid_ok && I->use_grid);
    flags |= gc.flags;
    if (gc.flags & WT_F_GEOM_LDS) dyn_lds = gc.dyn_lds;
    P.ns = I->prep_ns; P.np = I->prep_np; P.nl = I->prep_nl; P.geom_f4 = (uint32_t)I->geom_f4;
    P.lpt = gc.lpt; P.vis = gc.vis;
    P.through = I->through;
    bind_scene_pointers(w, I, kid, P, gc.flags);
}

/* one strip of a frame: rows [row0, row0 + rows) of the launch range, scheduling state in scheds[slot] */
struct Strip { uint32_t row0, rows; int slot; };

/* what a trace launch is: the whole thing, or one of the two passes of an adaptive launch (run_raytracer; launch_plan.h) */
enum TracePass { PASS_PLAIN = WT_PASS_PLAIN, PASS_BASE = WT_PASS_BASE, PASS_REFINE = WT_PASS_REFINE };

/* what the planner is told about a launch: the knobs, the prepared scene, the ray buffer, the range */
void plan_input(const Impl* I, const Buffer* rays, size_t array_size, uint32_t total, size_t out_size, const Strip* strip, TracePass pass, wt_plan_in& in) {
    in.depth = I->depth; in.strict = I->strict; in.fuse = I->fuse; in.counting = I->counting; in.stamps = I->stamps; in.tpt_clock = I->tpt_clock;
    in.variant = I->variant; in.supersample = I->supersample; in.adaptive = I->adaptive; in.seed_offset = I->seed_offset;
    in.acc_frame = I->acc.frame; in.acc_jitter = I->acc_jitter;
    in.aperture = I->aperture; in.focus = I->focus; in.through = I->through;
    in.tpt_max = I->tpt_max; in.tpt_pool_mb = I->tpt_pool_mb; in.tpt_min = I->tpt_min; in.split_min_quota = I->split_min_quota;
    in.occ_tiles_per_depth = I->occ_tiles_per_depth; in.sched = I->sched;
    in.diag = (I->variant & WT_V_TIMELINE) ? (env_int("CLWRAP_TIMELINE_EDGES", 0) ? 255u + (uint32_t)env_int("CLWRAP_TIMELINE_EDGES", 0) : 1u + (uint32_t)env_int("CLWRAP_TIMELINE_SHIFT", 0)) : 0u;
    in.id_offset = I->id_offset; in.band_stride = I->band_stride;
    in.scene_ok = 1;      /* (prepare_bound_scene refused anything else, with the planner's text, where the planner would) */
    in.ns = I->prep_ns; in.np = I->prep_np; in.nl = I->prep_nl; in.geom_f4 = (uint32_t)I->geom_f4;
    in.have_lpt = I->have_lpt; in.grid_usable = I->grid_ok && I->use_grid;
    in.args_ok = 1;
    in.rays_generated = rays->gen_valid ? 1 + (int32_t)I->proj.model : 0; in.rays_exposed = rays->exposed; in.gen = rays->gen; in.rays_size = rays->size;
    in.array_size = array_size; in.out_size = out_size; in.total = total;
    in.has_strip = strip != nullptr; in.strip_row0 = strip ? strip->row0 : 0u; in.strip_rows = strip ? strip->rows : 0u;
    in.pass = pass;
    in.cams = I->cams.data(); in.n_cams = (uint32_t)I->cams.size();
    in.times = I->motion_times.data(); in.n_times = (uint32_t)I->motion_times.size(); in.explicit_times = I->motion_explicit_times;
    in.disp = I->motion_disp.data(); in.n_disp = (uint32_t)I->motion_disp.size();
}

/* ---- the effects of a planned launch, in stream order; each touches one piece of Impl state -------------------------------------------- */
/* the tables of the launch, for clw_ext_get_sample_cameras / _times */
void keep_samples(Impl* I, const wt_plan_out& plan) {
    I->cams_used.clear(); I->times_used.clear();
    if (plan.n_cams) I->cams_used.assign(plan.cams_used, plan.cams_used + plan.n_cams);
    if (plan.n_times) I->times_used.assign(plan.times_used, plan.times_used + plan.n_times);
}

/* scene, framebuffer and -- for a launch that reads its rays -- the ray buffer, generated now if it is still virtual */
void bind_buffers(cl_wrap* w, Impl* I, cl_uint kid, Buffer* rays, const Buffer* out, wt_plan_out& plan) {
    whitted_params& P = plan.P;
    bind_scene_pointers(w, I, kid, P, plan.flags);
    P.out = (uint32_t*)out->dptr + plan.out_offset;
    P.out_rgb = I->debug_rgb;
    if (!plan.fused) {
        materialise_rays(I, rays);
        ensure_allocated(I, rays);
        P.rays = (const float*)rays->dptr;
    }
}

/* The per-lane sample cameras and the moving spheres' table: the device copy is rewritten, only when it changed, by a small kernel on the
 * launch stream that carries the table (in pieces of one wt_cam_table) as its argument */
void bind_tables(Impl* I, wt_plan_out& plan) {
    if (plan.n_cams) {
        if (!I->d_cams) HIP_OK(hipMalloc((void**)&I->d_cams, sizeof(wt_cam_table)), "Couldn't allocate device memory");
        wait_tables_fence(I);
        if (!I->cams_dev_valid || memcmp(&plan.cam_table, &I->cams_dev, sizeof plan.cam_table)) {
            if (wt_fast_launch_cams(&plan.cam_table, I->d_cams, I->stream) != hipSuccess) die("Couldn't run the kernel");
            I->cams_dev = plan.cam_table; I->cams_dev_valid = true;
        }
        I->tables_in_flight = true;
        plan.P.ss_cams = I->d_cams;
    }
    if (plan.motion_floats) {
        if (!I->d_motion) HIP_OK(hipMalloc((void**)&I->d_motion, 2 * sizeof(wt_cam_table)), "Couldn't allocate device memory");
        wait_tables_fence(I);
        if (!same_bits(I->motion_dev, plan.motion_table, plan.motion_floats)) {
            for (size_t c = 0; c < plan.motion_floats / WT_CAM_TABLE_FLOATS; c++) {
                wt_cam_table piece;
                memcpy(piece.v, &plan.motion_table[c * WT_CAM_TABLE_FLOATS], sizeof piece);
                if (wt_fast_launch_cams(&piece, I->d_motion + c * WT_CAM_TABLE_FLOATS, I->stream) != hipSuccess) die("Couldn't run the kernel");
            }
            I->motion_dev.assign(plan.motion_table, plan.motion_table + plan.motion_floats);
        }
        I->tables_in_flight = true;
        plan.P.ss_times = I->d_motion; plan.P.ss_disp = I->d_motion + 64;
    }
}

/* the running sum of an accumulated view: 3 floats per output pixel of the launch range (whole-range launches only: the pipelined read-back
 * declines in the mode) */
void bind_accumulation(Impl* I, wt_plan_out& plan) {
    Impl::Accum& A = I->acc;
    if (!plan.fused || A.frame < 0) return;
    if (A.pixels != (size_t)plan.out_pixels || !A.sum) {
        if (A.frame != 0) die("Couldn't run the kernel");      /* (the range is part of the key: a new range starts at frame 0) */
        if (A.sum) { finish(I); (void)hipFree(A.sum); A.sum = nullptr; }
        HIP_OK(hipMalloc((void**)&A.sum, (size_t)plan.out_pixels * 12), "Couldn't allocate device memory");
        A.pixels = plan.out_pixels;
    }
    wait_tables_fence(I);
    I->tables_in_flight = true;
    plan.P.acc_sum = A.sum;
}

void bind_counters(Impl* I, wt_plan_out& plan) {
    if (!plan.need_counters) return;
    if (!I->d_counters) {
        HIP_OK(hipMalloc((void**)&I->d_counters, COUNTER_WORDS * sizeof(unsigned long long)), "Couldn't allocate device memory");
        HIP_OK(hipMemsetAsync(I->d_counters, 0, COUNTER_WORDS * sizeof(unsigned long long), I->stream), "Couldn't allocate device memory");
    }
    plan.P.counters = I->d_counters;
}

/* the refine pass of an adaptive launch: the classifier reads the base pass's pixels and writes the mask, the eight tile lists and their lengths;
 * the buffers follow the launch range and the factor */
void classify_blocks(Impl* I, wt_plan_out& plan) {
    whitted_params& P = plan.P;
    const uint32_t ow = P.width >> P.ss_lg, orows = P.rows >> P.ss_lg;
    Impl::Adaptive& A = I->adapt;
    if (A.w != ow || A.rows != orows || A.ss != plan.ss || !A.mask) {
        A.free_all();
        HIP_OK(hipMalloc((void**)&A.mask, (size_t)plan.trows * plan.tpr), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&A.order, (size_t)plan.grid * 4), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&A.count, 8 * WT_LIST_COUNT_STRIDE * 4), "Couldn't allocate device memory");
        A.w = ow; A.rows = orows; A.ss = plan.ss;
    }
    wait_tables_fence(I);
    HIP_OK(hipMemsetAsync(A.count, 0, 8 * WT_LIST_COUNT_STRIDE * 4, I->stream), "Couldn't run the kernel");
    if (wt_fast_launch_classify(P.out, ow, orows, 3u - P.ss_lg, (unsigned)I->adaptive, A.mask, A.order, A.count, plan.per_share, I->stream) != hipSuccess)
        die("Couldn't run the kernel");
    I->tables_in_flight = true;
    A.blocks = plan.trows * plan.tpr;
    P.tile_order = A.order; P.list_count = A.count;
}

/* the cost-sorted tile order of a tiled launch: the cost buffer it writes, the order it reads (wt_order_choose), the builds it waits for
 * -> whether this frame's costs are sorted behind the launch (sort_tile_costs) */
bool bind_tile_order(Impl* I, Impl::Sched& S, wt_plan_out& plan, const Strip* strip) {
    whitted_params& P = plan.P;
    if (!strip) S.last_rd = -1;
    if (!plan.use_order) return false;
    const size_t ntiles = (size_t)plan.trows * plan.tpr;
    if (S.w != P.width || S.rows != P.rows || S.cap != plan.per_share_cap || S.ss != plan.ss || !S.cost[0]) {
        S.free_all();
        for (int i = 0; i < 2; i++) {
            HIP_OK(hipMalloc((void**)&S.cost[i], ntiles * 4), "Couldn't allocate device memory");
            HIP_OK(hipMalloc((void**)&S.order[i], (size_t)plan.grid * 4), "Couldn't allocate device memory");
            HIP_OK(hipEventCreateWithFlags(&S.built[i], hipEventDisableTiming), "Couldn't create a timing event");
        }
        HIP_OK(hipEventCreateWithFlags(&S.traced, hipEventDisableTiming), "Couldn't create a timing event");
        S.w = P.width; S.rows = P.rows; S.cap = plan.per_share_cap; S.ss = plan.ss; S.o.wr = 0;
    }
    const int wr = S.o.wr;
    P.tile_cost = S.cost[wr];
    const wt_order_choice c = wt_order_choose(&S.o);
    if (c.wait_wr) HIP_OK(hipStreamWaitEvent(I->stream, S.built[wr], 0), "Couldn't run the kernel");
    if (c.wait_rd) HIP_OK(hipStreamWaitEvent(I->stream, S.built[c.rd], 0), "Couldn't run the kernel");
    P.tile_order = c.rd >= 0 ? S.order[c.rd] : nullptr;
    if (!strip) S.last_rd = c.rd;
    /* the costs can only change when the camera, the depth or the scene did */
    const bool have_cams = plan.n_cams != 0;
    const bool changed = !S.o.sig_valid || !same_raygen(plan.sig, S.sig) || S.sig_depth != I->depth || S.sig_scene != I->scene_generation || S.sig_has_cams != have_cams ||
                         (have_cams && memcmp(&S.sig_cams, &plan.cam_table, sizeof plan.cam_table)) || !same_bits(S.sig_motion, plan.motion_table, plan.motion_floats);
    /* (costs that add up: the buffer starts at zero; the build that read it two frames ago has been waited for above) */
    if (P.cost_sum) HIP_OK(hipMemsetAsync(S.cost[wr], 0, ntiles * 4, I->stream), "Couldn't run the kernel");
    if (changed) {
        S.sig_motion.assign(plan.motion_table, plan.motion_table + plan.motion_floats);
        S.sig_has_cams = have_cams; if (have_cams) S.sig_cams = plan.cam_table;
        S.sig = plan.sig; S.sig_depth = I->depth; S.sig_scene = I->scene_generation;
    }
    return wt_order_rebuild(&S.o, changed, plan.flags & WT_F_GRID) != 0;
}

/* the tree-parallel tail's pool: one allocation for every launch of its size; without room the launch runs without the tail */
void bind_tail_pool(Impl* I, wt_plan_out& plan) {
    if (!plan.tail_wanted) return;
    whitted_params& P = plan.P;
    const size_t need = (size_t)plan.tpt_slice * 4u * plan.tpt_nslots;
    if (I->tpt_pool_bytes != need) {
        finish(I);
        if (I->d_tpt_pool) (void)hipFree(I->d_tpt_pool);
        if (I->d_tpt_flags) (void)hipFree(I->d_tpt_flags);
        I->d_tpt_pool = nullptr; I->d_tpt_flags = nullptr; I->tpt_pool_bytes = 0;
        if (hipMalloc((void**)&I->d_tpt_pool, need) == hipSuccess && hipMalloc((void**)&I->d_tpt_flags, plan.tpt_nslots * 4u) == hipSuccess) {
            /* on the LAUNCH stream: it does not synchronise with the null stream (hipStreamNonBlocking), and a hipMemset of device memory may
             * return before it has run -- cleared there, the flags could still be garbage when the first waves take their slots, or be
             * zeroed under a wave that holds one, and two tiles would share a slot (seen as an occasional wrong first frame of a deep
             * launch whose tiles all enter the tail at once, clw_ext_set_tpt(64)) */
            HIP_OK(hipMemsetAsync(I->d_tpt_flags, 0, plan.tpt_nslots * 4u, I->stream), "Couldn't allocate device memory");
            I->tpt_pool_bytes = need;
        } else {                                /* no room: the launch runs without the tail */
            (void)hipGetLastError();
            if (I->d_tpt_pool) (void)hipFree(I->d_tpt_pool);
            I->d_tpt_pool = nullptr;
        }
    }
    if (I->tpt_pool_bytes) { P.tpt_pool = I->d_tpt_pool; P.tpt_flags = I->d_tpt_flags; P.tpt_jump = I->d_tpt_jump; }
    else P.tpt_slice_words = P.tpt_cap = P.tpt_slots = P.tpt_max = P.tpt_min = 0u;
}

/* behind the launch: when asked, sort this frame's costs on the side stream; then the cost buffers swap */
void sort_tile_costs(Impl* I, Impl::Sched& S, const wt_plan_out& plan, bool rebuild) {
    const int wr = S.o.wr;
    if (rebuild) {
        if (!I->sched_stream) HIP_OK(hipStreamCreateWithFlags(&I->sched_stream, hipStreamNonBlocking), "Couldn't create a command queue for the given device");
        HIP_OK(hipEventRecord(S.traced, I->stream), "Couldn't run the kernel");
        HIP_OK(hipStreamWaitEvent(I->sched_stream, S.traced, 0), "Couldn't run the kernel");
        if (wt_fast_launch_sched(S.cost[wr], S.order[wr], plan.tpr, plan.trows, plan.per_share, (plan.flags & WT_F_GRID) ? 1u : 0u, plan.per_share_cap,
                                 plan.split ? I->split_slots : 0u, I->split_min_quota, plan.split_max_lg, I->sched_stream) != hipSuccess)
            die("Couldn't run the kernel");
        HIP_OK(hipEventRecord(S.built[wr], I->sched_stream), "Couldn't run the kernel");
    }
    wt_order_launched(&S.o, rebuild);
}

/* One trace launch: the plan (launch_plan.c decides everything that needs no device), then its effects in stream order.
 * -> whether a kernel was launched (an empty range launches none) */
bool trace_launch(cl_wrap* w, Impl* I, cl_uint kid, size_t array_size, const Strip* strip, TracePass pass) {
    Buffer* rays = rays_of(w, I, kid);
    const uint32_t total = total_of(I->kernels[kid]);
    Buffer* out = buffer_arg(w, kid, 10);
    ensure_allocated(I, out);
    if (wt_plan_range(array_size, total, out->size) == 0) return false;      /* before the scene is looked at */
    prepare_bound_scene(w, I, kid);

    wt_plan_in in;
    wt_plan_out plan;      /* (not cleared: the planner writes the head, and the tables only for a launch that uses them) */
    plan_input(I, rays, array_size, total, out->size, strip, pass, in);
    wt_plan(&in, &plan);
    if (plan.status == WT_PLAN_REFUSED) die("%s", plan.message);
    if (plan.samples_decided) keep_samples(I, plan);
    if (plan.status == WT_PLAN_NONE) return false;

    Impl::Sched& S = I->scheds[strip ? strip->slot : 0];
    bind_buffers(w, I, kid, rays, out, plan);
    bind_tables(I, plan);
    bind_accumulation(I, plan);
    bind_counters(I, plan);
    bool sort = false;
    if (pass == PASS_REFINE) classify_blocks(I, plan);
    else if (plan.P.tiled) sort = bind_tile_order(I, S, plan, strip);
    I->last_trace_flags = plan.flags;
    bind_tail_pool(I, plan);
    LaunchTimer t(I, kid, pass == PASS_PLAIN);      /* (an adaptive launch is timed as one: run_raytracer) */
    hipError_t e = (I->strict ? wt_strict_launch_trace : wt_fast_launch_trace)(&plan.P, plan.flags, plan.grid, plan.dyn_lds, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
    if (plan.P.tile_cost) sort_tile_costs(I, S, plan, sort);
    return true;
}

/* what the sampling modes do not combine with (wt_plan_mode_check); `rays` only matters to an accumulated launch */
void check_modes(const Impl* I, const Buffer* rays, bool accumulating) {
    wt_plan_in in{};
    char message[200];
    in.fuse = I->fuse; in.supersample = I->supersample; in.adaptive = I->adaptive; in.aperture = I->aperture;
    in.n_cams = (uint32_t)I->cams.size(); in.n_disp = (uint32_t)I->motion_disp.size();
    in.rays_generated = 1 + (int32_t)I->proj.model;      /* (an adaptive call does not look at the buffer: the plan of its passes does) */
    if (rays) { in.rays_generated = rays->gen_valid ? 1 + (int32_t)I->proj.model : 0; in.rays_exposed = rays->exposed; }
    if (wt_plan_mode_check(&in, accumulating, message)) die("%s", message);
}

/* A trace launch with progressive accumulation on (hip_wrap_ext.h: clw_ext_set_accumulate): refuses what the mode does not combine with, restarts
 * the sum when the key of the image changed, holds a converged view (no launch at all), else traces frame K and folds it in. */
void run_accumulated(cl_wrap* w, Impl* I, cl_uint kid, size_t array_size, const Strip* strip) {
    Kernel& k = I->kernels[kid];
    Buffer* rays = rays_of(w, I, kid);
    check_modes(I, rays, true);
    Impl::Accum& A = I->acc;
    Impl::AccKey key;
    key.gen = rays->gen;
    key.total = total_of(k); key.n_out = (uint64_t)array_size;
    key.depth = I->depth; key.strict = I->strict; key.fuse = I->fuse; key.ss = I->supersample; key.max_frames = I->acc_max; key.jitter = I->acc_jitter;
    key.through = I->through; key.seed = I->seed_offset;
    const cl_uint args[6] = {1, 2, 3, 8, 9, 10};
    key.buf[0] = rays; key.size[0] = rays->size;
    /* (a lazily created buffer -- the framebuffer -- gets its memory here, not inside the first launch: its address is part of the key) */
    for (int a = 0; a < 6; a++) { Buffer* b = buffer_arg(w, kid, args[a]); ensure_allocated(I, b); key.buf[1 + a] = b; key.dptr[1 + a] = b->dptr; key.size[1 + a] = b->size; }
    for (int a = 0; a < 3; a++) key.counts[a] = read_count(k, 4 + (cl_uint)a);
    { const Buffer* t = key.buf[4]; const Buffer* s = key.buf[5]; key.img[0] = t->w; key.img[1] = t->h; key.img[2] = t->layers; key.img[3] = s->w; key.img[4] = s->h; }
    key.epoch = A.epoch;
    if (!A.key_valid || !same_acc_key(key, A.key)) { A.K = 0; A.key = key; A.key_valid = true; }
    if (A.K >= (uint32_t)I->acc_max) return;      /* converged: framebuffer, sum, tile costs, timing log and flavour stay as the last frame left them */
    A.frame = (int)A.K;
    const bool launched = trace_launch(w, I, kid, array_size, strip, PASS_PLAIN);
    A.frame = -1;
    if (launched) A.K++;      /* (an empty launch range traces nothing and adds no frame) */
}

void run_raytracer(cl_wrap* w, Impl* I, cl_uint kid, size_t array_size, const Strip* strip = nullptr) {
    I->adapt.blocks = 0;
    if (I->acc_max > 0) { run_accumulated(w, I, kid, array_size, strip); return; }
    I->acc.key_valid = false;      /* a launch outside the mode: the next accumulated one starts at frame 0 */
    if (I->adaptive < 0) { trace_launch(w, I, kid, array_size, strip, PASS_PLAIN); return; }
    /* Adaptive supersampling (hip_wrap_ext.h: clw_ext_set_adaptive): a 1-sample base pass, the classifier and a supersampled pass over the blocks it listed */
    check_modes(I, nullptr, false);
    LaunchTimer t(I, kid);
    trace_launch(w, I, kid, array_size, strip, PASS_BASE);
    trace_launch(w, I, kid, array_size, strip, PASS_REFINE);
    t.done();
}

/* cl_wrap_output of a big frame with read-back (what rayinteractive.c does every frame, :183-191): the launch is cut
 * into strips of whole tile rows, and strip c travels to the host while strip c+1 renders.  Same pixels (strips
 * keep their global ids), same blocking semantics -- the call returns when the whole frame is in `host_output`.
 * Returns false when the call is not of that shape; the caller then takes the plain path. */
bool pipelined_output(cl_wrap* w, Impl* I, size_t array_size, size_t output_size, cl_uint kid, cl_uint out_kernel,
                      cl_int out_arg, void* host_output) {
    if (!I->pipeline || I->async || !host_output || !I->fuse || I->counting || I->debug_rgb || (I->variant & WT_V_LINEAR_IDS)) return false;
    if (I->acc_max > 0) return false;        /* an accumulated view is one launch per frame, or none at all once it has converged */
    if (I->proj.model != CLW_PROJ_PERSPECTIVE) return false;      /* a projected frame is traced from its ray buffer: one launch */
    if (I->adaptive >= 0) return false;      /* a strip's edge rows would be classified without their neighbours in the next strip: another frame */
    if (out_kernel != kid || out_arg != 10 || !is_registered(w, kid, 10)) return false;
    Buffer* rays = find_rays(w, I, kid);
    uint32_t total;
    if (!rays || !rays->gen_valid || rays->exposed || !find_total(I->kernels[kid], total)) return false;
    const RaygenArgs& g = rays->gen;
    Buffer* out = (Buffer*)w->buffers[kid][10];
    const uint64_t n = g.n_items;
    if (g.band_stride > 1 || g.id_offset % g.width != 0 || n % g.width != 0) return false;
    if (array_size < n || total < n || out->size < n * 4 || output_size != n * 4) return false;   /* the launch covers exactly the generated rays */
    const uint32_t rows = (uint32_t)(n / g.width);
    /* worth it only when the copy is long and the launch is throughput-bound: measured 1.06 -> 0.745 ms at 3840x2160
     * depth 4, +3 % at 1920x1080 (four 2 MB copies are no faster than one of 8 MB), and a LOSS for deep launches,
     * where every strip would pay its own serial tail of refraction trees (0.76 -> 1.30 ms at 1280x1024 depth 15) */
    if (n * 4 < (16u << 20) || rows < 4 * 64 || I->depth > WT_SHALLOW_LEVELS + 1) return false;
    ensure_allocated(I, out);

    const int nch = Impl::MAX_CHUNKS;
    const uint32_t base = rows / nch / 64 * 64;      /* strips of whole 64-row blocks: 8 tile rows, one per XCD */
    if (!I->copy_stream) {
        HIP_OK(hipStreamCreateWithFlags(&I->copy_stream, hipStreamNonBlocking), "Couldn't create a command queue for the given device");
        for (hipEvent_t& e : I->chunk_done) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming), "Couldn't create a timing event");
    }
    for (int c = 0; c < nch; c++) {
        Strip st{(uint32_t)c * base, c == nch - 1 ? rows - (uint32_t)c * base : base, 1 + c};
        run_raytracer(w, I, kid, array_size, &st);
        HIP_OK(hipEventRecord(I->chunk_done[c], I->stream), "Couldn't run the kernel");
    }
    for (int c = 0; c < nch; c++) {
        const size_t off = (size_t)c * base * g.width * 4;
        const size_t bytes = (c == nch - 1 ? (size_t)(rows - (uint32_t)c * base) : (size_t)base) * g.width * 4;
        HIP_OK(hipStreamWaitEvent(I->copy_stream, I->chunk_done[c], 0), "Failed to transfer device memory to host");
        if (hipMemcpyAsync((uint8_t*)host_output + off, (const uint8_t*)out->dptr + off, bytes, hipMemcpyDeviceToHost, I->copy_stream) != hipSuccess)
            die("Failed to transfer device memory to host");
    }
    hipError_t e = hipStreamSynchronize(I->copy_stream);
    if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
    finish(I);
    return true;
}

void run_raygen(cl_wrap* w, Impl* I, cl_uint kid, size_t array_size) {
    Kernel& k = I->kernels[kid];
    Buffer* rays = buffer_arg(w, kid, 8);
    RaygenArgs g = snapshot_raygen(I, k, array_size);
    /* under a camera model the records live in the buffer: a still view -- the same latched values, range and projection, the buffer not handed
     * out -- keeps the ones it has */
    const bool keep = I->proj.model != CLW_PROJ_PERSPECTIVE && rays->gen_valid && rays->gen_materialised && !rays->exposed && same_raygen(g, rays->gen) &&
                      same_projection(rays->gen_proj, I->proj);
    rays->gen = g;
    rays->gen_valid = true;
    rays->gen_materialised = keep;
    rays->exposed = false;
    if (!I->fuse && !keep) {
        if (I->proj.model != CLW_PROJ_PERSPECTIVE) run_raygen_proj_kernel(I, g, rays, kid);
        else run_raygen_kernel(I, g, rays, kid);
        rays->gen_materialised = true;
        rays->gen_proj = I->proj;
    }
}

/* ---- the primary-hit pass -------------------------------------------------------------------------------------------------------- */
constexpr uint32_t GB_WORDS[5] = {1, 1, 3, 3, 3};      /* 4-byte words per work-item of the channels depth, id, normal, point, albedo */

/* The pass's launch parameters over the range the next trace launch would cover: the camera and range the raygen launch latched, clipped by
 * the raytracer's `pixels` argument, bands included; the scene as bind_scene binds it.  false (nothing filled in) when there is no raytracer
 * kernel, no latched camera or no bound scene yet -- the callers return 0 then, they do not terminate the process. */
bool gbuffer_params(cl_wrap* w, Impl* I, whitted_params& P, int& flags, size_t& dyn_lds, wt_projection& T) {
    memset(&T, 0, sizeof T);      /* model 0: the pinhole */
    cl_uint kid = 0;
    while (kid < I->kernels.size() && I->kernels[kid].kind != K_RAYTRACER) kid++;
    if (kid >= I->kernels.size()) return false;
    const Kernel& k = I->kernels[kid];
    Buffer* rays = find_rays(w, I, kid);
    if (!rays || !rays->gen_valid) return false;
    for (cl_uint a : {1u, 2u, 3u, 8u, 9u}) if (!is_registered(w, kid, a)) return false;
    for (cl_uint a : {4u, 5u, 6u}) if (!k.values[a].set) return false;
    uint32_t total;
    if (!find_total(k, total)) return false;
    const RaygenArgs& g = rays->gen;
    const uint32_t n = g.n_items < total ? g.n_items : total;
    if (n == 0) return false;
    if (I->proj.model != CLW_PROJ_PERSPECTIVE && !resolve_projection(I, g, T)) return false;      /* (before anything is bound or launched) */
    bind_scene(w, I, kid, P, flags, dyn_lds);
    wt_plan_fused_range(&g, n, &P);      /* as the fused trace launch: the rays are this library's own */
    if (T.model != CLW_PROJ_PERSPECTIVE) P.unit_dirs = 0u;      /* as the trace launch of a projected view: no direction is taken for unit */
    P.vis = 0;
    return true;
}

void launch_gbuffer(Impl* I, const whitted_params& P, int flags, size_t dyn_lds, void* const chan[5], const wt_projection& T, bool timed) {
    const unsigned grid = wt_plan_grid(&P);      /* as trace_launch: tile rows dealt to the 8 XCDs */
    LaunchTimer t(I, CLW_TIMING_GBUFFER, timed);
    hipError_t e = (I->strict ? wt_strict_launch_gbuffer : wt_fast_launch_gbuffer)(&P, flags, grid, dyn_lds, (float*)chan[0], (unsigned*)chan[1], (float*)chan[2],
                                                                                   (float*)chan[3], (float*)chan[4], &T, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* index of a single CLW_GB_* bit, -1 for anything else */
int gbuffer_channel(uint32_t channel) {
    for (int c = 0; c < 5; c++) if (channel == (1u << c)) return c;
    return -1;
}

/* ---- ray queries ------------------------------------------------------------------------------------------------------------------ */
/* The scene side of a query of n rays: the raytracer's arguments 1-6, prepared as a primary-hit pass prepares them (once per scene), and the plan
 * (wt_plan_cast).  Needs no ray buffer, no camera, no images and no framebuffer.  false (nothing prepared or filled in) when there is no
 * raytracer kernel or no bound scene -- the callers return 0 then, they do not terminate the process. */
bool cast_params(cl_wrap* w, Impl* I, uint32_t n, whitted_params& P, wt_cast_class& cc) {
    cl_uint kid = 0;
    while (kid < I->kernels.size() && I->kernels[kid].kind != K_RAYTRACER) kid++;
    if (kid >= I->kernels.size()) return false;
    const Kernel& k = I->kernels[kid];
    for (cl_uint a : {1u, 2u, 3u}) if (!is_registered(w, kid, a)) return false;
    for (cl_uint a : {4u, 5u, 6u}) if (!k.values[a].set) return false;
    Buffer* bs = (Buffer*)w->buffers[kid][1];
    Buffer* bp = (Buffer*)w->buffers[kid][2];
    Buffer* bl = (Buffer*)w->buffers[kid][3];
    prepare_scene(I, bs, read_count(k, 4), bp, read_count(k, 5), bl, read_count(k, 6));
    cc = wt_plan_cast(I->variant, I->prep_ns, (uint32_t)I->geom_f4, I->grid_ok && I->use_grid, n, (uint32_t)std::max(0, env_int("CLWRAP_CAST_BATCHES", 0)));   /* CLWRAP_CAST_BATCHES: tuning knob */
    if (cc.groups == 0u) return false;
    P.ns = I->prep_ns; P.np = I->prep_np; P.nl = I->prep_nl; P.geom_f4 = (uint32_t)I->geom_f4;
    P.geom = I->d_geom; P.ptex = I->d_ptex;
    if (cc.flags & WT_F_GRID) {
        P.grid_pair = I->grid_pair ? 1u : 0u;
        P.grid_start = I->d_grid_start; P.grid_items = I->d_grid_items; P.grid_box = I->d_grid_box; P.grid_geom = I->d_grid_geom;
        for (int a = 0; a < 3; a++) {
            P.grid_min[a] = I->grid.gmin[a]; P.grid_inv[a] = I->grid.inv[a]; P.grid_cell[a] = I->grid.cell[a]; P.grid_res[a] = I->grid.res[a];
        }
    }
    return true;
}

/* wt_cast over device memory on the launch stream; exactly one of hits / blocked */
void launch_cast(Impl* I, const whitted_params& P, const wt_cast_class& cc, const void* rays, uint32_t n, uint32_t flags, void* hits, uint8_t* blocked) {
    LaunchTimer t(I, CLW_TIMING_CAST, true);
    hipError_t e = (I->strict ? wt_strict_launch_cast : wt_fast_launch_cast)(&P, cc.flags, cc.groups, cc.batches, cc.dyn_lds, rays, n, flags, hits, blocked, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* the two host-array entry points: upload, launch, read back, all in the order of the launch stream, then wait */
uint32_t cast_host_arrays(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, clw_hit* hits, uint8_t* blocked) {
    Impl* I = impl_of(wrap);
    use_device(I);
    static_assert(sizeof(clw_ray) == 32 && sizeof(clw_hit) == 32, "the queries' ABI");
    if (!wt_cast_check(n, flags) || !rays || (!hits && !blocked)) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!cast_params(wrap, I, n, P, cc)) return 0;
    Impl::Cast& C = I->cast;
    if (C.cap < n) {
        C.free_buffers();
        HIP_OK(hipMalloc(&C.rays, (size_t)n * sizeof(clw_ray)), "Couldn't allocate device memory");
        HIP_OK(hipMalloc(&C.hits, (size_t)n * sizeof(clw_hit)), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&C.blocked, (size_t)n), "Couldn't allocate device memory");
        C.cap = n;
    }
    HIP_OK(hipMemcpyAsync(C.rays, rays, (size_t)n * sizeof(clw_ray), hipMemcpyHostToDevice, I->stream), "Couldn't transfer the data from host to the device");
    launch_cast(I, P, cc, C.rays, n, flags, hits ? C.hits : nullptr, hits ? nullptr : C.blocked);
    if (hits) HIP_OK(hipMemcpyAsync(hits, C.hits, (size_t)n * sizeof(clw_hit), hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    else HIP_OK(hipMemcpyAsync(blocked, C.blocked, (size_t)n, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    finish(I);
    return n;
}

/* ---- the selection overlay ------------------------------------------------------------------------------------------------------- */
/* wt_overlay over a width x rows range on the launch stream; the caller has checked style and selection (wt_overlay_check).  The kernel is
 * integer work compiled into both units; the build in use launches its own copy. */
void launch_overlay(Impl* I, const uint32_t* frame, const uint32_t* ids, uint32_t* out, uint32_t width, uint32_t rows, const clw_overlay& st,
                    const uint32_t* sel, uint32_t count, bool timed) {
    const unsigned style[5] = {st.radius, st.outline_rgb, st.fill_rgb, st.fill_alpha, st.edge_rgb};
    LaunchTimer t(I, CLW_TIMING_OVERLAY, timed);
    hipError_t e = (I->strict ? wt_strict_launch_overlay : wt_fast_launch_overlay)(frame, ids, out, width, rows, st.flags, style, sel, count, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* ---- ambient occlusion ------------------------------------------------------------------------------------------------------------ */
/* the direction table of K rays on the device: built by the definition (clw_host_ao_dirs) and uploaded only when K changes -- then behind a wait
 * for whatever the launch stream still runs, which may read the old one */
const float* ao_dirs(Impl* I, uint32_t K) {
    Impl::AO& O = I->ao;
    if (O.dirs && O.dirs_K == K) return O.dirs;
    std::vector<float> tab(4 * (size_t)WT_AO_PATTERNS * K);
    if (!clw_host_ao_dirs(K, tab.data())) die("Couldn't run the kernel");
    if (!O.dirs) HIP_OK(hipMalloc((void**)&O.dirs, 4 * sizeof(float) * WT_AO_PATTERNS * WT_AO_MAX_RAYS), "Couldn't allocate device memory");
    finish(I);
    if (O.done) (void)hipEventSynchronize(O.done);
    HIP_OK(hipMemcpy(O.dirs, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    O.dirs_K = K;
    return O.dirs;
}

/* wt_ao_trace over device channels of a width x rows range on the launch stream, the scene as `P` and `flags` bind it (bind_scene); the caller
 * has checked `ao` and the range (wt_ao_check, wt_ao_range_ok) */
void launch_ao_trace(Impl* I, const whitted_params& P, int flags, const float* point, const float* normal, const uint32_t* ids, uint32_t width,
                     uint32_t rows, uint32_t first_row, const clw_ao& ao, uint8_t* open, bool timed) {
    const float* dirs = ao_dirs(I, ao.rays);
    LaunchTimer t(I, CLW_TIMING_AO, timed);
    hipError_t e = (I->strict ? wt_strict_launch_ao_trace : wt_fast_launch_ao_trace)(&P, flags, point, normal, ids, dirs, open, width, rows, first_row,
                                                                                     ao.rays, ao.radius, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* wt_ao_resolve likewise.  Integer work compiled into both units; the build in use launches its own copy. */
void launch_ao_resolve(Impl* I, const uint8_t* open, const uint32_t* ids, const uint32_t* frame, uint32_t* out, uint32_t width, uint32_t rows,
                       const clw_ao& ao, bool timed) {
    LaunchTimer t(I, CLW_TIMING_AO_RESOLVE, timed);
    hipError_t e = (I->strict ? wt_strict_launch_ao_resolve : wt_fast_launch_ao_resolve)(open, ids, frame, out, width, rows, ao.flags, ao.rays, ao.strength,
                                                                                         I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* ---- the visible-object table ---------------------------------------------------------------------------------------------------- */
/* The clear of the slot table, wt_objects_reduce and wt_objects_compact over device channels of a width x rows range on the launch stream, then
 * the read-back of the summary and of min(objects, capacity) records; waits.  The caller has checked the arguments (wt_objects_check).  The
 * kernels are integer work compiled into both units; the build in use launches its own copy. */
void run_objects(Impl* I, const uint32_t* ids, const float* depth, uint32_t width, uint32_t rows, uint32_t first_row, const clw_rect* rect,
                 const uint32_t counts[3], clw_object_stat* out, uint32_t capacity, clw_object_summary* summary, bool timed) {
    static_assert(sizeof(clw_object_stat) == 48 && sizeof(clw_object_summary) == 16 && sizeof(clw_rect) == 16, "the table's ABI");
    uint32_t clip[4];
    (void)wt_objects_clip(width, rows, first_row, rect, clip);      /* a rectangle that misses the range: clip = 0 -> nothing reduced, an empty table */
    Impl::Objects& O = I->obj;
    O.size_table(counts[0] + counts[1] + counts[2] + 1u);
    {
        LaunchTimer t(I, CLW_TIMING_OBJECTS, timed);
        hipError_t e = (I->strict ? wt_strict_launch_objects : wt_fast_launch_objects)(ids, (const unsigned*)depth, width, rows, first_row, clip, counts,
                                                                                       O.table, O.result, I->stream);
        if (e != hipSuccess) die("Couldn't run the kernel");
        t.done();
    }
    clw_object_summary h;
    if (hipMemcpyAsync(&h, O.result, sizeof h, hipMemcpyDeviceToHost, I->stream) != hipSuccess) die("Failed to transfer device memory to host");
    finish(I);
    const uint32_t n = !out ? 0u : h.objects < capacity ? h.objects : capacity;
    if (n) {
        if (n > O.slots) die("The device kernel failed");      /* (more records than slots cannot be) */
        if (hipMemcpyAsync(out, (const uint8_t*)O.result + sizeof h, (size_t)n * sizeof(clw_object_stat), hipMemcpyDeviceToHost, I->stream) != hipSuccess)
            die("Failed to transfer device memory to host");
        finish(I);
    }
    *summary = h;
}

} /* namespace */

/* ======================================================================================== */
extern "C" {

void cl_wrap_init(cl_wrap* wrap, cl_device_type type, ...) {
    memset(wrap, 0, sizeof *wrap);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) die("Cannot find a HIP platform");
    if (!(type & (CL_DEVICE_TYPE_GPU | CL_DEVICE_TYPE_DEFAULT)) || count <= 0)
        die("Cannot find a device of the given type");

    Impl* I = new Impl();
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) cur = 0;
    I->device = env_int("CLWRAP_DEVICE", cur);
    if (I->device < 0 || I->device >= count) die("Cannot find a device of the given type");
    HIP_OK(hipSetDevice(I->device), "Could not create a HIP context from device");

    va_list vars;
    va_start(vars, type);
    const char* path = va_arg(vars, const char*);
    while (path) {
        const char* name = va_arg(vars, const char*);
        if (!name) { va_end(vars); die("Source file was not followed by kernel name"); }
        if (I->kernels.size() >= __MAX_KERNELS) { va_end(vars); die("Too many kernels"); }
        Kernel k;
        k.name = name;
        /* kernels are precompiled: identity comes from the NAME, the source path is not read */
        if (k.name == "raygen") k.kind = K_RAYGEN;
        else if (k.name == "raytracer") k.kind = K_RAYTRACER;
        else { va_end(vars); die("Couldn't create the CL kernel from: %s", name); }
        I->kernels.push_back(k);
        path = va_arg(vars, const char*);
    }
    va_end(vars);

    HIP_OK(hipStreamCreateWithFlags(&I->own_stream, hipStreamNonBlocking), "Couldn't create a command queue for the given device");
    I->stream = I->own_stream;
    I->depth = env_int("CLWRAP_DEPTH", 15);
    if (I->depth < 1 || I->depth > CLW_MAX_DEPTH) die("CLWRAP_DEPTH must be in [1, %d]", CLW_MAX_DEPTH);
    I->strict = env_int("CLWRAP_STRICT", 0) ? 1 : 0;
    I->fuse = env_int("CLWRAP_FUSE", 1) ? 1 : 0;
    I->variant = env_int("CLWRAP_VARIANT", 0);
    I->timing_every = (uint32_t)env_int("CLWRAP_TIMING_EVERY", 1);
    if (I->timing_every == 0) I->timing_every = 1;
    I->pipeline = env_int("CLWRAP_PIPELINE", 1) ? 1 : 0;
    I->supersample = env_int("CLWRAP_SUPERSAMPLE", 1);
    if (I->supersample != 1 && I->supersample != 2 && I->supersample != 4 && I->supersample != 8) die("CLWRAP_SUPERSAMPLE (supersampling factor) must be 1, 2, 4 or 8");
    if (const char* ad = getenv("CLWRAP_ADAPTIVE")) {
        if (*ad) {
            char* end = nullptr;
            const long v = strtol(ad, &end, 10);
            if (end == ad || *end || v < 0 || v > 256) die("CLWRAP_ADAPTIVE (adaptive supersampling: contrast threshold) must be an integer in [0, 256]");
            I->adaptive = (int)v;
        }
    }
    if (const char* so = getenv("CLWRAP_SEED_OFFSET")) {
        if (*so) {
            char* end = nullptr;
            const unsigned long long v = strtoull(so, &end, 0);
            if (end == so || *end || *so == '-' || v > 0xFFFFFFFFull) die("CLWRAP_SEED_OFFSET (seed offset of every trace launch) must be an integer in [0, 4294967295]");
            I->seed_offset = (uint32_t)v;
        }
    }
    I->acc_max = env_int("CLWRAP_ACCUMULATE", 0);
    if (I->acc_max < 0 || I->acc_max > 65536) die("CLWRAP_ACCUMULATE (frames a still view accumulates) must be in [0, 65536]");
    I->acc_jitter = env_int("CLWRAP_ACC_JITTER", 1);
    if (I->acc_jitter != 0 && I->acc_jitter != 1) die("CLWRAP_ACC_JITTER (sub-pixel offset per accumulated frame) must be 0 or 1");
    I->aperture = env_float("CLWRAP_APERTURE", 0.0f);
    I->focus = env_float("CLWRAP_FOCUS", 1.0f);
    if (!(I->aperture >= 0.0f) || !std::isfinite(I->aperture)) die("CLWRAP_APERTURE (lens aperture) must be a finite number >= 0");
    if (!(I->focus > 0.0f) || !std::isfinite(I->focus)) die("CLWRAP_FOCUS (lens focus distance) must be a finite number > 0");
    if (const char* pm = getenv("CLWRAP_PROJECTION")) {
        if (*pm) {
            if (!strcmp(pm, "ortho")) I->proj.model = CLW_PROJ_ORTHO;
            else if (!strcmp(pm, "equirect")) I->proj.model = CLW_PROJ_EQUIRECT;
            else if (strcmp(pm, "perspective")) die("CLWRAP_PROJECTION (camera model) must be ortho or equirect (or perspective, the default)");
        }
    }
    if (const char* ow = getenv("CLWRAP_ORTHO_WIDTH")) {
        if (*ow) {
            char* end = nullptr;
            const float v = strtof(ow, &end);
            if (end == ow || *end || !std::isfinite(v) || v < 0.0f) die("CLWRAP_ORTHO_WIDTH (world units an orthographic frame's width spans) must be a finite number >= 0");
            I->proj.ortho_width = v;
        }
    }
    if (const char* ps = getenv("CLWRAP_PANO_SPAN")) {
        if (*ps) {
            char *end = nullptr, *end2 = nullptr;
            const float h = strtof(ps, &end);
            const float v = (end != ps && *end == ',') ? strtof(end + 1, &end2) : 0.0f;
            if (end == ps || *end != ',' || end2 == end + 1 || !end2 || *end2 || !std::isfinite(h) || !std::isfinite(v) || h < 0.0f || h > 360.0f || v < 0.0f || v > 180.0f)
                die("CLWRAP_PANO_SPAN (degrees a panorama covers) must be <h>,<v> with h in [0, 360] and v in [0, 180] (0 = 360 / 180)");
            I->proj.h_span = h; I->proj.v_span = v;
        }
    }
    I->stamps = env_int("CLWRAP_STAMPS", 0) ? 1 : 0;
    if (const char* th = getenv("CLWRAP_THROUGH")) { if (*th) I->through = (float)atof(th); }
    I->occ_tiles_per_depth = (unsigned)env_int("CLWRAP_OCC_TILES_PER_DEPTH", (int)WT_OCC_TILES_PER_DEPTH);
    I->tpt_max = (unsigned)env_int("CLWRAP_TPT_MAX", (int)WT_TPT_MAX_LANES);
    I->tpt_min = (unsigned)env_int("CLWRAP_TPT_MIN", (int)WT_TPT_MIN_PATHS);
    I->tpt_pool_mb = (unsigned)env_int("CLWRAP_TPT_POOL_MB", (int)WT_TPT_POOL_MB);
    I->split_min_quota = (unsigned)env_int("CLWRAP_SPLIT_MIN_QUOTA", (int)WT_SPLIT_MIN_QUOTA);
    I->tpt_clock = env_int("CLWRAP_TPT_CLOCK", 0) ? 1 : 0;
    I->split_slots = (unsigned)std::max(1, env_int("CLWRAP_SPLIT_SLOTS", (int)WT_SPLIT_SLOTS));

    wrap->impl = I;
    wrap->kernels_num = (cl_uint)I->kernels.size();
}

void cl_wrap_load_global_data(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, const void* data,
                              size_t size, cl_mem_flags mem_flags) {
    (void)mem_flags;
    Impl* I = impl_of(wrap);
    use_device(I);
    precheck_buffer_arg(wrap, kernel_id, arg_id);
    Buffer* b = new_buffer(I);
    b->size = size;
    if (kernel_id < I->kernels.size() && I->kernels[kernel_id].kind == K_RAYTRACER && arg_id >= 1 && arg_id <= 9) I->acc.epoch++;
    if (data) {
        ensure_allocated(I, b);
        if (size) {
            if (hipMemcpy(b->dptr, data, size, hipMemcpyHostToDevice) != hipSuccess)
                die("Couldn't transfer the data from host to the device");
            if (size <= (64u << 20)) b->shadow.assign((const uint8_t*)data, (const uint8_t*)data + size);
        }
    } else {
        b->lazy = true; /* e.g. the 64 B/pixel ray buffer: stays virtual unless somebody needs the bytes */
    }
    register_buffer(wrap, kernel_id, arg_id, b);
}

void cl_wrap_load_single_data(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, const void* data, size_t obj_size) {
    Impl* I = impl_of(wrap);
    check_kernel_id(wrap, kernel_id);
    if (arg_id < __MAX_BUFFERS && is_registered(wrap, kernel_id, arg_id)) die("Given kernel argument already in use");
    if (arg_id >= __MAX_BUFFERS || !data || obj_size == 0 || obj_size > sizeof(ArgValue::bytes))
        die("Couldn't pass the data argument to the kernel");
    ArgValue& v = I->kernels[kernel_id].values[arg_id];
    if (I->kernels[kernel_id].kind == K_RAYTRACER && arg_id >= 1 && arg_id <= 9) I->acc.epoch++;      /* (an accumulated view starts again) */
    memcpy(v.bytes, data, obj_size); /* copied at call time, like clSetKernelArg */
    v.size = obj_size;
    v.set = true;
}

static void install_images(cl_wrap* wrap, Impl* I, cl_uint kernel_id, cl_uint arg_id, const uint8_t* rgba,
                           uint32_t w, uint32_t h, uint32_t layers) {
    Buffer* b = new_buffer(I);
    b->size = (size_t)w * h * layers * 4;
    b->image = true; b->w = w; b->h = h; b->layers = layers;
    if (b->size == 0) die("Couldn't create an image array %d", -40);
    ensure_allocated(I, b);
    if (hipMemcpy(b->dptr, rgba, b->size, hipMemcpyHostToDevice) != hipSuccess)
        die("Couldn't create an image array %d", -1);
    if (I->kernels[kernel_id].kind == K_RAYTRACER && arg_id >= 1 && arg_id <= 9) I->acc.epoch++;
    register_buffer(wrap, kernel_id, arg_id, b);
}

void cl_wrap_load_images(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, cl_mem_flags mem_flags,
                         cl_uint image_num, ...) {
    (void)mem_flags;
    Impl* I = impl_of(wrap);
    use_device(I);
    precheck_buffer_arg(wrap, kernel_id, arg_id);
    std::vector<uint8_t> all;
    uint32_t W = 0, H = 0;
    va_list vars;
    va_start(vars, image_num);
    for (cl_uint i = 0; i < image_num; i++) {
        const char* filename = va_arg(vars, const char*);
        uint32_t w = 0, h = 0;
        uint8_t* px = nullptr;
        int rc = wpng_read_rgba(filename, &w, &h, &px);
        switch (rc) { /* the reference's messages (opencl_wrap.c:233-307) */
            case WPNG_OK: break;
            case WPNG_ERR_OPEN: va_end(vars); die("Cannot open file \"%s\"", filename);
            case WPNG_ERR_NOT_PNG: va_end(vars); die("\"%s\" is not a PNG file", filename);
            case WPNG_ERR_FORMAT: va_end(vars); die("\"%s\" must have a depth of 8 bits and be RGB", filename);
            default: va_end(vars); die("Could not decode PNG file \"%s\" (code %d)", filename, rc);
        }
        if (i == 0) { W = w; H = h; all.reserve((size_t)w * h * 4 * image_num); }
        if (w != W || h != H) { free(px); va_end(vars); die("All images must have same dimensions"); }
        all.insert(all.end(), px, px + (size_t)w * h * 4);
        free(px);
    }
    va_end(vars);
    install_images(wrap, I, kernel_id, arg_id, all.data(), W, H, image_num);
}

void cl_wrap_output(cl_wrap* wrap, size_t array_size, size_t output_size, cl_uint kernel_run_id,
                    cl_uint kernel_id, cl_int arg_id, void* host_output) {
    Impl* I = impl_of(wrap);
    use_device(I);
    check_kernel_id(wrap, kernel_run_id);
    if (I->kernels[kernel_run_id].kind == K_RAYGEN) run_raygen(wrap, I, kernel_run_id, array_size);
    else if (pipelined_output(wrap, I, array_size, output_size, kernel_run_id, kernel_id, arg_id, host_output)) return;
    else run_raytracer(wrap, I, kernel_run_id, array_size);

    if (!host_output) {
        if (!I->async) finish(I);
        return;
    }
    /* blocking device -> host copy of buffers[kernel_id][arg_id] (opencl_wrap.c:390-397) */
    check_kernel_id(wrap, kernel_id);
    if (arg_id < 0 || arg_id >= __MAX_BUFFERS || !is_registered(wrap, kernel_id, (cl_uint)arg_id))
        die("Failed to transfer device memory to host");
    Buffer* b = (Buffer*)wrap->buffers[kernel_id][arg_id];
    materialise_rays(I, b);
    ensure_allocated(I, b);
    if (output_size > b->size) die("Failed to transfer device memory to host");
    if (output_size &&
        hipMemcpyAsync(host_output, b->dptr, output_size, hipMemcpyDeviceToHost, I->stream) != hipSuccess)
        die("Failed to transfer device memory to host");
    finish(I);
}

void cl_wrap_release(cl_wrap* wrap) {
    if (!wrap || !wrap->impl) return;
    Impl* I = (Impl*)wrap->impl;
    use_device(I);
    (void)hipStreamSynchronize(I->stream);
    for (Buffer* b : I->live) {
        if (b->owned && b->dptr) (void)hipFree(b->dptr);
        delete b;
    }
    if (I->d_geom) (void)hipFree(I->d_geom);
    if (I->d_ptex) (void)hipFree(I->d_ptex);
    if (I->d_counters) (void)hipFree(I->d_counters);
    if (I->d_tpt_pool) (void)hipFree(I->d_tpt_pool);
    if (I->d_tpt_flags) (void)hipFree(I->d_tpt_flags);
    if (I->d_tpt_jump) (void)hipFree(I->d_tpt_jump);
    if (I->d_cams) (void)hipFree(I->d_cams);
    if (I->d_motion) (void)hipFree(I->d_motion);
    if (I->acc.sum) (void)hipFree(I->acc.sum);
    I->gb.free_channels();
    if (I->gb.pick) (void)hipFree(I->gb.pick);
    if (I->gb.done) (void)hipEventDestroy(I->gb.done);
    I->ov.free_buffers();
    if (I->ov.done) (void)hipEventDestroy(I->ov.done);
    I->obj.free_buffers();
    I->ao.free_buffers();
    if (I->ao.dirs) (void)hipFree(I->ao.dirs);
    if (I->ao.done) (void)hipEventDestroy(I->ao.done);
    I->cast.free_buffers();
    I->ptab.free_all();
    I->adapt.free_all();
    if (I->tables_fence) (void)hipEventDestroy(I->tables_fence);
    for (uint32_t* q : {I->d_grid_start, I->d_grid_items, I->d_grid_box}) if (q) (void)hipFree(q);
    if (I->d_grid_geom) (void)hipFree(I->d_grid_geom);
    if (I->sched_stream) (void)hipStreamSynchronize(I->sched_stream);
    for (auto& sc : I->scheds) sc.free_all();
    if (I->sched_stream) (void)hipStreamDestroy(I->sched_stream);
    if (I->copy_stream) (void)hipStreamDestroy(I->copy_stream);
    for (hipEvent_t e : I->chunk_done) if (e) (void)hipEventDestroy(e);
    for (auto& t : I->timing) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    for (auto& p : I->free_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (I->own_stream) (void)hipStreamDestroy(I->own_stream);
    delete I;
    memset(wrap, 0, sizeof *wrap);
}

/* ---------------------------------- extensions ------------------------------------------ */
void clw_ext_set_depth(cl_wrap* wrap, int depth) {
    if (depth < 1 || depth > CLW_MAX_DEPTH) die("Trace depth must be in [1, %d]", CLW_MAX_DEPTH);
    impl_of(wrap)->depth = depth;
}
int clw_ext_get_depth(const cl_wrap* wrap) { return impl_of(wrap)->depth; }
void clw_ext_set_strict(cl_wrap* wrap, int strict) { impl_of(wrap)->strict = strict ? 1 : 0; }
void clw_ext_set_fuse(cl_wrap* wrap, int fuse) { impl_of(wrap)->fuse = fuse ? 1 : 0; }
void clw_ext_set_id_offset(cl_wrap* wrap, uint64_t first_id) { impl_of(wrap)->id_offset = first_id; }
void clw_ext_set_row_bands(cl_wrap* wrap, uint32_t stride, uint32_t phase) {
    if (stride == 0 || phase >= stride) die("Row bands need 0 <= phase < stride");
    Impl* I = impl_of(wrap);
    I->band_stride = stride; I->band_phase = phase;
}
void clw_ext_set_async(cl_wrap* wrap, int async) { impl_of(wrap)->async = async ? 1 : 0; }
void clw_ext_sync(cl_wrap* wrap) { Impl* I = impl_of(wrap); use_device(I); finish(I); }
void clw_ext_set_stream(cl_wrap* wrap, void* hip_stream) {
    Impl* I = impl_of(wrap);
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : I->own_stream;
    if (next != I->stream && I->tables_in_flight) {   /* the sample-camera / moving-sphere tables and an adaptive launch's tile list were written / are read in the old stream's order: fence them */
        use_device(I);
        if (!I->tables_fence) HIP_OK(hipEventCreateWithFlags(&I->tables_fence, hipEventDisableTiming), "Couldn't create a timing event");
        HIP_OK(hipEventRecord(I->tables_fence, I->stream), "Couldn't run the kernel");
        I->tables_fence_pending = true; I->tables_in_flight = false;
    }
    I->stream = next;
}
void clw_ext_unit(cl_wrap* wrap, int op, const float* in, uint32_t stride_in, float* out, uint32_t stride_out, uint32_t n,
                  uint32_t aux) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (n == 0) return;
    float *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc((void**)&din, (size_t)n * stride_in * 4), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dout, (size_t)n * stride_out * 4), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(din, in, (size_t)n * stride_in * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemset(dout, 0, (size_t)n * stride_out * 4), "Couldn't allocate device memory");
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    hipError_t e = I->strict ? wt_strict_launch_unit(op, din, dout, n, stride_in, stride_out, aux, I->stream)
                             : wt_fast_launch_unit(op, din, dout, n, stride_in, stride_out, aux, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    finish(I);
    HIP_OK(hipMemcpy(out, dout, (size_t)n * stride_out * 4, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(din); (void)hipFree(dout);
}
void clw_ext_unit_scene(cl_wrap* wrap, cl_uint kernel_id, int op, const float* in, uint32_t stride_in, float* out,
                        uint32_t stride_out, uint32_t n) {
    Impl* I = impl_of(wrap);
    use_device(I);
    check_kernel_id(wrap, kernel_id);
    if (I->kernels[kernel_id].kind != K_RAYTRACER) die("Wrong kernel ID given");
    if (n == 0) return;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    bind_scene(wrap, I, kernel_id, P, flags, dyn_lds);
    P.depth = I->depth;
    float *din = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc((void**)&din, (size_t)n * stride_in * 4), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dout, (size_t)n * stride_out * 4), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(din, in, (size_t)n * stride_in * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemset(dout, 0, (size_t)n * stride_out * 4), "Couldn't allocate device memory");
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    hipError_t e = I->strict ? wt_strict_launch_unit_scene(&P, flags, op, din, dout, n, stride_in, stride_out, dyn_lds, I->stream)
                             : wt_fast_launch_unit_scene(&P, flags, op, din, dout, n, stride_in, stride_out, dyn_lds, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    finish(I);
    HIP_OK(hipMemcpy(out, dout, (size_t)n * stride_out * 4, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(din); (void)hipFree(dout);
}
uint32_t clw_ext_read_tile_costs(cl_wrap* wrap, uint32_t* out, uint32_t capacity) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    const Impl::Sched& S = I->scheds[0];
    if (!S.cost[0]) return 0;
    uint32_t n = ((S.rows + 7) / 8) * ((S.w + 7) / 8);
    if (out && capacity >= n) HIP_OK(hipMemcpy(out, S.cost[S.o.wr ^ 1], (size_t)n * 4, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    return n;
}
uint32_t clw_ext_read_tile_order(cl_wrap* wrap, uint32_t* out, uint32_t capacity, uint32_t* per_share_cap) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    if (I->sched_stream) HIP_OK(hipStreamSynchronize(I->sched_stream), "The device kernel failed");
    const Impl::Sched& S = I->scheds[0];
    if (per_share_cap) *per_share_cap = 0;
    if (S.last_rd < 0 || !S.order[S.last_rd]) return 0;
    if (per_share_cap) *per_share_cap = S.cap;
    const uint32_t n = 8u * S.cap;
    if (out && capacity >= n) HIP_OK(hipMemcpy(out, S.order[S.last_rd], (size_t)n * 4, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    return n;
}
uint32_t clw_ext_unit_sched(cl_wrap* wrap, const uint32_t* cost, uint32_t tpr, uint32_t trows, int clamp_outliers, uint32_t per_share_cap,
                            uint32_t split_slots, uint32_t min_quota, uint32_t max_lg, uint32_t* out, uint32_t out_words) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (tpr == 0 || trows == 0 || tpr > 0xFFFu || trows > 0xFFFu || max_lg > 4u) die("clw_ext_unit_sched: %u x %u tiles, max_lg %u", tpr, trows, max_lg);
    const uint32_t per_share = ((trows + 7u) / 8u) * tpr;
    if (per_share_cap < per_share) die("clw_ext_unit_sched: per_share_cap %u is below the %u tiles of a share", per_share_cap, per_share);
    const uint64_t words = 8ull * ((uint64_t)per_share << max_lg) + 8ull * per_share_cap;
    if (words > 0xFFFFFFFFull) die("clw_ext_unit_sched: the table is too large");
    if (!out || out_words < words) return (uint32_t)words;
    const size_t ntiles = (size_t)trows * tpr;
    unsigned *dcost = nullptr, *dorder = nullptr;
    HIP_OK(hipMalloc((void**)&dcost, ntiles * 4), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dorder, (size_t)words * 4), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(dcost, cost, ntiles * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    std::vector<uint32_t> fill((size_t)words, CLW_SCHED_SENTINEL);
    HIP_OK(hipMemcpy(dorder, fill.data(), (size_t)words * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    if (wt_fast_launch_sched(dcost, dorder, tpr, trows, per_share, clamp_outliers ? 1u : 0u, per_share_cap, split_slots, min_quota, max_lg, I->stream) != hipSuccess)
        die("Couldn't run the kernel");
    finish(I);
    HIP_OK(hipMemcpy(out, dorder, (size_t)words * 4, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(dcost); (void)hipFree(dorder);
    return (uint32_t)words;
}
void clw_ext_set_split(cl_wrap* wrap, int slots, int min_quota) {
    Impl* I = impl_of(wrap);
    if (slots >= 0) I->split_slots = (unsigned)std::max(1, slots);
    if (min_quota >= 0) I->split_min_quota = (unsigned)min_quota;
    for (auto& sc : I->scheds) sc.reset();
}
void clw_ext_get_split(const cl_wrap* wrap, uint32_t* slots, uint32_t* min_quota, uint32_t* extra_per_share) {
    const Impl* I = impl_of(wrap);
    if (slots) *slots = I->split_slots;
    if (min_quota) *min_quota = I->split_min_quota;
    if (extra_per_share) *extra_per_share = WT_SPLIT_EXTRA_PER_SHARE;
}
void clw_ext_set_shadow_through(cl_wrap* wrap, float factor) { impl_of(wrap)->through = factor; }
void clw_ext_set_grid(cl_wrap* wrap, int on) { impl_of(wrap)->use_grid = on ? 1 : 0; }
int clw_ext_get_grid(const cl_wrap* wrap, clw_grid_info* out) {
    const Impl* I = impl_of(wrap);
    if (!I->d_geom || !out) return 0;
    memset(out, 0, sizeof *out);
    if (!I->grid_ok) return 1;
    out->built = 1; out->pair = I->grid_pair ? 1 : 0;
    out->ncells = I->grid.ncells; out->pairs = (uint64_t)I->grid_pairs; out->reg_pad = I->grid.reg_pad;
    for (int a = 0; a < 3; a++) { out->res[a] = I->grid.res[a]; out->cell[a] = I->grid.cell[a]; out->gmin[a] = I->grid.gmin[a]; }
    return 1;
}
void clw_ext_set_grid_pair(cl_wrap* wrap, int on) {
    if (on < -1 || on > 1) die("The grid's shadow walk must be -1 (default), 0 (single) or 1 (paired)");
    Impl* I = impl_of(wrap);
    I->grid_pair_req = on;
    I->prep_s = I->prep_p = I->prep_l = nullptr;      /* the next launch prepares the scene again, as clw_ext_invalidate_scene makes it */
    I->acc.epoch++;
}
void clw_ext_set_tile_sched(cl_wrap* wrap, int on) { Impl* I = impl_of(wrap); I->sched = on ? 1 : 0; for (auto& sc : I->scheds) sc.reset(); }
void clw_ext_set_variant(cl_wrap* wrap, int variant) { impl_of(wrap)->variant = variant; }
int clw_ext_last_trace_flags(cl_wrap* wrap) { return impl_of(wrap)->last_trace_flags; }
void clw_ext_set_tpt(cl_wrap* wrap, int max_lanes, int min_paths, int pool_mb) {
    Impl* I = impl_of(wrap);
    if (max_lanes >= 0) I->tpt_max = (unsigned)std::min(max_lanes, 64);
    if (min_paths >= 0) I->tpt_min = (unsigned)min_paths;
    if (pool_mb >= 0) I->tpt_pool_mb = (unsigned)pool_mb;
}
void clw_ext_get_tpt(const cl_wrap* wrap, uint32_t* max_lanes, uint32_t* min_paths, uint32_t* pool_mb) {
    const Impl* I = impl_of(wrap);
    if (max_lanes) *max_lanes = I->tpt_max;
    if (min_paths) *min_paths = I->tpt_min;
    if (pool_mb) *pool_mb = I->tpt_pool_mb;
}
void clw_ext_set_debug_rgb(cl_wrap* wrap, void* p) { impl_of(wrap)->debug_rgb = (float*)p; }
void clw_ext_set_supersample(cl_wrap* wrap, int n) {
    if (n != 1 && n != 2 && n != 4 && n != 8) die("The supersampling factor must be 1, 2, 4 or 8");
    impl_of(wrap)->supersample = n;
}
int clw_ext_get_supersample(const cl_wrap* wrap) { return impl_of(wrap)->supersample; }
void clw_ext_set_adaptive(cl_wrap* wrap, int threshold) {
    if (threshold < -1 || threshold > 256) die("The adaptive supersampling threshold must be in [0, 256], or -1 for off");
    impl_of(wrap)->adaptive = threshold;
}
int clw_ext_get_adaptive(const cl_wrap* wrap) { return impl_of(wrap)->adaptive; }
uint32_t clw_ext_read_refine_mask(cl_wrap* wrap, uint8_t* out, uint32_t cap) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    const uint32_t n = I->adapt.blocks;
    if (out && n && cap >= n) HIP_OK(hipMemcpy(out, I->adapt.mask, n, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    return n;
}
void clw_ext_set_sample_cameras(cl_wrap* wrap, const clw_sample_camera* cams, uint32_t count) {
    Impl* I = impl_of(wrap);
    if (cams && count) I->cams.assign(cams, cams + count); else I->cams.clear();
    I->aperture = 0.0f;     /* the table and the lens are alternatives: the later call wins */
}
uint32_t clw_ext_get_sample_cameras(const cl_wrap* wrap, clw_sample_camera* out, uint32_t cap) {
    const Impl* I = impl_of(wrap);
    const uint32_t n = (uint32_t)I->cams_used.size();
    if (out && n && cap >= n) memcpy(out, I->cams_used.data(), (size_t)n * sizeof(clw_sample_camera));
    return n;
}
void clw_ext_set_sphere_motion(cl_wrap* wrap, const float* disp, uint32_t ns, const float* times, uint32_t count) {
    Impl* I = impl_of(wrap);
    bool any = false;
    if (disp) for (size_t i = 0; i < 3 * (size_t)ns; i++) {
        if (!std::isfinite(disp[i])) die("Moving spheres: displacement %u of sphere %u is not finite", (unsigned)(i % 3), (unsigned)(i / 3));
        any |= disp[i] != 0.0f;
    }
    if (times) for (uint32_t k = 0; k < count; k++) if (!std::isfinite(times[k])) die("Moving spheres: sample time %u is not finite", (unsigned)k);
    I->motion_disp.clear(); I->motion_times.clear(); I->motion_explicit_times = false;
    if (!any) return;                            /* no table, or nothing moves: the plain launch */
    I->motion_disp.assign(disp, disp + 3 * (size_t)ns);
    if (times) { I->motion_times.assign(times, times + count); I->motion_explicit_times = true; }   /* a count that is not n * n, 0 included, is refused at the launch */
}
uint32_t clw_ext_get_sample_times(const cl_wrap* wrap, float* out, uint32_t cap) {
    const Impl* I = impl_of(wrap);
    const uint32_t n = (uint32_t)I->times_used.size();
    if (out && n && cap >= n) memcpy(out, I->times_used.data(), (size_t)n * sizeof(float));
    return n;
}
void clw_ext_set_lens(cl_wrap* wrap, float aperture, float focus) {
    if (!(aperture >= 0.0f) || !std::isfinite(aperture)) die("The lens aperture must be a finite number >= 0");
    if (!(focus > 0.0f) || !std::isfinite(focus)) die("The lens focus distance must be a finite number > 0");
    Impl* I = impl_of(wrap);
    I->aperture = aperture; I->focus = focus;
    I->cams.clear();
}

void clw_ext_set_seed_offset(cl_wrap* wrap, uint32_t s) { impl_of(wrap)->seed_offset = s; }
uint32_t clw_ext_get_seed_offset(const cl_wrap* wrap) { return impl_of(wrap)->seed_offset; }
void clw_ext_set_accumulate(cl_wrap* wrap, int max_frames, int jitter) {
    if (max_frames < 0 || max_frames > 65536) die("Frame accumulation: the number of frames must be in [0, 65536] (0 = off)");
    if (jitter != 0 && jitter != 1) die("Frame accumulation: jitter must be 0 or 1");
    Impl* I = impl_of(wrap);
    I->acc_max = max_frames; I->acc_jitter = jitter;
}
uint32_t clw_ext_get_accumulated(cl_wrap* wrap) { Impl* I = impl_of(wrap); return I->acc_max > 0 ? I->acc.K : 0u; }
void clw_ext_reset_accumulation(cl_wrap* wrap) { impl_of(wrap)->acc.epoch++; }

void clw_ext_set_projection(cl_wrap* wrap, const clw_projection* proj) {
    Impl* I = impl_of(wrap);
    clw_projection p{};
    if (proj && proj->model != CLW_PROJ_PERSPECTIVE) {
        p = *proj;
        if (p.model > CLW_PROJ_EQUIRECT) die("The projection model must be CLW_PROJ_PERSPECTIVE, CLW_PROJ_ORTHO or CLW_PROJ_EQUIRECT");
        if (p.reserved != 0u) die("The projection's reserved word must be 0");
        if (!std::isfinite(p.axis[0]) || !std::isfinite(p.axis[1]) || !std::isfinite(p.axis[2])) die("The projection's axis must be finite");
        if (!std::isfinite(p.ortho_width) || p.ortho_width < 0.0f) die("The projection's ortho_width must be a finite number >= 0");
        if (!std::isfinite(p.h_span) || p.h_span < 0.0f || p.h_span > 360.0f || !std::isfinite(p.v_span) || p.v_span < 0.0f || p.v_span > 180.0f)
            die("The projection's spans must be in [0, 360] and [0, 180] degrees (0 = 360 / 180)");
    }
    I->proj = p;      /* (the pinhole is stored as all zero, whatever else the caller's struct held) */
}
void clw_ext_get_projection(const cl_wrap* wrap, clw_projection* out) { if (out) *out = impl_of(wrap)->proj; }

int clw_ext_unit_projection(cl_wrap* wrap, const clw_camera* cam, const clw_projection* proj, uint64_t id_begin, uint64_t id_end, float* out_rays) {
    Impl* I = impl_of(wrap);
    use_device(I);
    wt_projection T;
    if (!out_rays || !wt_projection_terms(cam, proj, &T) || T.model == CLW_PROJ_PERSPECTIVE) return 0;
    const uint64_t total = (uint64_t)cam->width * cam->height;
    if (id_begin >= id_end || id_end > total || id_end - id_begin > 0x03FFFFFFull) return 0;      /* (64 n bytes in 32 bits) */
    const uint32_t n = (uint32_t)(id_end - id_begin);
    float *drays = nullptr, *dcol = nullptr, *drow = nullptr;
    if (T.model == CLW_PROJ_EQUIRECT) {
        std::vector<float> col(4 * (size_t)cam->width), row(4 * (size_t)cam->height);
        if (!clw_host_projection_tables(cam, proj, col.data(), row.data())) return 0;
        HIP_OK(hipMalloc((void**)&dcol, col.size() * sizeof(float)), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&drow, row.size() * sizeof(float)), "Couldn't allocate device memory");
        HIP_OK(hipMemcpy(dcol, col.data(), col.size() * sizeof(float), hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
        HIP_OK(hipMemcpy(drow, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
        T.col = dcol; T.row = drow;
    }
    HIP_OK(hipMalloc((void**)&drays, (size_t)n * 64), "Couldn't allocate device memory");
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    raygen_params P{};
    P.width = cam->width; P.height = cam->height; P.id_offset = id_begin; P.n_items = n; P.rays = drays; P.band_stride = 1; P.band_phase = 0;
    hipError_t e = (I->strict ? wt_strict_launch_raygen_proj : wt_fast_launch_raygen_proj)(&P, &T, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    finish(I);
    HIP_OK(hipMemcpy(out_rays, drays, (size_t)n * 64, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(drays);
    if (dcol) (void)hipFree(dcol);
    if (drow) (void)hipFree(drow);
    return 1;
}

uint32_t clw_ext_render_gbuffer(cl_wrap* wrap, uint32_t channels) {
    Impl* I = impl_of(wrap);
    use_device(I);
    channels &= CLW_GB_ALL;
    if (!channels) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    wt_projection T;
    if (!gbuffer_params(wrap, I, P, flags, dyn_lds, T)) return 0;
    Impl::GBuffer& B = I->gb;
    if (B.n != P.n_items) {      /* another range: a pass under way may still write the old buffers */
        if (B.n) { finish(I); if (B.done) (void)hipEventSynchronize(B.done); }
        B.free_channels();
        B.n = P.n_items;
    }
    void* chan[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int c = 0; c < 5; c++) {
        if (!(channels & (1u << c))) continue;
        if (!B.chan[c]) HIP_OK(hipMalloc(&B.chan[c], (size_t)B.n * GB_WORDS[c] * 4), "Couldn't allocate device memory");
        chan[c] = B.chan[c];
    }
    launch_gbuffer(I, P, flags, dyn_lds, chan, T, true);
    if (!B.done) HIP_OK(hipEventCreateWithFlags(&B.done, hipEventDisableTiming), "Couldn't create a timing event");
    HIP_OK(hipEventRecord(B.done, I->stream), "Couldn't run the kernel");
    B.written = channels;
    return B.n;
}

uint32_t clw_ext_read_gbuffer(cl_wrap* wrap, uint32_t channel, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::GBuffer& B = I->gb;
    const int c = gbuffer_channel(channel);
    if (c < 0 || !(B.written & channel) || !B.chan[c]) return 0;
    const uint64_t bytes = (uint64_t)B.n * GB_WORDS[c] * 4;
    if (bytes > 0xFFFFFFFFull) return 0;
    if (out && capacity_bytes >= bytes) {
        hipError_t e = hipEventSynchronize(B.done);
        if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
        HIP_OK(hipMemcpy(out, B.chan[c], (size_t)bytes, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    }
    return (uint32_t)bytes;
}

void* clw_ext_gbuffer_device_ptr(cl_wrap* wrap, uint32_t channel) {
    const Impl::GBuffer& B = impl_of(wrap)->gb;
    const int c = gbuffer_channel(channel);
    return (c < 0 || !(B.written & channel)) ? nullptr : B.chan[c];
}

int clw_ext_pick(cl_wrap* wrap, uint32_t x, uint32_t y, clw_pick* out) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!out) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    wt_projection T;
    if (!gbuffer_params(wrap, I, P, flags, dyn_lds, T)) return 0;
    if (x >= P.width || y >= P.height) return 0;
    /* is the pixel one of the wrapper's work-items? */
    if (P.band_stride > 1u) {
        const uint32_t band = y / 8u;
        if (band % P.band_stride != P.band_phase) return 0;
        const uint64_t item = (uint64_t)((band / P.band_stride) * 8u + y % 8u) * P.width + x;
        if (item >= P.n_items) return 0;
    } else {
        const uint64_t id = (uint64_t)y * P.width + x;
        if (id < P.id_offset || id - P.id_offset >= P.n_items) return 0;
    }
    /* the same kernel on the one-pixel range [id, id + 1): a linear range, whose work-item takes (id % W, id / W) = (x, y) */
    P.id_offset = (uint64_t)y * P.width + x; P.n_items = 1;
    P.band_stride = 1; P.band_phase = 0; P.tiled = 0; P.rows = 0; P.row_offset = y;
    Impl::GBuffer& B = I->gb;
    if (!B.pick) HIP_OK(hipMalloc((void**)&B.pick, sizeof(clw_pick)), "Couldn't allocate device memory");
    static_assert(sizeof(clw_pick) == 44, "clw_pick is 11 words");
    void* chan[5] = {B.pick + 1, B.pick + 0, B.pick + 5, B.pick + 2, B.pick + 8};      /* depth, id, normal, point, albedo as clw_pick lays them out */
    launch_gbuffer(I, P, flags, dyn_lds, chan, T, false);
    clw_pick h;
    if (hipMemcpyAsync(&h, B.pick, sizeof h, hipMemcpyDeviceToHost, I->stream) != hipSuccess) die("Failed to transfer device memory to host");
    finish(I);
    *out = h;
    return 1;
}

uint32_t clw_ext_render_overlay(cl_wrap* wrap, const clw_overlay* style, const uint32_t* sel, uint32_t count) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_overlay_check(style, sel, count)) return 0;
    if (I->band_stride > 1u) return 0;
    cl_uint kid = 0;
    while (kid < I->kernels.size() && I->kernels[kid].kind != K_RAYTRACER) kid++;
    if (kid >= I->kernels.size() || !is_registered(wrap, kid, 10)) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    wt_projection T;
    if (!gbuffer_params(wrap, I, P, flags, dyn_lds, T)) return 0;
    /* whole rows of one contiguous range: work-item i is pixel (i % width, i / width) of the range's own image */
    if (P.band_stride > 1u || !P.tiled || P.rows == 0u) return 0;
    Buffer* fb = (Buffer*)wrap->buffers[kid][10];
    if (fb->size < (size_t)P.n_items * 4) return 0;
    ensure_allocated(I, fb);
    Impl::Overlay& O = I->ov;
    if (O.n != P.n_items) {      /* another range: a pass under way may still use the old buffers */
        if (O.n) { finish(I); if (O.done) (void)hipEventSynchronize(O.done); }
        O.free_buffers();
        HIP_OK(hipMalloc((void**)&O.ids, (size_t)P.n_items * 4), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&O.frame, (size_t)P.n_items * 4), "Couldn't allocate device memory");
        O.n = P.n_items;
    }
    void* chan[5] = {nullptr, O.ids, nullptr, nullptr, nullptr};
    launch_gbuffer(I, P, flags, dyn_lds, chan, T, true);
    launch_overlay(I, (const uint32_t*)fb->dptr, O.ids, O.frame, P.width, P.rows, *style, sel, count, true);
    if (!O.done) HIP_OK(hipEventCreateWithFlags(&O.done, hipEventDisableTiming), "Couldn't create a timing event");
    HIP_OK(hipEventRecord(O.done, I->stream), "Couldn't run the kernel");
    O.written = true;
    return O.n;
}

uint32_t clw_ext_read_overlay(cl_wrap* wrap, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::Overlay& O = I->ov;
    if (!O.written) return 0;
    const uint64_t bytes = (uint64_t)O.n * 4;
    if (bytes > 0xFFFFFFFFull) return 0;
    if (out && capacity_bytes >= bytes) {
        hipError_t e = hipEventSynchronize(O.done);
        if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
        HIP_OK(hipMemcpy(out, O.frame, (size_t)bytes, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    }
    return (uint32_t)bytes;
}

void* clw_ext_overlay_device_ptr(cl_wrap* wrap) {
    const Impl::Overlay& O = impl_of(wrap)->ov;
    return O.written ? O.frame : nullptr;
}

uint32_t clw_ext_unit_overlay(cl_wrap* wrap, const uint32_t* frame, const uint32_t* ids, uint32_t width, uint32_t rows, const clw_overlay* style,
                              const uint32_t* sel, uint32_t count, uint32_t* out) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_overlay_check(style, sel, count) || width == 0u || rows == 0u || !frame || !ids || !out) return 0;
    const uint64_t n = (uint64_t)width * rows;
    if (n > 0x3FFFFFFFull) return 0;      /* (4 n bytes per buffer in 32 bits) */
    const size_t bytes = (size_t)n * 4;
    uint32_t *dframe = nullptr, *dids = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc((void**)&dframe, bytes), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dids, bytes), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dout, bytes), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(dframe, frame, bytes, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemcpy(dids, ids, bytes, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    launch_overlay(I, dframe, dids, dout, width, rows, *style, sel, count, false);
    finish(I);
    HIP_OK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(dframe); (void)hipFree(dids); (void)hipFree(dout);
    return (uint32_t)n;
}

int clw_ext_object_stats(cl_wrap* wrap, const clw_rect* rect, clw_object_stat* out, uint32_t capacity, clw_object_summary* summary) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!summary || I->band_stride > 1u) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    wt_projection T;
    if (!gbuffer_params(wrap, I, P, flags, dyn_lds, T)) return 0;
    /* whole rows of one contiguous range: work-item i is pixel (i % width, row_offset + i / width) of the frame */
    if (P.band_stride > 1u || !P.tiled || P.rows == 0u) return 0;
    const uint32_t counts[3] = {P.ns, P.np, P.nl};
    Impl::Objects& O = I->obj;
    if (!wt_objects_check(&O, P.width, P.rows, P.row_offset, rect, counts, summary)) return 0;      /* (the ids are the pass's own: any non-NULL pointer) */
    O.size_range(P.n_items);
    void* chan[5] = {O.depth, O.ids, nullptr, nullptr, nullptr};
    launch_gbuffer(I, P, flags, dyn_lds, chan, T, true);
    run_objects(I, O.ids, O.depth, P.width, P.rows, P.row_offset, rect, counts, out, capacity, summary, true);
    return 1;
}

int clw_ext_unit_object_stats(cl_wrap* wrap, const uint32_t* ids, const float* depth, uint32_t width, uint32_t rows, uint32_t first_row,
                              const clw_rect* rect, const uint32_t counts[3], clw_object_stat* out, uint32_t capacity, clw_object_summary* summary) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_objects_check(ids, width, rows, first_row, rect, counts, summary)) return 0;
    const size_t bytes = (size_t)width * rows * 4;      /* (width * rows fits 30 bits) */
    uint32_t* dids = nullptr;
    float* ddepth = nullptr;
    HIP_OK(hipMalloc((void**)&dids, bytes), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(dids, ids, bytes, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    if (depth) {
        HIP_OK(hipMalloc((void**)&ddepth, bytes), "Couldn't allocate device memory");
        HIP_OK(hipMemcpy(ddepth, depth, bytes, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    }
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    run_objects(I, dids, ddepth, width, rows, first_row, rect, counts, out, capacity, summary, false);
    (void)hipFree(dids);
    if (ddepth) (void)hipFree(ddepth);
    return 1;
}

uint32_t clw_ext_render_ao(cl_wrap* wrap, const clw_ao* ao) {
    Impl* I = impl_of(wrap);
    use_device(I);
    static_assert(sizeof(clw_ao) == 16, "the pass's ABI");
    if (!wt_ao_check(ao)) return 0;
    if (I->band_stride > 1u) return 0;
    cl_uint kid = 0;
    while (kid < I->kernels.size() && I->kernels[kid].kind != K_RAYTRACER) kid++;
    if (kid >= I->kernels.size()) return 0;
    const bool compose = (ao->flags & CLW_AO_COMPOSE) != 0u;
    if (compose && !is_registered(wrap, kid, 10)) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    wt_projection T;
    if (!gbuffer_params(wrap, I, P, flags, dyn_lds, T)) return 0;
    /* whole rows of one contiguous range: work-item i is pixel (i % width, row_offset + i / width) of the frame */
    if (P.band_stride > 1u || !P.tiled || P.rows == 0u || !wt_ao_range_ok(P.width, P.rows)) return 0;
    Buffer* fb = nullptr;
    if (compose) {
        fb = (Buffer*)wrap->buffers[kid][10];
        if (fb->size < (size_t)P.n_items * 4) return 0;
        ensure_allocated(I, fb);
    }
    Impl::AO& O = I->ao;
    if (O.n != P.n_items) {      /* another range: a pass under way may still use the old buffers */
        if (O.n) { finish(I); if (O.done) (void)hipEventSynchronize(O.done); }
        O.free_buffers();
        HIP_OK(hipMalloc((void**)&O.point, (size_t)P.n_items * 12), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&O.normal, (size_t)P.n_items * 12), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&O.ids, (size_t)P.n_items * 4), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&O.open, (size_t)P.n_items), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&O.frame, (size_t)P.n_items * 4), "Couldn't allocate device memory");
        O.n = P.n_items;
    }
    void* chan[5] = {nullptr, O.ids, O.normal, O.point, nullptr};
    launch_gbuffer(I, P, flags, dyn_lds, chan, T, true);
    launch_ao_trace(I, P, flags, O.point, O.normal, O.ids, P.width, P.rows, P.row_offset, *ao, O.open, true);
    launch_ao_resolve(I, O.open, O.ids, compose ? (const uint32_t*)fb->dptr : nullptr, O.frame, P.width, P.rows, *ao, true);
    if (!O.done) HIP_OK(hipEventCreateWithFlags(&O.done, hipEventDisableTiming), "Couldn't create a timing event");
    HIP_OK(hipEventRecord(O.done, I->stream), "Couldn't run the kernel");
    O.written = true;
    return O.n;
}

uint32_t clw_ext_read_ao(cl_wrap* wrap, uint32_t what, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::AO& O = I->ao;
    if (!O.written || what > 1u) return 0;
    const uint64_t bytes = (uint64_t)O.n * (what == 0u ? 4u : 1u);      /* (n < 2^30) */
    if (out && capacity_bytes >= bytes) {
        hipError_t e = hipEventSynchronize(O.done);
        if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
        HIP_OK(hipMemcpy(out, what == 0u ? (const void*)O.frame : (const void*)O.open, (size_t)bytes, hipMemcpyDeviceToHost),
               "Failed to transfer device memory to host");
    }
    return (uint32_t)bytes;
}

void* clw_ext_ao_device_ptr(cl_wrap* wrap, uint32_t what) {
    const Impl::AO& O = impl_of(wrap)->ao;
    if (!O.written || what > 1u) return nullptr;
    return what == 0u ? (void*)O.frame : (void*)O.open;
}

uint32_t clw_ext_unit_ao_open(cl_wrap* wrap, const float* point, const float* normal, const uint32_t* ids, uint32_t width, uint32_t rows,
                              uint32_t first_row, const clw_ao* ao, uint8_t* open_u8) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_ao_check(ao) || !wt_ao_range_ok(width, rows) || !point || !normal || !ids || !open_u8) return 0;
    /* the wrapper's bound scene, as gbuffer_params asks for it */
    cl_uint kid = 0;
    while (kid < I->kernels.size() && I->kernels[kid].kind != K_RAYTRACER) kid++;
    if (kid >= I->kernels.size()) return 0;
    for (cl_uint a : {1u, 2u, 3u, 8u, 9u}) if (!is_registered(wrap, kid, a)) return 0;
    for (cl_uint a : {4u, 5u, 6u}) if (!I->kernels[kid].values[a].set) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    bind_scene(wrap, I, kid, P, flags, dyn_lds);
    const size_t n = (size_t)width * rows;
    float *dpoint = nullptr, *dnormal = nullptr;
    uint32_t* dids = nullptr;
    uint8_t* dopen = nullptr;
    HIP_OK(hipMalloc((void**)&dpoint, n * 12), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dnormal, n * 12), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dids, n * 4), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dopen, n), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(dpoint, point, n * 12, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemcpy(dnormal, normal, n * 12, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemcpy(dids, ids, n * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    launch_ao_trace(I, P, flags, dpoint, dnormal, dids, width, rows, first_row, *ao, dopen, false);
    finish(I);
    HIP_OK(hipMemcpy(open_u8, dopen, n, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(dpoint); (void)hipFree(dnormal); (void)hipFree(dids); (void)hipFree(dopen);
    return (uint32_t)n;
}

uint32_t clw_ext_unit_ao_resolve(cl_wrap* wrap, const uint8_t* open_u8, const uint32_t* ids, const uint32_t* frame, uint32_t width, uint32_t rows,
                                 const clw_ao* ao, uint32_t* out) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_ao_check(ao) || !wt_ao_range_ok(width, rows) || !open_u8 || !ids || !out || ((ao->flags & CLW_AO_COMPOSE) && !frame)) return 0;
    const size_t n = (size_t)width * rows;
    uint8_t* dopen = nullptr;
    uint32_t *dids = nullptr, *dframe = nullptr, *dout = nullptr;
    HIP_OK(hipMalloc((void**)&dopen, n), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dids, n * 4), "Couldn't allocate device memory");
    HIP_OK(hipMalloc((void**)&dout, n * 4), "Couldn't allocate device memory");
    HIP_OK(hipMemcpy(dopen, open_u8, n, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    HIP_OK(hipMemcpy(dids, ids, n * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    if (ao->flags & CLW_AO_COMPOSE) {
        HIP_OK(hipMalloc((void**)&dframe, n * 4), "Couldn't allocate device memory");
        HIP_OK(hipMemcpy(dframe, frame, n * 4, hipMemcpyHostToDevice), "Couldn't transfer the data from host to the device");
    }
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    launch_ao_resolve(I, dopen, dids, dframe, dout, width, rows, *ao, false);
    finish(I);
    HIP_OK(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    (void)hipFree(dopen); (void)hipFree(dids); (void)hipFree(dout);
    if (dframe) (void)hipFree(dframe);
    return (uint32_t)n;
}

uint32_t clw_ext_cast_rays(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, clw_hit* hits) {
    if (!hits) return 0;
    return cast_host_arrays(wrap, rays, n, flags, hits, nullptr);
}

uint32_t clw_ext_occluded_rays(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, uint8_t* blocked) {
    if (!blocked) return 0;
    return cast_host_arrays(wrap, rays, n, flags, nullptr, blocked);
}

uint32_t clw_ext_cast_rays_device(cl_wrap* wrap, const void* d_rays, uint32_t n, uint32_t flags, void* d_hits, void* d_blocked) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_cast_check(n, flags) || !d_rays || (d_hits != nullptr) == (d_blocked != nullptr)) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!cast_params(wrap, I, n, P, cc)) return 0;
    launch_cast(I, P, cc, d_rays, n, flags, d_hits, (uint8_t*)d_blocked);
    return n;
}

void clw_ext_set_pipeline(cl_wrap* wrap, int on) { impl_of(wrap)->pipeline = on ? 1 : 0; }
void clw_ext_set_timing_every(cl_wrap* wrap, uint32_t n) { Impl* I = impl_of(wrap); I->timing_every = n ? n : 1; I->timing_tick = 0; I->timing_on = n != 0; }

void clw_ext_timing_reset(cl_wrap* wrap) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    for (auto& t : I->timing) I->free_events.push_back({t.start, t.stop});
    I->timing.clear();
    I->timing_on = true;
}

void clw_ext_timing_get(cl_wrap* wrap, cl_uint kernel_id, uint32_t* launches, double* total_ms) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    uint32_t n = 0;
    double sum = 0.0;
    for (auto& t : I->timing) {
        if (t.kernel != kernel_id) continue;
        float ms = 0.0f;
        HIP_OK(hipEventElapsedTime(&ms, t.start, t.stop), "Couldn't read a timing event");
        sum += ms;
        n++;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = sum;
}

void clw_ext_load_images_raw(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, const uint8_t* rgba,
                             uint32_t width, uint32_t height, uint32_t layers) {
    Impl* I = impl_of(wrap);
    use_device(I);
    precheck_buffer_arg(wrap, kernel_id, arg_id);
    if (!rgba) die("Couldn't create an image array %d", -37);
    install_images(wrap, I, kernel_id, arg_id, rgba, width, height, layers);
}

void clw_ext_bind_device_buffer(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id, void* device_ptr, size_t size) {
    Impl* I = impl_of(wrap);
    precheck_buffer_arg(wrap, kernel_id, arg_id);
    if (!device_ptr) die("Couldn't pass the data argument to the kernel");
    Buffer* b = new_buffer(I);
    b->dptr = device_ptr; b->size = size; b->owned = false;
    if (I->kernels[kernel_id].kind == K_RAYTRACER && arg_id >= 1 && arg_id <= 10) I->acc.epoch++;      /* scene arrays, images, the framebuffer */
    register_buffer(wrap, kernel_id, arg_id, b);
}

void clw_ext_invalidate_scene(cl_wrap* wrap) {
    Impl* I = impl_of(wrap);
    I->prep_s = I->prep_p = I->prep_l = nullptr;
    I->acc.epoch++;
    /* a scene buffer rewritten in place on the device no longer matches its host copy */
    for (Buffer* b : I->live) if (!b->image) b->shadow.clear();
}

void* clw_ext_device_ptr(cl_wrap* wrap, cl_uint kernel_id, cl_uint arg_id) {
    Impl* I = impl_of(wrap);
    use_device(I);
    check_kernel_id(wrap, kernel_id);
    if (arg_id >= __MAX_BUFFERS || !is_registered(wrap, kernel_id, arg_id)) die("Wrong kernel ID given");
    Buffer* b = (Buffer*)wrap->buffers[kernel_id][arg_id];
    materialise_rays(I, b);
    ensure_allocated(I, b);
    if (b->gen_valid) b->exposed = true;
    return b->dptr;
}

void clw_ext_enable_counters(cl_wrap* wrap, int enable) { impl_of(wrap)->counting = enable ? 1 : 0; }

void clw_ext_read_counters_ex(cl_wrap* wrap, uint64_t* out, uint32_t n) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    for (uint32_t k = 0; k < n; k++) out[k] = 0;
    if (!I->d_counters) return;
    std::vector<unsigned long long> h(COUNTER_WORDS);
    HIP_OK(hipMemcpy(h.data(), I->d_counters, COUNTER_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    HIP_OK(hipMemsetAsync(I->d_counters, 0, COUNTER_WORDS * sizeof(unsigned long long), I->stream), "Couldn't allocate device memory");
    finish(I);
    for (size_t sh = 0; sh < CLW_STAMP_SHARDS; sh++)        /* stamp shards of the diagnostic build -> words 16.. */
        for (int k = 0; k < 16; k++) h[16 + k] += h[CLW_NUM_COUNTERS + 16 * sh + k];
    for (uint32_t k = 0; k < n && k < CLW_NUM_COUNTERS; k++) out[k] = h[k];
}
void clw_ext_read_counters(cl_wrap* wrap, uint64_t out[8]) { clw_ext_read_counters_ex(wrap, out, 8); }

int clw_host_write_png(const char* path, const uint32_t* xrgb, uint32_t width, uint32_t height) {
    return wpng_write_xrgb(path, xrgb, width, height, 1);
}
int clw_host_write_png_rgba(const char* path, const uint8_t* rgba, uint32_t width, uint32_t height) {
    return wpng_write_rgba_as_rgb(path, rgba, width, height, 1);
}
int clw_host_read_png(const char* path, uint32_t* width, uint32_t* height, uint8_t** rgba_malloced) {
    return wpng_read_rgba(path, width, height, rgba_malloced);
}
void clw_host_free(void* p) { free(p); }

#ifndef WT_SOURCE_HASH
#define WT_SOURCE_HASH "unknown"
#endif
const char* clw_ext_version(void) { return "opencl_wrap_hip 0.2 gfx950 fast+strict kernels:" WT_SOURCE_HASH; }

} /* extern "C" */
