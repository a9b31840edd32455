/*
 * hip_wrap_passes.cpp -- the passes beside the trace launch (include/hip_wrap_ext.h): the primary-hit pass and the pick, the selection
 * overlay, the visible-object table, ambient occlusion, the ray queries, the layered ray queries and the path queries.  Same conventions as hip_wrap.cpp; the shared internals are
 * hip_wrap_impl.h's.
 */
#include "hip_wrap_impl.h"

using namespace clw;

namespace {

/* ---- range-sized pass buffers (Impl::GBuffer, Overlay, AO and the range half of Objects) ------------------------------------------------- */
/* The buffers follow the pass's range.  Another range: a pass under way may still use the old buffers, and with async launches nothing but
 * `done` says when it has finished -- so wait for the launch stream and for `done` (the pass may have run on an earlier stream), then free,
 * then allocate.  `done` null = the owner waits for its own work in every call (Objects): nothing can be in flight. */
template <class B> void range_resize(Impl* I, B& b, uint32_t items, hipEvent_t done) {
    if (b.n == items) return;
    if (b.n && done) { finish(I); (void)hipEventSynchronize(done); }
    b.free_buffers();
    b.alloc_buffers(items);
    b.n = items;
}

/* behind a pass's last launch: the event is created on first use and recorded on the launch stream */
void range_mark_done(Impl* I, Impl::RangePass& b, uint32_t written) {
    if (!b.done) HIP_OK(hipEventCreateWithFlags(&b.done, hipEventDisableTiming), "Couldn't create a timing event");
    HIP_OK(hipEventRecord(b.done, I->stream), "Couldn't run the kernel");
    b.written = written;
}

/* The read-back of `src`, `item_bytes` per work-item of the range: -> the byte count, 0 when 32 bits do not hold it; copied, behind a wait for
 * the pass, when `out` has room for it */
uint32_t range_read(const Impl::RangePass& b, const void* src, uint32_t item_bytes, void* out, uint32_t capacity_bytes) {
    const uint64_t bytes = (uint64_t)b.n * item_bytes;
    if (bytes > 0xFFFFFFFFull) return 0;
    if (out && capacity_bytes >= bytes) {
        hipError_t e = hipEventSynchronize(b.done);
        if (e != hipSuccess) { printf("%d\n", (int)e); die("The device kernel failed"); }
        HIP_OK(hipMemcpy(out, src, (size_t)bytes, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    }
    return (uint32_t)bytes;
}

/* ---- the primary-hit pass -------------------------------------------------------------------------------------------------------- */
constexpr uint32_t GB_WORDS[5] = {1, 1, 3, 3, 3};      /* 4-byte words per work-item of the channels depth, id, normal, point, albedo */

/* the raytracer kernel's id, or -1: the wrapper has none */
int raytracer_kernel(const Impl* I) {
    cl_uint kid = 0;
    while (kid < I->kernels.size() && I->kernels[kid].kind != K_RAYTRACER) kid++;
    return kid < I->kernels.size() ? (int)kid : -1;
}

/* is a scene bound to raytracer kernel `kid`: the arrays (arguments 1, 2, 3) registered and their counts (4, 5, 6) set; `images`: and the
 * textures and the skybox (8, 9), which a launch that shades reads and a query does not */
bool scene_bound(const cl_wrap* w, const Impl* I, cl_uint kid, bool images) {
    for (cl_uint a : {1u, 2u, 3u}) if (!is_registered(w, kid, a)) return false;
    if (images) for (cl_uint a : {8u, 9u}) if (!is_registered(w, kid, a)) return false;
    for (cl_uint a : {4u, 5u, 6u}) if (!I->kernels[kid].values[a].set) return false;
    return true;
}

/* What a primary-hit pass launches over: the range the next trace launch would cover -- the camera and range the raygen launch latched, clipped
 * by the raytracer's `pixels` argument, bands included -- on the scene as bind_scene binds it, under the wrapper's camera model. */
struct PassRange {
    cl_uint kid; whitted_params P; int flags; size_t dyn_lds;
    wt_projection T;      /* model 0: the pinhole */
    Buffer* fb;           /* the framebuffer (argument 10), for a caller that asked for it with RANGE_FRAME; not yet allocated if it was created lazily */
};
/* what a caller needs of the range: whole rows of one contiguous range (work-item i is pixel (i % width, row_offset + i / width) of the frame);
 * the framebuffer of argument 10, holding the range's 4 * n_items bytes */
enum { RANGE_ROWS = 1, RANGE_FRAME = 2 };

/* Fills `R`, or refuses: false when there is no raytracer kernel, no latched camera, no bound scene or no work-item yet, when the projection
 * does not resolve, or when the range is not what the caller needs -- the callers return 0 then, they do not terminate the process, and have
 * neither allocated nor launched anything of their own (a refusal after the scene was looked at may have prepared it). */
bool pass_range(cl_wrap* w, Impl* I, unsigned needs, PassRange& R) {
    R = PassRange{};
    const int kid = raytracer_kernel(I);
    if (kid < 0 || ((needs & RANGE_ROWS) && I->band_stride > 1u) || ((needs & RANGE_FRAME) && !is_registered(w, kid, 10))) return false;
    R.kid = (cl_uint)kid;
    Buffer* rays = find_rays(w, I, R.kid);
    uint32_t total;
    if (!rays || !rays->gen_valid || !scene_bound(w, I, R.kid, true) || !find_total(I->kernels[kid], total)) return false;
    const RaygenArgs& g = rays->gen;
    const uint32_t n = g.n_items < total ? g.n_items : total;
    if (n == 0) return false;
    if (I->proj.model != CLW_PROJ_PERSPECTIVE && !resolve_projection(I, g, R.T)) return false;      /* (before anything is bound or launched) */
    whitted_params& P = R.P;
    bind_scene(w, I, R.kid, P, R.flags, R.dyn_lds);
    wt_plan_fused_range(&g, n, &P);      /* as the fused trace launch: the rays are this library's own */
    if (R.T.model != CLW_PROJ_PERSPECTIVE) P.unit_dirs = 0u;      /* as the trace launch of a projected view: no direction is taken for unit */
    P.vis = 0;
    if ((needs & RANGE_ROWS) && (P.band_stride > 1u || !P.tiled || P.rows == 0u)) return false;
    if (needs & RANGE_FRAME) {
        R.fb = (Buffer*)w->buffers[kid][10];
        if (R.fb->size < (size_t)P.n_items * 4) return false;
    }
    return true;
}

void launch_gbuffer(Impl* I, const PassRange& R, void* const chan[5], bool timed) {
    const unsigned grid = wt_plan_grid(&R.P);      /* as trace_launch: tile rows dealt to the 8 XCDs */
    LaunchTimer t(I, CLW_TIMING_GBUFFER, timed);
    hipError_t e = WT_LAUNCH(I, gbuffer)(&R.P, R.flags, grid, R.dyn_lds, (float*)chan[0], (unsigned*)chan[1], (float*)chan[2], (float*)chan[3],
                                         (float*)chan[4], &R.T, I->stream);
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
    const int kid = raytracer_kernel(I);
    if (kid < 0 || !scene_bound(w, I, kid, false)) return false;
    const Kernel& k = I->kernels[kid];
    Buffer* bs = (Buffer*)w->buffers[kid][1];
    Buffer* bp = (Buffer*)w->buffers[kid][2];
    Buffer* bl = (Buffer*)w->buffers[kid][3];
    prepare_scene(I, bs, read_count(k, 4), bp, read_count(k, 5), bl, read_count(k, 6));
    cc = wt_plan_cast(I->variant, I->prep_ns, (uint32_t)I->geom_f4, I->grid_ok && I->use_grid, n, (uint32_t)std::max(0, env_int("CLWRAP_CAST_BATCHES", 0)));   /* CLWRAP_CAST_BATCHES: tuning knob */
    if (cc.groups == 0u) return false;
    bind_geometry(I, P, cc.flags);
    return true;
}

/* wt_cast over device memory on the launch stream; exactly one of hits / blocked */
void launch_cast(Impl* I, const whitted_params& P, const wt_cast_class& cc, const void* rays, uint32_t n, uint32_t flags, void* hits, uint8_t* blocked) {
    LaunchTimer t(I, CLW_TIMING_CAST, true);
    hipError_t e = WT_LAUNCH(I, cast)(&P, cc.flags, cc.groups, cc.batches, cc.dyn_lds, rays, n, flags, hits, blocked, I->stream);
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
    void* d_rays = C.rays.reserve((size_t)n * sizeof(clw_ray));
    void* d_out = hits ? C.hits.reserve((size_t)n * sizeof(clw_hit)) : C.blocked.reserve((size_t)n);
    HIP_OK(hipMemcpyAsync(d_rays, rays, (size_t)n * sizeof(clw_ray), hipMemcpyHostToDevice, I->stream), "Couldn't transfer the data from host to the device");
    launch_cast(I, P, cc, d_rays, n, flags, hits ? d_out : nullptr, hits ? nullptr : (uint8_t*)d_out);
    if (hits) HIP_OK(hipMemcpyAsync(hits, d_out, (size_t)n * sizeof(clw_hit), hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    else HIP_OK(hipMemcpyAsync(blocked, d_out, (size_t)n, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    finish(I);
    return n;
}

/* ---- layered ray queries ------------------------------------------------------------------------------------------------------------ */
/* wt_cast_layers over device memory on the launch stream: K * n words into each of t and id.  CLWRAP_LAYERS_CAPACITY (4 or 8): tuning knob, the
 * compiled list capacity to run where both hold K; anything else = the smallest that does */
void launch_layers(Impl* I, const whitted_params& P, const wt_cast_class& cc, const void* rays, uint32_t n, uint32_t flags, uint32_t K, float* t,
                   uint32_t* id, bool timed) {
    const int want = env_int("CLWRAP_LAYERS_CAPACITY", 0);
    const unsigned capacity = ((want == 4 || want == 8) && (uint32_t)want >= K) ? (unsigned)want : 0u;
    LaunchTimer tm(I, CLW_TIMING_LAYERS, timed);
    hipError_t e = WT_LAUNCH(I, cast_layers)(&P, cc.flags, cc.dyn_lds, rays, n, flags, K, capacity, t, id, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    tm.done();
}

/* ---- proximity queries ---------------------------------------------------------------------------------------------------------------- */
/* The scene side of a proximity query of n probes: a ray query's (cast_params) under the plan wt_plan_near -- the grid only where every prepared
 * r * r word is finite.  CLWRAP_NEAR_BOX_CELLS: the cap on a probe's box, for tests and A/B runs.  false as cast_params. */
bool near_params(cl_wrap* w, Impl* I, uint32_t n, whitted_params& P, wt_near_class& nc) {
    wt_cast_class cc;
    if (!cast_params(w, I, n, P, cc)) return false;      /* (prepares the scene; its geometry class is chosen again below) */
    nc = wt_plan_near(I->variant, I->prep_ns, (uint32_t)I->geom_f4, I->grid_ok && I->use_grid && I->near_grid_ok, n, env_int("CLWRAP_NEAR_BOX_CELLS", -1));
    if (nc.groups == 0u) return false;
    P = whitted_params{};
    bind_geometry(I, P, nc.flags);
    return true;
}

/* wt_near over device memory on the launch stream; exactly one of hits / within / (d and id) */
void launch_near(Impl* I, const whitted_params& P, const wt_near_class& nc, const void* probes, const void* ignore, uint32_t n, uint32_t flags, uint32_t K,
                 void* hits, void* within, void* d, void* id) {
    LaunchTimer t(I, CLW_TIMING_NEAR, true);
    hipError_t e = WT_LAUNCH(I, near)(&P, nc.flags, nc.dyn_lds, nc.box_cells, probes, (const unsigned*)ignore, n, flags, K, hits, (unsigned char*)within,
                                      (float*)d, (unsigned*)id, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* the three host-array entry points: upload, launch, read back, all in the order of the launch stream, then wait.  K = 0: hits or within */
uint32_t near_host_arrays(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, uint32_t K, clw_hit* hits,
                          uint8_t* within, float* d, uint32_t* id) {
    Impl* I = impl_of(wrap);
    use_device(I);
    static_assert(sizeof(clw_probe) == 16, "the proximity queries' ABI");
    if (!(K ? wt_near_list_check(n, flags, K) : wt_near_check(n, flags)) || !probes) return 0;
    whitted_params P{};
    wt_near_class nc;
    if (!near_params(wrap, I, n, P, nc)) return 0;
    Impl::Near& B = I->near;
    const size_t words = (size_t)K * n;
    void* d_probes = B.probes.reserve((size_t)n * sizeof(clw_probe));
    void* d_ignore = ignore ? B.ignore.reserve((size_t)n * 4) : nullptr;
    void* d_out = K ? nullptr : B.out.reserve(hits ? (size_t)n * sizeof(clw_hit) : (size_t)n);
    void* d_d = K ? B.d.reserve(words * 4) : nullptr;
    void* d_id = K ? B.id.reserve(words * 4) : nullptr;
    HIP_OK(hipMemcpyAsync(d_probes, probes, (size_t)n * sizeof(clw_probe), hipMemcpyHostToDevice, I->stream), "Couldn't transfer the data from host to the device");
    if (ignore) HIP_OK(hipMemcpyAsync(d_ignore, ignore, (size_t)n * 4, hipMemcpyHostToDevice, I->stream), "Couldn't transfer the data from host to the device");
    launch_near(I, P, nc, d_probes, d_ignore, n, flags, K, hits ? d_out : nullptr, within ? d_out : nullptr, d_d, d_id);
    if (hits) HIP_OK(hipMemcpyAsync(hits, d_out, (size_t)n * sizeof(clw_hit), hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    else if (within) HIP_OK(hipMemcpyAsync(within, d_out, (size_t)n, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    else {
        HIP_OK(hipMemcpyAsync(d, d_d, words * 4, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
        HIP_OK(hipMemcpyAsync(id, d_id, words * 4, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    }
    finish(I);
    return n;
}

/* ---- path queries -------------------------------------------------------------------------------------------------------------------- */
/* The scene side of a path query of n rays: a ray query's (cast_params), and the bound sphere and plane arrays themselves, from which
 * wt_cast_paths reads the winner's material.  false as cast_params. */
bool paths_params(cl_wrap* w, Impl* I, uint32_t n, whitted_params& P, wt_cast_class& cc) {
    if (!cast_params(w, I, n, P, cc)) return false;
    const int kid = raytracer_kernel(I);
    Buffer* bs = (Buffer*)w->buffers[kid][1];
    Buffer* bp = (Buffer*)w->buffers[kid][2];
    ensure_allocated(I, bs); ensure_allocated(I, bp);
    P.spheres_raw = (const uint8_t*)bs->dptr; P.planes_raw = (const uint8_t*)bp->dptr;
    return true;
}

/* wt_cast_paths over device memory on the launch stream: bounces * n hits, n status bytes, n outgoing rays (next may be null) */
void launch_paths(Impl* I, const whitted_params& P, const wt_cast_class& cc, const void* rays, uint32_t n, uint32_t flags, uint32_t bounces, void* hits,
                  uint8_t* status, void* next, bool timed) {
    LaunchTimer tm(I, CLW_TIMING_PATHS, timed);
    hipError_t e = WT_LAUNCH(I, cast_paths)(&P, cc.flags, cc.dyn_lds, rays, n, flags, bounces, hits, status, next, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    tm.done();
}

/* What the camera-ray kernel launches over: the linear range the next trace launch would cover -- the camera and range the raygen launch
 * latched, clipped by the raytracer's `pixels` argument -- under the wrapper's camera model.  Needs no scene.  false (nothing launched; the
 * panorama's tables may have been resolved) without a raytracer kernel or a latched camera, with row bands, for a projection the definition
 * refuses, and for a range whose ids leave 32 bits. */
struct CameraRange { whitted_params P; wt_projection T; };
bool camera_range(cl_wrap* w, Impl* I, CameraRange& R) {
    R = CameraRange{};
    const int kid = raytracer_kernel(I);
    if (kid < 0 || I->band_stride > 1u) return false;
    Buffer* rays = find_rays(w, I, (cl_uint)kid);
    uint32_t total;
    if (!rays || !rays->gen_valid || !find_total(I->kernels[kid], total)) return false;
    const RaygenArgs& g = rays->gen;
    const uint32_t n = g.n_items < total ? g.n_items : total;
    if (n == 0 || n >= (1u << 30) || g.width == 0u || g.band_stride > 1u || g.id_offset + n > (1ull << 32)) return false;
    if (!resolve_projection(I, g, R.T)) return false;      /* (the pinhole too: what clw_host_camera_rays refuses) */
    wt_plan_fused_range(&g, n, &R.P);
    return true;
}

void launch_camera_rays(Impl* I, const CameraRange& R, void* rays, bool timed) {
    LaunchTimer t(I, CLW_TIMING_CAMRAYS, timed);
    hipError_t e = WT_LAUNCH(I, camera_rays)(&R.P, &R.T, rays, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* ---- the selection overlay ------------------------------------------------------------------------------------------------------- */
/* wt_overlay over a width x rows range on the launch stream; the caller has checked style and selection (wt_overlay_check).  The kernel is
 * integer work compiled into both units; the build in use launches its own copy. */
void launch_overlay(Impl* I, const uint32_t* frame, const uint32_t* ids, uint32_t* out, uint32_t width, uint32_t rows, const clw_overlay& st,
                    const uint32_t* sel, uint32_t count, bool timed) {
    const unsigned style[5] = {st.radius, st.outline_rgb, st.fill_rgb, st.fill_alpha, st.edge_rgb};
    LaunchTimer t(I, CLW_TIMING_OVERLAY, timed);
    hipError_t e = WT_LAUNCH(I, overlay)(frame, ids, out, width, rows, st.flags, style, sel, count, I->stream);
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
    hipError_t e = WT_LAUNCH(I, ao_trace)(&P, flags, point, normal, ids, dirs, open, width, rows, first_row, ao.rays, ao.radius, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

/* wt_ao_resolve likewise.  Integer work compiled into both units; the build in use launches its own copy. */
void launch_ao_resolve(Impl* I, const uint8_t* open, const uint32_t* ids, const uint32_t* frame, uint32_t* out, uint32_t width, uint32_t rows,
                       const clw_ao& ao, bool timed) {
    LaunchTimer t(I, CLW_TIMING_AO_RESOLVE, timed);
    hipError_t e = WT_LAUNCH(I, ao_resolve)(open, ids, frame, out, width, rows, ao.flags, ao.rays, ao.strength, I->stream);
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
        hipError_t e = WT_LAUNCH(I, objects)(ids, (const unsigned*)depth, width, rows, first_row, clip, counts, O.table, O.result, I->stream);
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

extern "C" {

uint32_t clw_ext_render_gbuffer(cl_wrap* wrap, uint32_t channels) {
    Impl* I = impl_of(wrap);
    use_device(I);
    channels &= CLW_GB_ALL;
    if (!channels) return 0;
    PassRange R;
    if (!pass_range(wrap, I, 0, R)) return 0;
    Impl::GBuffer& B = I->gb;
    range_resize(I, B, R.P.n_items, B.done);
    void* chan[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int c = 0; c < 5; c++) {
        if (!(channels & (1u << c))) continue;
        if (!B.chan[c]) HIP_OK(hipMalloc(&B.chan[c], (size_t)B.n * GB_WORDS[c] * 4), "Couldn't allocate device memory");
        chan[c] = B.chan[c];
    }
    launch_gbuffer(I, R, chan, true);
    range_mark_done(I, B, channels);
    return B.n;
}

uint32_t clw_ext_read_gbuffer(cl_wrap* wrap, uint32_t channel, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::GBuffer& B = I->gb;
    const int c = gbuffer_channel(channel);
    if (c < 0 || !(B.written & channel) || !B.chan[c]) return 0;
    return range_read(B, B.chan[c], GB_WORDS[c] * 4, out, capacity_bytes);
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
    PassRange R;
    if (!pass_range(wrap, I, 0, R)) return 0;
    whitted_params& P = R.P;
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
    launch_gbuffer(I, R, chan, false);
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
    PassRange R;      /* (work-item i is pixel (i % width, i / width) of the range's own image) */
    if (!pass_range(wrap, I, RANGE_ROWS | RANGE_FRAME, R)) return 0;
    const whitted_params& P = R.P;
    ensure_allocated(I, R.fb);
    Impl::Overlay& O = I->ov;
    range_resize(I, O, P.n_items, O.done);
    void* chan[5] = {nullptr, O.ids, nullptr, nullptr, nullptr};
    launch_gbuffer(I, R, chan, true);
    launch_overlay(I, (const uint32_t*)R.fb->dptr, O.ids, O.frame, P.width, P.rows, *style, sel, count, true);
    range_mark_done(I, O, 1);
    return O.n;
}

uint32_t clw_ext_read_overlay(cl_wrap* wrap, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::Overlay& O = I->ov;
    return O.written ? range_read(O, O.frame, 4, out, capacity_bytes) : 0;
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
    const DeviceTemp<uint32_t> dframe(frame, bytes), dids(ids, bytes), dout(bytes);
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    launch_overlay(I, dframe, dids, dout, width, rows, *style, sel, count, false);
    finish(I);
    dout.read(out, bytes);
    return (uint32_t)n;
}

int clw_ext_object_stats(cl_wrap* wrap, const clw_rect* rect, clw_object_stat* out, uint32_t capacity, clw_object_summary* summary) {
    Impl* I = impl_of(wrap);
    use_device(I);
    PassRange R;
    if (!summary || !pass_range(wrap, I, RANGE_ROWS, R)) return 0;
    const whitted_params& P = R.P;
    const uint32_t counts[3] = {P.ns, P.np, P.nl};
    Impl::Objects& O = I->obj;
    if (!wt_objects_check(&O, P.width, P.rows, P.row_offset, rect, counts, summary)) return 0;      /* (the ids are the pass's own: any non-NULL pointer) */
    range_resize(I, O, P.n_items, nullptr);
    void* chan[5] = {O.depth, O.ids, nullptr, nullptr, nullptr};
    launch_gbuffer(I, R, chan, true);
    run_objects(I, O.ids, O.depth, P.width, P.rows, P.row_offset, rect, counts, out, capacity, summary, true);
    return 1;
}

int clw_ext_unit_object_stats(cl_wrap* wrap, const uint32_t* ids, const float* depth, uint32_t width, uint32_t rows, uint32_t first_row,
                              const clw_rect* rect, const uint32_t counts[3], clw_object_stat* out, uint32_t capacity, clw_object_summary* summary) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_objects_check(ids, width, rows, first_row, rect, counts, summary)) return 0;
    const size_t bytes = (size_t)width * rows * 4;      /* (width * rows fits 30 bits) */
    const DeviceTemp<uint32_t> dids(ids, bytes);
    const DeviceTemp<float> ddepth(depth, bytes);      /* (optional) */
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    run_objects(I, dids, ddepth, width, rows, first_row, rect, counts, out, capacity, summary, false);
    return 1;
}

uint32_t clw_ext_render_ao(cl_wrap* wrap, const clw_ao* ao) {
    Impl* I = impl_of(wrap);
    use_device(I);
    static_assert(sizeof(clw_ao) == 16, "the pass's ABI");
    if (!wt_ao_check(ao)) return 0;
    const bool compose = (ao->flags & CLW_AO_COMPOSE) != 0u;
    PassRange R;
    if (!pass_range(wrap, I, RANGE_ROWS | (compose ? RANGE_FRAME : 0), R)) return 0;
    const whitted_params& P = R.P;
    if (!wt_ao_range_ok(P.width, P.rows)) return 0;
    if (compose) ensure_allocated(I, R.fb);
    Impl::AO& O = I->ao;
    range_resize(I, O, P.n_items, O.done);
    void* chan[5] = {nullptr, O.ids, O.normal, O.point, nullptr};
    launch_gbuffer(I, R, chan, true);
    launch_ao_trace(I, P, R.flags, O.point, O.normal, O.ids, P.width, P.rows, P.row_offset, *ao, O.open, true);
    launch_ao_resolve(I, O.open, O.ids, compose ? (const uint32_t*)R.fb->dptr : nullptr, O.frame, P.width, P.rows, *ao, true);
    range_mark_done(I, O, 1);
    return O.n;
}

uint32_t clw_ext_read_ao(cl_wrap* wrap, uint32_t what, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::AO& O = I->ao;
    if (!O.written || what > 1u) return 0;
    return what == 0u ? range_read(O, O.frame, 4, out, capacity_bytes) : range_read(O, O.open, 1, out, capacity_bytes);
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
    /* the wrapper's bound scene, as a primary-hit pass asks for it (pass_range); no camera, no range */
    const int kid = raytracer_kernel(I);
    if (kid < 0 || !scene_bound(wrap, I, kid, true)) return 0;
    whitted_params P{};
    int flags = 0;
    size_t dyn_lds = 0;
    bind_scene(wrap, I, kid, P, flags, dyn_lds);
    const size_t n = (size_t)width * rows;
    const DeviceTemp<float> dpoint(point, n * 12), dnormal(normal, n * 12);
    const DeviceTemp<uint32_t> dids(ids, n * 4);
    const DeviceTemp<uint8_t> dopen(n);
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    launch_ao_trace(I, P, flags, dpoint, dnormal, dids, width, rows, first_row, *ao, dopen, false);
    finish(I);
    dopen.read(open_u8, n);
    return (uint32_t)n;
}

uint32_t clw_ext_unit_ao_resolve(cl_wrap* wrap, const uint8_t* open_u8, const uint32_t* ids, const uint32_t* frame, uint32_t width, uint32_t rows,
                                 const clw_ao* ao, uint32_t* out) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_ao_check(ao) || !wt_ao_range_ok(width, rows) || !open_u8 || !ids || !out || ((ao->flags & CLW_AO_COMPOSE) && !frame)) return 0;
    const size_t n = (size_t)width * rows;
    const DeviceTemp<uint8_t> dopen(open_u8, n);
    const DeviceTemp<uint32_t> dids(ids, n * 4), dout(n * 4);
    const DeviceTemp<uint32_t> dframe((ao->flags & CLW_AO_COMPOSE) ? frame : nullptr, n * 4);      /* (read with COMPOSE only) */
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    launch_ao_resolve(I, dopen, dids, dframe, dout, width, rows, *ao, false);
    finish(I);
    dout.read(out, n * 4);
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

uint32_t clw_ext_cast_layers(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t K, float* t, uint32_t* id) {
    Impl* I = impl_of(wrap);
    use_device(I);
    static_assert(sizeof(clw_layer) == 8, "the layered queries' ABI");
    if (!wt_layers_check(n, flags, K) || !rays || !t || !id) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!cast_params(wrap, I, n, P, cc)) return 0;
    Impl::Layers& B = I->layers;
    const size_t words = (size_t)K * n;
    void* d_rays = B.h_rays.reserve((size_t)n * sizeof(clw_ray));
    float* d_t = (float*)B.h_t.reserve(words * 4);
    uint32_t* d_id = (uint32_t*)B.h_id.reserve(words * 4);
    HIP_OK(hipMemcpyAsync(d_rays, rays, (size_t)n * sizeof(clw_ray), hipMemcpyHostToDevice, I->stream), "Couldn't transfer the data from host to the device");
    launch_layers(I, P, cc, d_rays, n, flags, K, d_t, d_id, true);
    HIP_OK(hipMemcpyAsync(t, d_t, words * 4, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    HIP_OK(hipMemcpyAsync(id, d_id, words * 4, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    finish(I);
    return n;
}

uint32_t clw_ext_cast_layers_device(cl_wrap* wrap, const void* d_rays, uint32_t n, uint32_t flags, uint32_t K, void* d_t, void* d_id) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_layers_check(n, flags, K) || !d_rays || !d_t || !d_id) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!cast_params(wrap, I, n, P, cc)) return 0;
    launch_layers(I, P, cc, d_rays, n, flags, K, (float*)d_t, (uint32_t*)d_id, true);
    return n;
}

uint32_t clw_ext_camera_rays_device(cl_wrap* wrap, void* d_rays, uint32_t capacity) {
    Impl* I = impl_of(wrap);
    use_device(I);
    CameraRange R;
    if (!d_rays || !camera_range(wrap, I, R) || capacity < R.P.n_items) return 0;
    launch_camera_rays(I, R, d_rays, true);
    return R.P.n_items;
}

uint32_t clw_ext_camera_rays(cl_wrap* wrap, clw_ray* out, uint32_t capacity) {
    Impl* I = impl_of(wrap);
    use_device(I);
    CameraRange R;
    if (!out || !camera_range(wrap, I, R) || capacity < R.P.n_items) return 0;
    const uint32_t n = R.P.n_items;
    void* d_rays = I->layers.h_rays.reserve((size_t)n * sizeof(clw_ray));
    launch_camera_rays(I, R, d_rays, true);
    HIP_OK(hipMemcpyAsync(out, d_rays, (size_t)n * sizeof(clw_ray), hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    finish(I);
    return n;
}

uint32_t clw_ext_render_layers(cl_wrap* wrap, uint32_t flags, uint32_t K) {
    Impl* I = impl_of(wrap);
    use_device(I);
    CameraRange R;
    if (!wt_layers_check(1u, flags, K) || !camera_range(wrap, I, R)) return 0;
    const uint32_t n = R.P.n_items;
    whitted_params P{};
    wt_cast_class cc;
    if (!cast_params(wrap, I, n, P, cc)) return 0;
    Impl::Layers& B = I->layers;
    if (B.n != n || B.K < K) {      /* (as range_resize: a pass under way may still use the old buffers) */
        if (B.n && B.done) { finish(I); (void)hipEventSynchronize(B.done); }
        B.free_range();
        HIP_OK(hipMalloc(&B.rays, (size_t)n * sizeof(clw_ray)), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&B.t, (size_t)K * n * 4), "Couldn't allocate device memory");
        HIP_OK(hipMalloc((void**)&B.id, (size_t)K * n * 4), "Couldn't allocate device memory");
        B.n = n; B.K = K;
    }
    launch_camera_rays(I, R, B.rays, true);
    launch_layers(I, P, cc, B.rays, n, flags, K, B.t, B.id, true);
    range_mark_done(I, B, K);      /* (written: the layers the last pass left to read) */
    return n;
}

uint32_t clw_ext_read_layers(cl_wrap* wrap, uint32_t what, void* out, uint32_t capacity_bytes) {
    Impl* I = impl_of(wrap);
    use_device(I);
    const Impl::Layers& B = I->layers;
    if (!B.written || what > 1u) return 0;
    return range_read(B, what == 0u ? (const void*)B.t : (const void*)B.id, 4u * B.written, out, capacity_bytes);
}

void* clw_ext_layers_device_ptr(cl_wrap* wrap, uint32_t what) {
    const Impl::Layers& B = impl_of(wrap)->layers;
    if (!B.written || what > 1u) return nullptr;
    return what == 0u ? (void*)B.t : (void*)B.id;
}

int clw_ext_pick_layers(cl_wrap* wrap, uint32_t x, uint32_t y, uint32_t flags, uint32_t K, clw_layer* out) {
    Impl* I = impl_of(wrap);
    use_device(I);
    CameraRange R;
    if (!out || !wt_layers_check(1u, flags, K) || !camera_range(wrap, I, R)) return 0;
    if (x >= R.P.width || y >= R.P.height) return 0;
    const uint64_t pixel = (uint64_t)y * R.P.width + x;      /* is the pixel one of the wrapper's work-items? */
    if (pixel < R.P.id_offset || pixel - R.P.id_offset >= R.P.n_items) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!cast_params(wrap, I, 1u, P, cc)) return 0;
    /* the same two kernels on the one-pixel range [pixel, pixel + 1) */
    R.P.id_offset = pixel; R.P.n_items = 1; R.P.tiled = 0; R.P.rows = 0; R.P.row_offset = y;
    Impl::Layers& B = I->layers;
    constexpr uint32_t RAY_WORDS = sizeof(clw_ray) / 4;
    if (!B.pick) HIP_OK(hipMalloc((void**)&B.pick, (RAY_WORDS + 2 * WT_LAYERS_MAX) * 4), "Couldn't allocate device memory");
    float* dt = (float*)(B.pick + RAY_WORDS);
    uint32_t* did = B.pick + RAY_WORDS + WT_LAYERS_MAX;
    launch_camera_rays(I, R, B.pick, false);
    launch_layers(I, P, cc, B.pick, 1u, flags, K, dt, did, false);      /* (n = 1: layer k is word k) */
    uint32_t h[2 * WT_LAYERS_MAX];
    if (hipMemcpyAsync(h, dt, sizeof h, hipMemcpyDeviceToHost, I->stream) != hipSuccess) die("Failed to transfer device memory to host");
    finish(I);
    for (uint32_t k = 0; k < K; k++) { memcpy(&out[k].t, &h[k], 4); out[k].id = h[WT_LAYERS_MAX + k]; }
    return 1;
}

uint32_t clw_ext_nearest_surface(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, clw_hit* out) {
    if (!out) return 0;
    return near_host_arrays(wrap, probes, ignore, n, flags, 0u, out, nullptr, nullptr, nullptr);
}

uint32_t clw_ext_within_reach(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, uint8_t* within) {
    if (!within) return 0;
    return near_host_arrays(wrap, probes, ignore, n, flags, 0u, nullptr, within, nullptr, nullptr);
}

uint32_t clw_ext_near_surfaces(cl_wrap* wrap, const clw_probe* probes, const uint32_t* ignore, uint32_t n, uint32_t flags, uint32_t K, float* d,
                               uint32_t* id) {
    if (K == 0u || !d || !id) return 0;
    return near_host_arrays(wrap, probes, ignore, n, flags, K, nullptr, nullptr, d, id);
}

uint32_t clw_ext_probe_device(cl_wrap* wrap, const void* d_probes, const void* d_ignore, uint32_t n, uint32_t flags, void* d_hits, void* d_within) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_near_check(n, flags) || !d_probes || (d_hits != nullptr) == (d_within != nullptr)) return 0;
    whitted_params P{};
    wt_near_class nc;
    if (!near_params(wrap, I, n, P, nc)) return 0;
    launch_near(I, P, nc, d_probes, d_ignore, n, flags, 0u, d_hits, d_within, nullptr, nullptr);
    return n;
}

uint32_t clw_ext_near_surfaces_device(cl_wrap* wrap, const void* d_probes, const void* d_ignore, uint32_t n, uint32_t flags, uint32_t K, void* d_d,
                                      void* d_id) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_near_list_check(n, flags, K) || !d_probes || !d_d || !d_id) return 0;
    whitted_params P{};
    wt_near_class nc;
    if (!near_params(wrap, I, n, P, nc)) return 0;
    launch_near(I, P, nc, d_probes, d_ignore, n, flags, K, nullptr, nullptr, d_d, d_id);
    return n;
}

uint32_t clw_ext_cast_paths(cl_wrap* wrap, const clw_ray* rays, uint32_t n, uint32_t flags, uint32_t bounces, clw_hit* hits, uint8_t* status,
                            clw_ray* next) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_paths_check(n, flags, bounces) || !rays || !hits || !status) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!paths_params(wrap, I, n, P, cc)) return 0;
    Impl::Paths& B = I->paths;
    const size_t ray_bytes = (size_t)n * sizeof(clw_ray), hit_bytes = (size_t)bounces * n * sizeof(clw_hit);
    void* d_rays = B.rays.reserve(ray_bytes);
    void* d_hits = B.hits.reserve(hit_bytes);
    uint8_t* d_status = (uint8_t*)B.status.reserve(n);
    void* d_next = next ? B.next.reserve(ray_bytes) : nullptr;
    HIP_OK(hipMemcpyAsync(d_rays, rays, ray_bytes, hipMemcpyHostToDevice, I->stream), "Couldn't transfer the data from host to the device");
    launch_paths(I, P, cc, d_rays, n, flags, bounces, d_hits, d_status, d_next, true);
    HIP_OK(hipMemcpyAsync(hits, d_hits, hit_bytes, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    HIP_OK(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    if (next) HIP_OK(hipMemcpyAsync(next, d_next, ray_bytes, hipMemcpyDeviceToHost, I->stream), "Failed to transfer device memory to host");
    finish(I);
    return n;
}

uint32_t clw_ext_cast_paths_device(cl_wrap* wrap, const void* d_rays, uint32_t n, uint32_t flags, uint32_t bounces, void* d_hits, void* d_status,
                                   void* d_next) {
    Impl* I = impl_of(wrap);
    use_device(I);
    if (!wt_paths_check(n, flags, bounces) || !d_rays || !d_hits || !d_status) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!paths_params(wrap, I, n, P, cc)) return 0;
    launch_paths(I, P, cc, d_rays, n, flags, bounces, d_hits, (uint8_t*)d_status, d_next, true);
    return n;
}

int clw_ext_pick_path(cl_wrap* wrap, uint32_t x, uint32_t y, uint32_t bounces, uint32_t flags, clw_hit* out_hits, uint8_t* out_status) {
    Impl* I = impl_of(wrap);
    use_device(I);
    CameraRange R;
    if (!out_hits || !out_status || !wt_paths_check(1u, flags, bounces) || !camera_range(wrap, I, R)) return 0;
    if (x >= R.P.width || y >= R.P.height) return 0;
    const uint64_t pixel = (uint64_t)y * R.P.width + x;      /* is the pixel one of the wrapper's work-items? */
    if (pixel < R.P.id_offset || pixel - R.P.id_offset >= R.P.n_items) return 0;
    whitted_params P{};
    wt_cast_class cc;
    if (!paths_params(wrap, I, 1u, P, cc)) return 0;
    /* the camera-ray kernel on the one-pixel range [pixel, pixel + 1), then that ray's path */
    R.P.id_offset = pixel; R.P.n_items = 1; R.P.tiled = 0; R.P.rows = 0; R.P.row_offset = y;
    Impl::Paths& B = I->paths;
    constexpr uint32_t RAY_WORDS = sizeof(clw_ray) / 4, HIT_WORDS = sizeof(clw_hit) / 4, WORDS = RAY_WORDS + WT_PATHS_MAX * HIT_WORDS + 1;
    if (!B.pick) HIP_OK(hipMalloc((void**)&B.pick, WORDS * 4), "Couldn't allocate device memory");
    uint32_t* d_hits = B.pick + RAY_WORDS;
    uint32_t* d_status = d_hits + WT_PATHS_MAX * HIT_WORDS;
    launch_camera_rays(I, R, B.pick, false);
    launch_paths(I, P, cc, B.pick, 1u, flags, bounces, d_hits, (uint8_t*)d_status, nullptr, false);      /* (n = 1: segment k is record k) */
    uint32_t h[WT_PATHS_MAX * HIT_WORDS + 1];
    if (hipMemcpyAsync(h, d_hits, sizeof h, hipMemcpyDeviceToHost, I->stream) != hipSuccess) die("Failed to transfer device memory to host");
    finish(I);
    memcpy(out_hits, h, (size_t)bounces * sizeof(clw_hit));
    *out_status = (uint8_t)(h[WT_PATHS_MAX * HIT_WORDS] & 0xFFu);      /* (the byte the kernel wrote: the word's lowest) */
    return 1;
}

} /* extern "C" */
