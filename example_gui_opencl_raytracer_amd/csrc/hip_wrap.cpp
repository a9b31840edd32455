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
#include "hip_wrap_impl.h"

using namespace clw;

namespace clw {
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
} /* namespace clw */

namespace {

constexpr size_t COUNTER_WORDS = CLW_NUM_COUNTERS + 16 * (size_t)CLW_STAMP_SHARDS;
constexpr size_t GRID_MAX_PAIRS = (size_t)1 << 25;   /* 20 B per cell-list entry */

/* the same floats bit for bit (+0 and -0 differ, a NaN equals itself): "the device table is unchanged" is decided on what it holds */
bool same_bits(const std::vector<float>& a, const float* b, size_t n) {
    return a.size() == n && (n == 0 || !memcmp(a.data(), b, n * sizeof(float)));
}

/* field by field (the struct has tail padding, which a memcmp would also compare); floats by bit pattern */
bool same_raygen(const RaygenArgs& a, const RaygenArgs& b) {
    return !memcmp(a.corner, b.corner, 12) && !memcmp(a.origin, b.origin, 12) && !memcmp(a.up, b.up, 12) &&
           !memcmp(a.right, b.right, 12) && !memcmp(&a.w_factor, &b.w_factor, 4) && !memcmp(&a.h_factor, &b.h_factor, 4) &&
           a.width == b.width && a.height == b.height && a.id_offset == b.id_offset && a.n_items == b.n_items &&
           a.band_stride == b.band_stride && a.band_phase == b.band_phase;
}

bool same_acc_key(const Impl::AccKey& a, const Impl::AccKey& b) {
    return same_raygen(a.gen, b.gen) && a.n_out == b.n_out && a.total == b.total && a.depth == b.depth && a.strict == b.strict && a.fuse == b.fuse &&
           a.ss == b.ss && a.max_frames == b.max_frames && a.jitter == b.jitter && !memcmp(&a.through, &b.through, 4) && a.seed == b.seed &&
           !memcmp(a.buf, b.buf, sizeof a.buf) && !memcmp(a.dptr, b.dptr, sizeof a.dptr) && !memcmp(a.size, b.size, sizeof a.size) &&
           !memcmp(a.counts, b.counts, sizeof a.counts) && !memcmp(a.img, b.img, sizeof a.img) && a.epoch == b.epoch;
}

void check_kernel_id(const cl_wrap* w, cl_uint kernel_id) {
    if (kernel_id >= w->kernels_num) die("Wrong kernel ID given");
}

Buffer* new_buffer(Impl* I) {
    Buffer* b = new Buffer();
    I->live.push_back(b);
    return b;
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
    hipError_t e = WT_LAUNCH(I, raygen)(&P, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    t.done();
}

clw_camera camera_of(const RaygenArgs& g) {
    clw_camera c{};
    memcpy(c.im_corner, g.corner, 12); memcpy(c.origin, g.origin, 12); memcpy(c.up, g.up, 12); memcpy(c.right, g.right, 12);
    c.w_factor = g.w_factor; c.h_factor = g.h_factor; c.width = g.width; c.height = g.height;
    return c;
}

} /* namespace */
namespace clw {
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
} /* namespace clw */
namespace {

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
    hipError_t e = WT_LAUNCH(I, raygen_proj)(&P, &T, I->stream);
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

const uint8_t* host_view(Impl* I, Buffer* b, size_t need, std::vector<uint8_t>& tmp) {
    if (b->size < need) die("Couldn't run the kernel");
    if (b->shadow.size() >= need) return b->shadow.data();
    ensure_allocated(I, b);
    tmp.resize(need);
    if (need) HIP_OK(hipMemcpy(tmp.data(), b->dptr, need, hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    return tmp.data();
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

} /* namespace */
namespace clw {
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
    I->grid_ok = false; I->near_grid_ok = false;
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
            /* the proximity queries' box through the grid needs every prepared r * r word finite (whitted_near.inc) */
            I->near_grid_ok = true;
            for (uint32_t i = 0; i < ns; i++) if (!std::isfinite(geom[4 * (size_t)i + 3])) I->near_grid_ok = false;
        }
    }
    I->geom_f4 = f4;
    I->scene_generation++;
    I->prep_s = s; I->prep_p = p; I->prep_l = l; I->prep_ns = ns; I->prep_np = np; I->prep_nl = nl;
}
} /* namespace clw */
namespace {

Buffer* buffer_arg(cl_wrap* w, cl_uint kernel_id, cl_uint arg) {
    if (!is_registered(w, kernel_id, arg)) die("Couldn't run the kernel");
    return (Buffer*)w->buffers[kernel_id][arg];
}

Buffer* rays_of(const cl_wrap* w, Impl* I, cl_uint kid) {
    Buffer* rays = find_rays(w, I, kid);
    if (!rays) die("Couldn't run the kernel");
    return rays;
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
    bind_geometry(I, P, flags);
    P.spheres_raw = (const uint8_t*)bs->dptr; P.planes_raw = (const uint8_t*)bp->dptr;
    P.tex = (const uint32_t*)tex->dptr; P.tex_w = (int)tex->w; P.tex_h = (int)tex->h; P.tex_layers = (int)tex->layers;
    P.sky = (const uint32_t*)sky->dptr; P.sky_w = (int)sky->w; P.sky_h = (int)sky->h;
}
} /* namespace */
namespace clw {
/* both, for the launches that are not planned (the primary-hit pass, clw_ext_unit_scene): fills the scene fields of P and chooses between the
 * uniform grid, LDS-staged geometry and geometry read from global memory (flags WT_F_GRID / WT_F_GEOM_LDS, dynamic LDS bytes) */
void bind_scene(cl_wrap* w, Impl* I, cl_uint kid, whitted_params& P, int& flags, size_t& dyn_lds) {
    prepare_bound_scene(w, I, kid);
    const wt_geom_class gc = wt_plan_geometry(I->strict, I->variant, I->prep_ns, I->prep_np, (uint32_t)I->geom_f4, I->have_lpt, I->grid_ok && I->use_grid);
    flags |= gc.flags;
    if (gc.flags & WT_F_GEOM_LDS) dyn_lds = gc.dyn_lds;
    P.lpt = gc.lpt; P.vis = gc.vis;
    P.through = I->through;
    bind_scene_pointers(w, I, kid, P, gc.flags);
}
} /* namespace clw */
namespace {

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

/* the primary-ray cull table of a launch that reads one (wt_plan_cull): built on the launch stream, ahead of the trace, when the camera, the
 * frame, the row range or the prepared scene differ from what it was built for AND the launch before this one had the same view (a table is
 * never read for another view than its own) -> the table, or null (test everything) */
const unsigned char* bind_primary_cull(Impl* I, Impl::Cull& C, const wt_plan_in& in, const wt_plan_out& plan) {
    C.last_used = false;
    if (!wt_plan_cull(&in, &plan)) return nullptr;
    const whitted_params& P = plan.P;
    wt_cull_view V;
    memset(&V, 0, sizeof V);
    memcpy(V.corner, P.corner, sizeof V.corner); memcpy(V.origin, P.origin, sizeof V.origin);
    memcpy(V.up, P.up, sizeof V.up); memcpy(V.right, P.right, sizeof V.right);
    V.w_factor = P.w_factor; V.h_factor = P.h_factor;
    V.width = P.width; V.rows = P.rows; V.row_offset = P.row_offset; V.band_stride = P.band_stride; V.band_phase = P.band_phase;
    if (!wt_cull_view_ok(&V)) return nullptr;      /* a camera term that is not finite: no bit could be set */
    const uint32_t tiles = plan.trows * plan.tpr;
    const size_t bytes = (2u * (size_t)tiles + 3u) & ~(size_t)3u;      /* two bytes per tile: the primary byte, the bounce byte */
    /* (the bounce byte also depends on the launch depth -- it names the second iteration -- and on the parts asked for) */
    const bool current = C.valid && C.scene == I->scene_generation && C.tiles == tiles && C.depth == P.depth && C.parts == I->bounce_parts && !memcmp(&C.view, &V, sizeof V);
    if (!current) {
        /* A table pays when it is read more than once: the builder's launch runs 30 us (1920x1080, demo scene: both bytes of a tile, in
         * double precision) and the table saves a frame 5.6 us of kernel time; when the builder wrote the primary byte alone it ran 7 us, cost
         * a frame 4.7 us of wall time and saved it 1 us.  So a view is built for when it is seen the SECOND time in a row: a camera that
         * moves every frame never builds (its launches test everything, as before), a still view builds once, behind its first frame. */
        const bool again = C.seen && C.seen_scene == I->scene_generation && C.seen_tiles == tiles && !memcmp(&C.seen_view, &V, sizeof V);
        C.valid = false;
        if (!again) { C.seen = true; C.seen_view = V; C.seen_scene = I->scene_generation; C.seen_tiles = tiles; return nullptr; }
    }
    wait_tables_fence(I);
    if (C.bytes != bytes || !C.table) {
        if (C.table) { finish(I); C.free_all(); }
        HIP_OK(hipMalloc((void**)&C.table, bytes), "Couldn't allocate device memory");
        C.bytes = bytes;
    }
    if (!current) {
        if (wt_fast_launch_cull(&P, I->bounce_parts, C.table, I->stream) != hipSuccess) die("Couldn't run the kernel");
        C.view = V; C.scene = I->scene_generation; C.tiles = tiles; C.depth = P.depth; C.parts = I->bounce_parts; C.valid = true; C.builds++;
    }
    I->tables_in_flight = true;
    C.last_used = true;
    return C.table;
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
    const unsigned char* tile_cull = bind_primary_cull(I, I->culls[strip ? strip->slot : 0], in, plan);
    LaunchTimer t(I, kid, pass == PASS_PLAIN);      /* (an adaptive launch is timed as one: run_raytracer) */
    hipError_t e = WT_LAUNCH(I, trace)(&plan.P, tile_cull, plan.flags, plan.grid, plan.dyn_lds, I->stream);
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
    I->bounce_parts = (uint32_t)env_int("CLWRAP_BOUNCE_CULL", 3) & 3u;      /* A/B runs: clw_ext_set_bounce_cull */
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
    I->gb.release();
    I->ov.release();
    I->obj.release();
    I->ao.release();
    I->cast.free_buffers();
    I->layers.release();
    I->paths.release();
    I->near.release();
    I->ptab.free_all();
    I->adapt.free_all();
    if (I->tables_fence) (void)hipEventDestroy(I->tables_fence);
    for (uint32_t* q : {I->d_grid_start, I->d_grid_items, I->d_grid_box}) if (q) (void)hipFree(q);
    if (I->d_grid_geom) (void)hipFree(I->d_grid_geom);
    if (I->sched_stream) (void)hipStreamSynchronize(I->sched_stream);
    for (auto& sc : I->scheds) sc.free_all();
    for (auto& c : I->culls) c.free_all();
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
    hipError_t e = WT_LAUNCH(I, unit)(op, din, dout, n, stride_in, stride_out, aux, I->stream);
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
    hipError_t e = WT_LAUNCH(I, unit_scene)(&P, flags, op, din, dout, n, stride_in, stride_out, dyn_lds, I->stream);
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
/* byte `which` (0 = primary, 1 = bounce) of every tile's entry of a slot's table -> out[tiles] */
static void read_cull_bytes(const Impl::Cull& C, unsigned which, uint8_t* out) {
    std::vector<uint8_t> both(2u * (size_t)C.tiles);
    HIP_OK(hipMemcpy(both.data(), C.table, both.size(), hipMemcpyDeviceToHost), "Failed to transfer device memory to host");
    for (uint32_t t = 0; t < C.tiles; t++) out[t] = both[2u * (size_t)t + which];
}
uint32_t clw_ext_read_primary_cull(cl_wrap* wrap, uint8_t* out, uint32_t capacity, uint64_t* builds) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    const Impl::Cull& C = I->culls[0];
    if (builds) *builds = C.builds;
    if (!C.last_used || !C.table) return 0;
    if (out && capacity >= C.tiles) read_cull_bytes(C, 0, out);
    return C.tiles;
}
uint32_t clw_ext_read_bounce_cull(cl_wrap* wrap, uint8_t* out, uint32_t capacity) {
    Impl* I = impl_of(wrap);
    use_device(I);
    finish(I);
    const Impl::Cull& C = I->culls[0];
    if (!C.last_used || !C.table) return 0;
    if (out && capacity >= C.tiles) read_cull_bytes(C, 1, out);
    return C.tiles;
}
void clw_ext_set_bounce_cull(cl_wrap* wrap, int parts) {
    if (parts < 0 || parts > 3) die("The bounce cull parts must be 0 (none), 1 (shadow), 2 (reflected) or 3 (both)");
    Impl* I = impl_of(wrap);
    I->bounce_parts = (uint32_t)parts;
    for (auto& c : I->culls) c.valid = false;      /* the view's next launch builds its table again */
}
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
    std::vector<float> col, row;      /* the panorama's tables; the other model has none: null host arrays, null device pointers */
    if (T.model == CLW_PROJ_EQUIRECT) {
        col.resize(4 * (size_t)cam->width); row.resize(4 * (size_t)cam->height);
        if (!clw_host_projection_tables(cam, proj, col.data(), row.data())) return 0;
    }
    const DeviceTemp<float> dcol(col.empty() ? nullptr : col.data(), col.size() * sizeof(float)), drow(row.empty() ? nullptr : row.data(), row.size() * sizeof(float));
    const DeviceTemp<float> drays((size_t)n * 64);
    if (T.model == CLW_PROJ_EQUIRECT) { T.col = dcol; T.row = drow; }
    HIP_OK(hipDeviceSynchronize(), "The device kernel failed");
    raygen_params P{};
    P.width = cam->width; P.height = cam->height; P.id_offset = id_begin; P.n_items = n; P.rays = drays; P.band_stride = 1; P.band_phase = 0;
    hipError_t e = WT_LAUNCH(I, raygen_proj)(&P, &T, I->stream);
    if (e != hipSuccess) die("Couldn't run the kernel");
    finish(I);
    drays.read(out_rays, (size_t)n * 64);
    return 1;
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
