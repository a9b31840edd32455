/* whitted_layers.inc -- layered ray queries (hip_wrap_ext.h: clw_layer, clw_ext_cast_layers, clw_ext_render_layers, clw_ext_pick_layers,
 * clw_ext_camera_rays): the K nearest surfaces of every ray instead of the first one, and the launch camera's rays as query rays.  Included by
 * whitted_launch.inc behind whitted_cast.inc, so it exists in the fast and the strict unit.  csrc/layers_host.c is the definition.  The scan is
 * wt_cast's, the one copy in whitted_query.inc (wt_query_scan: the flat scan and the grid walk, their arithmetic and its proof), run with the
 * sink below.  No trace kernel and no other pass is touched.
 *
 * wt_cast_layers keeps wt_cast's mapping: one ray per lane, one wave per workgroup (one batch of 64 rays), the scene staged by wt_stage_scene,
 * read from global memory, or walked through the uniform grid.  What is new is the lane's list: the C smallest keys (t, id word) met so far,
 * ascending, in REGISTERS -- every access below has a compile-time index (fully unrolled loops over C), none goes to scratch.  C is the compiled
 * capacity (4 and 8 are built; a call with K <= 4 runs C = 4); K <= C entries are stored, planar and layer-major: entry k of ray i at
 * t[k * n + i], id[k * n + i].  An empty entry is {+inf, WT_GB_ID_NONE}; a candidate at t = +inf is not listed.
 * The lane's WORST is its K-th entry (not its C-th): a candidate that is not better is dropped before the insertion, and the grid walk ends on
 * it, so K = 1 walks what wt_cast walks. */

struct wt_layers_args {
    const float4* rays;         /* 2 per ray: {origin, tmax}, {dir, bits(ignore)} */
    float* t;                   /* K * n, layer-major */
    unsigned* id;               /* K * n, layer-major */
    unsigned n, flags, K;
};

/* entry K - 1 of the list (1 <= K <= C; K is wave-uniform): a chain of selects over compile-time indices */
template <int C>
__device__ __forceinline__ void wt_layers_worst(const float (&lt)[C], const unsigned (&li)[C], unsigned K, float& wt, unsigned& wi) {
    wt = lt[C - 1]; wi = li[C - 1];
#pragma unroll
    for (int j = 0; j < C - 1; j++)
        if (K == (unsigned)(j + 1)) { wt = lt[j]; wi = li[j]; }
}

/* the key (t, id) into its place: a compare-and-shift over the whole list.  Once the key has gone in, what is carried on is the entry it
 * displaced, which comes before every later entry: the rest of the chain shifts.  DEDUPE: a key the list already holds is dropped (the grid
 * walk meets a sphere once per cell it is listed in, with the same t bits every time). */
template <int C, bool DEDUPE>
__device__ __forceinline__ void wt_layers_insert(float (&lt)[C], unsigned (&li)[C], float t, unsigned id) {
    if (DEDUPE) {
        bool held = false;
#pragma unroll
        for (int j = 0; j < C; j++) held = held || (t == lt[j] && id == li[j]);
        if (held) return;
    }
#pragma unroll
    for (int j = 0; j < C; j++) {
        const float et = lt[j];
        const unsigned ei = li[j];
        const bool before = t < et || (t == et && id < ei);
        lt[j] = before ? t : et;
        li[j] = before ? id : ei;
        t = before ? et : t;
        id = before ? ei : id;
    }
}

/* the K smallest keys (t, id), ascending.  The list is ordered by the key, so it does not depend on the order in which the grid's cells
 * present their spheres: at equal t the lower index comes first, as in the scan, where the later primitive does not displace the earlier one.
 * The grid walk ends on entry K - 1, not C - 1: the entries past K are never stored, so they need not be complete. */
template <int C>
struct wt_sink_list {
    static constexpr bool FIRST = false;
    float lt[C];
    unsigned li[C];
    unsigned K;      /* (the launcher keeps 1 <= K <= C) */
    __device__ __forceinline__ explicit wt_sink_list(unsigned K_) : K(K_) {
#pragma unroll
        for (int j = 0; j < C; j++) { lt[j] = INFINITY; li[j] = WT_GB_ID_NONE; }
    }
    /* (t < worst.t: a candidate at +inf is never listed, and in scan order an equal t is the later primitive's) */
    __device__ __forceinline__ void take(float t, unsigned id) {
        float wt;
        unsigned wi;
        wt_layers_worst<C>(lt, li, K, wt, wi);
        if (t < wt) wt_layers_insert<C, false>(lt, li, t, id);
    }
    /* the index is fetched only when !(t > worst.t): at t == worst.t the id decides, below it the candidate goes in whatever its id.  The
     * worst entry is read once, in grid_wants, and kept for the grid_take that follows it at once (read again there, the compiler does not
     * merge the two select chains: 46 more instructions in the C = 8 walk and 3-5 % of its time, profiles/r21_query_refactor_ab.txt) */
    float worst_t;
    unsigned worst_i;
    __device__ __forceinline__ bool grid_wants(float t) {
        wt_layers_worst<C>(lt, li, K, worst_t, worst_i);
        return t < INFINITY && !(t > worst_t);
    }
    __device__ __forceinline__ void grid_take(float t, unsigned i) {
        if (t == worst_t && !(i < worst_i)) return;
        wt_layers_insert<C, true>(lt, li, t, i);
    }
    __device__ __forceinline__ bool grid_done(float texit) const {
        float wt;
        unsigned wi;
        wt_layers_worst<C>(lt, li, K, wt, wi);
        return wt < INFINITY && wt <= texit;      /* (a finite K-th t: the list holds K entries) */
    }
};

template <bool GEOM_LDS, bool GRID, int C>
__global__ void __launch_bounds__(WT_BLOCK) wt_cast_layers(const whitted_params P, const wt_layers_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;

    const unsigned base = blockIdx.x * 64u;      /* (the launcher keeps groups * 64 below 2^31) */
    if (base >= A.n) return;
    const bool valid = base + lane < A.n;
    const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last ray, tests nothing and stores nothing) */
    const wt_query_ray r = wt_query_load(A.rays, k);
    wt_sink_list<C> L(A.K);
    wt_query_scan<GEOM_LDS, GRID>(P, sg, r, A.flags, valid, L);

    if (!valid) return;
#pragma unroll
    for (int j = 0; j < C; j++)
        if ((unsigned)j < L.K) {
            A.t[(size_t)j * A.n + k] = L.lt[j];
            A.id[(size_t)j * A.n + k] = L.li[j];
        }
}

/* ---- the launch camera's rays as query rays (clw_ext_camera_rays): work-item i of a linear range is pixel (id % W, id / W) of the frame, id =
 *      id_offset + i; its record is {origin, tmax = +inf, dir, ignore = WT_GB_ID_NONE}.  The pinhole's direction is wt_primary_dir's, the other
 *      models' ray wt_proj_ray's (PROJ): csrc/layers_host.c's clw_host_camera_rays, bit for bit.  A streaming kernel: two float4 stores per
 *      lane, 32 contiguous bytes. ---- */
struct wt_camrays_args {
    float corner[3], right[3], up[3], origin[3];
    float w_factor, h_factor;
    unsigned width, n;
    unsigned long long id_offset;      /* (the launcher keeps id_offset + n within 32 bits) */
    float4* rays;
};

template <bool PROJ>
__global__ void __launch_bounds__(256) wt_camera_rays(const wt_camrays_args A, const wt_projection T) {
    const size_t item = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (item >= A.n) return;
    const unsigned gid = (unsigned)(A.id_offset + item);
    f3 o = mk3(A.origin[0], A.origin[1], A.origin[2]), d;
    if (PROJ) wt_proj_ray(T, gid % A.width, gid / A.width, o, d);
    else d = wt_primary_dir(A.corner, A.right, A.up, A.w_factor, A.h_factor, gid, A.width);
    A.rays[2 * item] = make_float4(o.x, o.y, o.z, INFINITY);
    A.rays[2 * item + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(WT_GB_ID_NONE));
}
