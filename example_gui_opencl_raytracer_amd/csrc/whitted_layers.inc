/* whitted_layers.inc -- layered ray queries (hip_wrap_ext.h: clw_layer, clw_ext_cast_layers, clw_ext_render_layers, clw_ext_pick_layers,
 * clw_ext_camera_rays): the K nearest surfaces of every ray instead of the first one, and the launch camera's rays as query rays.  Included by
 * whitted_launch.inc behind whitted_cast.inc, so it exists in the fast and the strict unit.  csrc/layers_host.c is the definition: the
 * arithmetic is wt_cast's -- wt_cast_sphere, wt_gb_ref_plane, wt_gb_ref_dot, no fused operation (`#pragma clang fp contract(off)` wherever a
 * float is computed) -- so both builds give the host's bits.  No trace kernel and no other pass is touched.
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

/* The spheres of one ray through the uniform grid: wt_cast_grid's walk with a list of K entries where that one keeps a best.  The walk may
 * only SKIP tests -- the list it leaves is the in-order scan's first K:
 *  (1) every entry is tested with the scan's operations on the scan's words (grid_geom[k] = geom[grid_items[k]]), so a sphere the walk tests
 *      gets the scan's verdict and the scan's t.  A sphere listed in several cells is tested in each and yields the same t bits every time: an
 *      insertion whose (t, id) equals an entry is dropped (wt_layers_insert<DEDUPE>), so a primitive appears once.  This is why the query has
 *      no total count: the walk cannot tell how many distinct candidates it dropped.  The list is ordered by the key (t, id word), so it does
 *      not depend on the order in which the cells present their spheres: at equal t the lower index comes first, as in the scan, where the
 *      later primitive does not displace the earlier one.  The index of an entry is fetched only when !(t > worst.t): at t == worst.t the id
 *      decides, below it the candidate goes in whatever its id.
 *  (2) no sphere that belongs to the first K is skipped: a sphere met at t is listed in the cell the ray is in at t (scene_prep.c lists it in
 *      every cell its box, padded by 1e-3 cell, touches), and the walk visits the cells of the ray in order.  It ends early in two places:
 *      where the list holds K entries and the K-th lies inside the cells walked (worst.t <= texit: a sphere with a smaller key has t <=
 *      worst.t, so it is listed in one of them) and where the rest of the walk lies beyond the ray's end (texit > tmax: a sphere met there is
 *      no candidate).  Both compare a cell boundary computed in the BUILD's arithmetic with a t or tmax in the REFERENCE's; the padding covers
 *      an ulp of the boundary, not an error of t.  So once either condition holds the walk takes ONE MORE cell before it stops, and it
 *      starts unclipped (wt_grid_begin with +inf), both exactly as wt_cast_grid and for its reasons.
 * The walk ends on entry K - 1, not C - 1: the entries past K are never stored, so they need not be complete.
 * A ray wt_ray_walkable rejects has no cells: it takes the in-order scan; an all-zero direction meets nothing (wt_cast_grid) and is spared it. */
template <int C>
__device__ __forceinline__ void wt_layers_grid(const whitted_params& P, f3 o, f3 d, float a, float tmax, unsigned ignore, bool opaque, unsigned K,
                                               float (&lt)[C], unsigned (&li)[C]) {
    float wt;
    unsigned wi;
    if (!wt_ray_walkable(o, d)) {
        if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return;
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            if (i == ignore || (opaque && (__float_as_uint(s.w) >> 31))) continue;
            const f3 v = o - mk3(s.x, s.y, s.z);
            float t;
            if (!wt_cast_sphere(v, wt_gb_ref_dot(v, v) - fabsf(s.w), d, a, tmax, t)) continue;
            wt_layers_worst<C>(lt, li, K, wt, wi);
            if (t < wt) wt_layers_insert<C, false>(lt, li, t, i);      /* (in order: an equal t is the later primitive's) */
        }
        return;
    }
    grid_walk w;
    if (!wt_grid_begin(P, o, d, INFINITY, w)) return;
    grid_cellrange cur = wt_grid_range(P, wt_grid_cell(P, w));
    bool ending = false;      /* an end condition held after the previous cell: this one is the one more */
    for (;;) {
        const float texit = w.texit;
        grid_walk nw = w;
        const bool more = wt_grid_next(P, nw) && !ending;
        grid_cellrange nxt; nxt.b = 0u; nxt.e = 0u;
        if (more) nxt = wt_grid_range(P, wt_grid_cell(P, nw));           /* in flight while this cell is tested */
        for (unsigned k = cur.b; k < cur.e; k++) {
            const float4 s = ((const float4*)P.grid_geom)[k];
            if (opaque && (__float_as_uint(s.w) >> 31)) continue;
            const f3 v = o - mk3(s.x, s.y, s.z);
            float t;
            if (!wt_cast_sphere(v, wt_gb_ref_dot(v, v) - fabsf(s.w), d, a, tmax, t) || !(t < INFINITY)) continue;
            wt_layers_worst<C>(lt, li, K, wt, wi);
            if (t > wt) continue;
            const unsigned i = P.grid_items[k];
            if (i == ignore || (t == wt && !(i < wi))) continue;
            wt_layers_insert<C, true>(lt, li, t, i);
        }
        if (!more) return;
        wt_layers_worst<C>(lt, li, K, wt, wi);
        if ((wt < INFINITY && wt <= texit) || texit > tmax) ending = true;      /* (a finite K-th t: the list holds K entries) */
        w = nw; cur = nxt;
    }
}

template <bool GEOM_LDS, bool GRID, int C>
__global__ void __launch_bounds__(WT_BLOCK) wt_cast_layers(const whitted_params P, const wt_layers_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;
    const bool opaque = (A.flags & WT_CAST_OPAQUE) != 0u;
    const unsigned K = A.K;      /* (the launcher keeps 1 <= K <= C) */

    const unsigned base = blockIdx.x * 64u;      /* (the launcher keeps groups * 64 below 2^31) */
    if (base >= A.n) return;
    const bool valid = base + lane < A.n;
    const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last ray, tests nothing and stores nothing) */
    const float4 r0 = A.rays[2 * (size_t)k], r1 = A.rays[2 * (size_t)k + 1];
    const f3 o = mk3(r0.x, r0.y, r0.z), d = mk3(r1.x, r1.y, r1.z);
    const float tmax = r0.w;
    const unsigned ignore = __float_as_uint(r1.w);
    const float a = wt_gb_ref_dot(d, d);
    float lt[C];
    unsigned li[C];
#pragma unroll
    for (int j = 0; j < C; j++) { lt[j] = INFINITY; li[j] = WT_GB_ID_NONE; }
    float wt;
    unsigned wi;

    if (A.flags & WT_CAST_SPHERES) {
        if (GRID) {
            if (valid) wt_layers_grid<C>(P, o, d, a, tmax, ignore, opaque, K, lt, li);
        }
        for (unsigned i = 0; !GRID && i < P.ns; i++) {
            const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
            const f3 v = o - mk3(s.x, s.y, s.z);
            bool ok;
            float b, D;
            {
#pragma clang fp contract(off)
                const float cc = wt_gb_ref_dot(v, v) - fabsf(s.w);
                b = wt_gb_ref_dot(v, d);
                D = b * b + (-(a * cc));
                ok = valid && i != ignore && !(opaque && (__float_as_uint(s.w) >> 31)) && !(D < 0);
            }
            if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;      /* nobody's line meets this one */
            if (ok) {
#pragma clang fp contract(off)
                const float sD = sqrtf(D);
                const float t0 = (-b - sD) / a;
                const float t = (t0 < 0) ? (-b + sD) / a : t0;
                wt_layers_worst<C>(lt, li, K, wt, wi);
                /* (t < worst.t: a candidate at +inf is never listed, and in scan order an equal t is the later primitive's) */
                if (!(t <= 0) && t <= tmax && t < wt) wt_layers_insert<C, false>(lt, li, t, i);
            }
        }
    }
    if (A.flags & WT_CAST_PLANES) {
        for (unsigned i = 0; i < P.np; i++) {
            const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
            const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
            float t;
            if (valid && (WT_GB_KIND_PLANE | i) != ignore && wt_gb_ref_plane(o, d, pn, p0, t) && t <= tmax) {
                wt_layers_worst<C>(lt, li, K, wt, wi);
                if (t < wt) wt_layers_insert<C, false>(lt, li, t, WT_GB_KIND_PLANE | i);      /* (kind 1 ids follow every sphere's) */
            }
        }
    }
    if (A.flags & WT_CAST_LIGHTS) {
        for (unsigned i = 0; i < P.nl; i++) {
            const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * i);
            const f3 v = o - mk3(l0.x, l0.y, l0.z);
            float t;
            if (valid && (WT_GB_KIND_LIGHT | i) != ignore && wt_cast_sphere(v, wt_gb_ref_dot(v, v) - fabsf(l0.w), d, a, tmax, t)) {
                wt_layers_worst<C>(lt, li, K, wt, wi);
                if (t < wt) wt_layers_insert<C, false>(lt, li, t, WT_GB_KIND_LIGHT | i);
            }
        }
    }

    if (!valid) return;
#pragma unroll
    for (int j = 0; j < C; j++)
        if ((unsigned)j < K) {
            A.t[(size_t)j * A.n + k] = lt[j];
            A.id[(size_t)j * A.n + k] = li[j];
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
