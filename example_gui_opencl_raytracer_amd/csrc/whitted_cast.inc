/* whitted_cast.inc -- ray queries (hip_wrap_ext.h: clw_ray, clw_hit, clw_ext_cast_rays, clw_ext_occluded_rays, clw_ext_cast_rays_device): where a
 * CALLER's rays meet the scene.  wt_cast answers, for every ray of a linear range, the nearest primitive (ANY = false: a clw_hit) or whether
 * there is one at all within tmax (ANY = true: a byte).  Included by whitted_launch.inc behind whitted_query.inc, whose scan (wt_query_scan: the
 * flat scan and the grid walk, their arithmetic and its proof) it runs with one of the two sinks below; csrc/cast_host.c is its definition.
 * No trace kernel and no other pass is touched.
 *
 * Mapping: one ray per lane, one wave per workgroup, no tiles, no camera.  A ray is two float4 loads, a hit two float4 stores, `blocked` a
 * byte.  The scene is staged by wt_stage_scene or read from global memory as in wt_gbuffer.  A wave serves A.batches consecutive batches of
 * 64 rays per staging (launch_plan.c: wt_plan_cast chooses the number; measured, one batch is best -- launch_plan.h, WT_CAST_BATCHES_LDS).
 * In ANY mode a wave whose lanes are all blocked leaves the scan's loops. */

struct wt_cast_args {
    const float4* rays;         /* 2 per ray: {origin, tmax}, {dir, bits(ignore)} */
    float4* hits;               /* nearest: 2 per ray: {t, bits(id), normal.xy}, {normal.z, point} */
    unsigned char* blocked;     /* any: 1 per ray */
    unsigned n, flags, batches;
};

/* the nearest candidate: in scan order the first of an equal t stays; the grid presents its entries in any order, so there an equal t goes to
 * the lower index.  `any` is raised by every candidate, one at t = +inf too (it keeps the id WT_GB_ID_NONE). */
struct wt_sink_nearest {
    static constexpr bool FIRST = false;
    float t = INFINITY; unsigned id = WT_GB_ID_NONE; bool any = false;
    __device__ __forceinline__ void take(float ct, unsigned cid) {
        any = true;
        if (ct < t) { t = ct; id = cid; }
    }
    __device__ __forceinline__ bool grid_wants(float ct) const { return !(ct > t); }
    __device__ __forceinline__ void grid_take(float ct, unsigned i) {
        any = true;
        if (ct < t || (ct < INFINITY && i < id)) { t = ct; id = i; }      /* (ct == t here unless ct < t) */
    }
    __device__ __forceinline__ bool grid_done(float texit) const { return any && t <= texit; }
};

/* is there a candidate: the first one settles the lane */
struct wt_sink_any {
    static constexpr bool FIRST = true;
    bool any = false;
    __device__ __forceinline__ void take(float, unsigned) { any = true; }
    __device__ __forceinline__ bool grid_wants(float) const { return true; }
    __device__ __forceinline__ void grid_take(float, unsigned) { any = true; }
    __device__ __forceinline__ bool grid_done(float) const { return false; }      /* (a walk that goes on has met nothing) */
};

/* the winner's point and normal (ref_tests.h: ref_hit_point, ref_hit_normal -- wt_gbuffer's, without the EPSILON offset): one fetch of the
 * plane's normal or the centre of the sphere or light */
template <bool GEOM_LDS>
__device__ __forceinline__ void wt_query_winner(const whitted_params& P, const float4* sg, const wt_query_ray& r, float t, unsigned id, f3& ip, f3& nrm) {
    const unsigned kind = id >> 30, index = id & 0x3FFFFFFFu;
    const float4 g = wt_geom<GEOM_LDS>(P, sg, kind == 0u ? index : P.ns + 2 * index + (kind == 1u ? 0u : 2 * P.np));
    ip = wt_ref_hit_point(r.o, r.d, t);
    nrm = fv3(ref_hit_normal(kind == 1u, rv3(ip), rv3(g)));
}

template <bool GEOM_LDS, bool GRID, bool ANY>
__global__ void __launch_bounds__(WT_BLOCK) wt_cast(const whitted_params P, const wt_cast_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;

    for (unsigned bt = 0; bt < A.batches; bt++) {      /* (wave-uniform) */
        const unsigned base = (blockIdx.x * A.batches + bt) * 64u;      /* (the launcher keeps groups * batches * 64 below 2^31) */
        if (base >= A.n) break;
        const bool valid = base + lane < A.n;
        const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last ray and tests nothing) */
        const wt_query_ray r = wt_query_load(A.rays, k);
        typename std::conditional<ANY, wt_sink_any, wt_sink_nearest>::type B;
        wt_query_scan<GEOM_LDS, GRID>(P, sg, r, A.flags, valid, B);

        if (!valid) continue;
        if constexpr (ANY) { A.blocked[k] = B.any ? 1 : 0; continue; }
        else {
            f3 ip = mk3(0, 0, 0), nrm = mk3(0, 0, 0);
            if (B.id != WT_GB_ID_NONE) wt_query_winner<GEOM_LDS>(P, sg, r, B.t, B.id, ip, nrm);
            A.hits[2 * (size_t)k] = make_float4(B.t, __uint_as_float(B.id), nrm.x, nrm.y);
            A.hits[2 * (size_t)k + 1] = make_float4(nrm.z, ip.x, ip.y, ip.z);
        }
    }
}
