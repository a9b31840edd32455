/* whitted_paths.inc -- path queries (hip_wrap_ext.h: clw_ext_cast_paths, clw_ext_cast_paths_device, clw_ext_pick_path): where a caller's ray
 * GOES -- its hit, the reference's reflected or refracted ray from there, that ray's hit, and so on for up to 8 segments -- in one launch.
 * Included by whitted_launch.inc behind whitted_layers.inc, so it exists in the fast and the strict unit.  csrc/paths_host.c is the definition.
 * A segment is wt_cast's nearest query: the one scan of whitted_query.inc (wt_query_scan: the flat scan and the grid walk, their arithmetic and
 * its proof) with wt_cast's sink (wt_sink_nearest), and wt_cast's evaluation of the winner (wt_query_winner).  What becomes of a hit -- the stop
 * rule, the outgoing ray -- is csrc/ref_tests.h (ref_path_stops, ref_bounce), the one text the definition is compiled from too.  No trace kernel
 * and no other pass is touched.
 *
 * Mapping: wt_cast's -- one ray per lane, one wave per workgroup (one batch of 64 rays), the scene staged by wt_stage_scene, read from global
 * memory, or walked through the uniform grid.  The lane's path lives in registers: the current ray, the refractive index n1, the count and the
 * reason.  The loop runs over segments and is wave-uniform: a lane whose path has ended runs along and tests nothing (`live` is the scan's
 * `valid`), and the wave leaves the loop when none of its lanes is live.  The number of segments is a run-time argument: the loop body is one
 * scan, a compile-time count would unroll nothing worth having.
 * The winner's four material words -- transperent, dielectric, n, reflectivity -- are read from the bound sphere / plane array itself
 * (wt_mat_f4: one 16-byte load at byte 64 of the 96-byte record, for the winner only, as the trace kernels gather materials), not from a
 * prepared table: a table would be one more thing to build and to invalidate with the scene, to spare one load per SEGMENT beside a scan
 * that makes one per primitive.
 * Output: hits[seg * n + ray] (2 float4 per clw_hit), layer-major; the layers a path does not reach receive the miss record.  status[ray] =
 * count | reason << 4.  next (may be null): the ray the path would go on with, see the header. */

struct wt_paths_args {
    const float4* rays;         /* 2 per ray: {origin, tmax}, {dir, bits(ignore)} */
    float4* hits;               /* 2 per ray and segment: {t, bits(id), normal.xy}, {normal.z, point}; segment-major */
    unsigned char* status;      /* 1 per ray */
    float4* next;               /* 2 per ray, or null */
    unsigned n, flags, bounces;
};

#define WT_PATH_TRANSMIT 16u
#define WT_PATH_ALL_SURFACES 32u

__device__ __forceinline__ void wt_path_store_hit(float4* hits, size_t at, float t, unsigned id, f3 nrm, f3 ip) {
    hits[2 * at] = make_float4(t, __uint_as_float(id), nrm.x, nrm.y);
    hits[2 * at + 1] = make_float4(nrm.z, ip.x, ip.y, ip.z);
}

template <bool GEOM_LDS, bool GRID>
__global__ void __launch_bounds__(WT_BLOCK) wt_cast_paths(const whitted_params P, const wt_paths_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;

    const unsigned base = blockIdx.x * 64u;      /* (the launcher keeps groups * 64 below 2^31) */
    if (base >= A.n) return;
    const bool valid = base + lane < A.n;
    const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last ray, tests nothing and stores nothing) */
    wt_query_ray r = wt_query_load(A.rays, k);
    const unsigned cast_flags = A.flags & (WT_CAST_SPHERES | WT_CAST_PLANES | WT_CAST_LIGHTS | WT_CAST_OPAQUE);
    float n1 = REF_DEFAULT_N;
    unsigned count = 0u, reason = 0u;
    bool live = valid;

    unsigned seg = 0u;
    for (; seg < A.bounces; seg++) {      /* (wave-uniform) */
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;      /* every path of the wave has ended */
        wt_sink_nearest B;
        wt_query_scan<GEOM_LDS, GRID>(P, sg, r, cast_flags, live, B);
        if (!live) {      /* an ended path's layer: the miss record */
            if (valid) wt_path_store_hit(A.hits, (size_t)seg * A.n + k, INFINITY, WT_GB_ID_NONE, mk3(0, 0, 0), mk3(0, 0, 0));
            continue;
        }
        if (B.id == WT_GB_ID_NONE) {      /* a miss: r stays the ray that missed */
            wt_path_store_hit(A.hits, (size_t)seg * A.n + k, B.t, WT_GB_ID_NONE, mk3(0, 0, 0), mk3(0, 0, 0));
            reason = 1u; live = false;
            continue;
        }
        f3 ip, nrm;
        wt_query_winner<GEOM_LDS>(P, sg, r, B.t, B.id, ip, nrm);
        wt_path_store_hit(A.hits, (size_t)seg * A.n + k, B.t, B.id, nrm, ip);
        count = seg + 1u;

        const unsigned kind = B.id >> 30, index = B.id & 0x3FFFFFFFu;
        const f3 p = wt_ref_hit_offset(ip, nrm);      /* the point shading uses */
        bool stops = kind == 2u;      /* a light */
        ref_material m = {0u, 0u, 0.0f, 0.0f};
        if (!stops) {
            const float4 w = wt_mat_f4(P, kind == 0u ? index : P.ns + index, 2u, P.ns);
            m.transperent = __float_as_uint(w.x); m.dielectric = __float_as_uint(w.y); m.n = w.z; m.reflectivity = w.w;
            stops = ref_path_stops(&m, (A.flags & WT_PATH_ALL_SURFACES) != 0u);
        }
        if (stops) {
            r.o = p; r.d = mk3(0, 0, 0); r.ignore = WT_GB_ID_NONE;
            reason = 2u; live = false;
            continue;
        }
        ref_v3 o, d;      /* the outgoing ray */
        ref_bounce(rv3(p), rv3(nrm), rv3(r.d), &m, (A.flags & WT_PATH_TRANSMIT) != 0u, &n1, &o, &d);
        r.o = fv3(o); r.d = fv3(d); r.ignore = WT_GB_ID_NONE;
        r.a = ref_dot(d, d);
    }
    if (!valid) return;
    for (; seg < A.bounces; seg++)      /* the layers no path of the wave reached */
        wt_path_store_hit(A.hits, (size_t)seg * A.n + k, INFINITY, WT_GB_ID_NONE, mk3(0, 0, 0), mk3(0, 0, 0));
    A.status[k] = (unsigned char)(count | reason << 4);
    if (A.next) {
        A.next[2 * (size_t)k] = make_float4(r.o.x, r.o.y, r.o.z, r.tmax);
        A.next[2 * (size_t)k + 1] = make_float4(r.d.x, r.d.y, r.d.z, __uint_as_float(r.ignore));
    }
}
