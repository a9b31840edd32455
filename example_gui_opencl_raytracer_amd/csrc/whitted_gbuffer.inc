/* whitted_gbuffer.inc -- the primary-hit pass: what the FIRST segment of every pixel of a launch range meets, written out as planar
 * geometric buffers (hip_wrap_ext.h: clw_ext_render_gbuffer, clw_ext_pick).  Included by whitted_launch.inc behind whitted_trace.inc, so it
 * exists in the fast and the strict unit and is built from the trace kernel's own pieces: the primary ray of wt_primary_dir(_xy) through the
 * work-item mapping of wt_trace_body, the ray invariants of wt_rayq, the split sphere test (wt_sphere_pre / _disc / _root), wt_plane, the
 * wave-uniform geometry fetch wt_geom over the scene staged by wt_stage_scene, the grid walks wt_grid_nearest / wt_grid_occluded.
 * The search is the one of whitted_hit.inc -- findLightIntersection first, a visible light ending it (primitives.cl:262-318), then the nearest of
 * spheres, then planes, ties keeping the earlier primitive (primitives.cl:322-394) -- in the same operations in the same order, so it takes the
 * decisions the trace kernel of the build takes; what it adds is WHICH primitive or light won.  Nothing else runs: no shading, no shadow rays, no
 * skybox fetch, no random numbers, no tile costs.
 * WHICH primitive wins is decided by that search, in the build's own arithmetic: the pass names the object the trace launch of the same build
 * shades.  WHERE it is hit -- depth, point, normal, a light's colour -- is then evaluated once more for the winner alone in the reference's
 * arithmetic (csrc/ref_tests.h: IEEE divide and square root, no fused operation), the same in both builds: D/4 = b b - c cancels near a silhouette
 * and from afar, where the fast build's fused products move t by 1e-4 and more and a light's (1 / d) * d by an ulp, and a consumer of the buffers
 * (a focus distance, a denoiser's normals) should not see which build made them.  In the strict build these are the search's own values.
 * The pass sees the launch camera at pixel centres and the scene as it stands: no sample cameras, no sphere motion, no jitter, no seed.
 * Under a camera model beside the pinhole (the kernel's third argument, wt_projection: hip_wrap_ext.h, clw_ext_set_projection) the primary ray is
 * wt_proj_ray's and no direction is taken for unit, as the trace launch of such a view takes none.  That is the PROJ instantiation: a run-time
 * branch on the model was measured first and cost the pinhole's pass 5-8 % on the demo scene (0.0245 against 0.0230 ms at 1920x1080: a = d.d = 1
 * stopped being a compile-time constant of the sphere tests), so the pinhole keeps an instantiation that executes what it executed. */

/* id word of a pixel: kind << 30 | index (hip_wrap_ext.h: CLW_GB_ID) */
#define WT_GB_KIND_PLANE (1u << 30)
#define WT_GB_KIND_LIGHT (2u << 30)
#define WT_GB_ID_NONE 0xFFFFFFFFu

/* the channels a launch writes: planar, indexed by work-item like `out`; a NULL pointer = the channel was not asked for (wave-uniform) */
struct wt_gbuffer_out {
    float* depth;        /* 1 per work-item */
    unsigned* id;        /* 1 */
    float* normal;       /* 3 */
    float* point;        /* 3 */
    float* albedo;       /* 3 */
};

/* ---- the reference's arithmetic (primitives.cl:170-215) is csrc/ref_tests.h, the one text the host definitions are compiled from too: both
 *      units are compiled without contraction and with correctly rounded divide and square root, so the fast unit computes the same bits.
 *      Here only the adapters between the kernels' f3 / float4 and its ref_v3: no arithmetic ---- */
static_assert(REF_EPSILON == WT_EPSILON, "the point shading uses");
__device__ __forceinline__ ref_v3 rv3(f3 a) { return ref_mk(a.x, a.y, a.z); }
__device__ __forceinline__ ref_v3 rv3(float4 a) { return ref_mk(a.x, a.y, a.z); }
__device__ __forceinline__ f3 fv3(ref_v3 a) { return mk3(a.x, a.y, a.z); }
__device__ __forceinline__ float wt_ref_dot(f3 a, f3 b) { return ref_dot(rv3(a), rv3(b)); }
__device__ __forceinline__ f3 wt_ref_hit_point(f3 o, f3 d, float t) { return fv3(ref_hit_point(rv3(o), rv3(d), t)); }
__device__ __forceinline__ f3 wt_ref_hit_offset(f3 point, f3 n) { return fv3(ref_hit_offset(rv3(point), rv3(n))); }

__device__ __forceinline__ void wt_gb_store3(float* __restrict__ p, unsigned item, f3 v) {
    if (p) { float* q = p + 3 * (size_t)item; q[0] = v.x; q[1] = v.y; q[2] = v.z; }
}

/* the ray of a pixel under a camera model beside the pinhole (whitted_projection.inc) */
__device__ __forceinline__ void wt_proj_ray(const wt_projection& T, unsigned x, unsigned y, f3& o, f3& d);

template <bool GEOM_LDS, bool GRID, bool PROJ>
__global__ void __launch_bounds__(WT_BLOCK) wt_gbuffer(const whitted_params P, const wt_gbuffer_out G, const wt_projection T) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wg = blockIdx.x;
    constexpr bool UNIT_CT = !WT_STRICT && GEOM_LDS && !GRID && !PROJ;       /* as the fused trace launch: see whitted_hit.inc (a projected view takes no direction for unit, as its trace launch takes none) */

    /* ---- work-item -> pixel: wt_trace_body's mapping in its default dispatch order (no tile order, no split tiles) ---- */
    bool valid;
    unsigned item, x = 0, y = 0;
    if (P.tiled) {
        const unsigned tpr = (P.width + 7u) >> 3;
        const unsigned k = wg & 7u, j = wg >> 3;
        const unsigned trow = (j / tpr) * 8u + k, tcol = j % tpr;
        x = tcol * 8u + (lane & 7u);
        y = trow * 8u + (lane >> 3);
        valid = (x < P.width) && (y < P.rows);
        item = y * P.width + x;
    } else {
        item = wg * WT_BLOCK + tid;
        valid = item < P.n_items;
        if (P.band_stride > 1u) { y = item / P.width; x = item % P.width; }
    }
    unsigned long long gid = P.id_offset + item;
    unsigned gy = y;
    if (P.band_stride > 1u) {
        gy = ((y >> 3) * P.band_stride + P.band_phase) * 8u + (y & 7u);
        gid = (unsigned long long)gy * P.width + x;
    } else if (P.tiled) {
        gy = P.row_offset + y;
    }
    if (!valid) return;      /* (behind the staging barrier; every ballot below is an early-out over per-lane predicates) */

    f3 d;
    f3 o = mk3(P.origin[0], P.origin[1], P.origin[2]);
    if (PROJ) {      /* the orthographic view or the panorama (the shim clears unit_dirs); the pinhole's instantiation never reads T */
        if (P.tiled || P.band_stride > 1u) wt_proj_ray(T, x, gy, o, d);
        else wt_proj_ray(T, (unsigned)gid % P.width, (unsigned)gid / P.width, o, d);
    } else if (P.tiled || P.band_stride > 1u) d = wt_primary_dir_xy(P.corner, P.right, P.up, P.w_factor, P.h_factor, x, gy);
    else d = wt_primary_dir(P.corner, P.right, P.up, P.w_factor, P.h_factor, (unsigned)gid, P.width);
    const rayq r = UNIT_CT ? wt_rayq<true>(o, d) : wt_rayq<false>(o, d, P.unit_dirs != 0u);
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;

    /* ---- findLightIntersection (primitives.cl:262-318): the nearest light sphere in index order, then is anything in front of it ---- */
    bool lit = false;
    float tl = INFINITY;
    unsigned li = 0u;
    for (unsigned i = 0; i < P.nl; i++) {
        const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * i);
        const sph_pre pre = wt_sphere_pre(r.o, l0);
        float bq, Dq;
        const bool ok = wt_sphere_disc(pre, r.d, r.a4, bq, Dq);
        if (__builtin_amdgcn_ballot_w64(ok)) {              /* rare: a light sphere is on somebody's line */
            float t;
            const bool hit = wt_sphere_root(bq, Dq, r.a2, t) && ok;
            if (hit && !(t >= tl)) { tl = t; li = i; lit = true; }
        }
    }
    if (__builtin_amdgcn_ballot_w64(lit)) {
        if (lit) {
            if (GRID) {
                if (wt_grid_occluded(P, r, tl)) lit = false;
            }
            for (unsigned i = 0; !GRID && i < P.ns; i++) {
                const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
                float t;
                const bool hit = wt_sphere(r, s, t);
                if (hit && t <= tl && !(__float_as_uint(s.w) >> 31)) lit = false;
            }
            for (unsigned i = 0; i < P.np; i++) {
                const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                float t;
                const bool hit = wt_plane(r, n, p0, t);
                if (hit && t <= tl) lit = false;
            }
        }
    }

    float depth = INFINITY;
    unsigned id = WT_GB_ID_NONE;
    f3 nrm = mk3(0, 0, 0), ip = mk3(0, 0, 0), alb = mk3(0, 0, 0);
    if (lit) {
        /* the light that was seen, in the reference's arithmetic (a test that does not confirm the hit keeps the search's t) */
        const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * li);
        const float4 l1 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * li + 1);
        float tr;
        if (ref_sphere(rv3(o), rv3(d), rv3(l0), l0.w, &tr)) tl = tr;
        const f3 hp = wt_ref_hit_point(o, d, tl);
        const float dist = ref_length(ref_sub(rv3(o), rv3(hp)));
        depth = tl; id = WT_GB_KIND_LIGHT | li;
        alb = mk3(l1.x, l1.y, l1.z) * (1 / dist * dist);      /* "(1/d*d)" = (1/d)*d, not inverse-square: kept (primitives.cl:287) */
    } else {
        /* ---- findSolidIntersection (primitives.cl:322-394): nearest wins, the strict `_t >= t` keeps the earlier primitive on ties ---- */
        float tbest = INFINITY;
        int best = -1;
        if (GRID) {
            best = wt_grid_nearest(P, r, tbest);
        } else {
            for (unsigned i = 0; i < P.ns; i++) {
                const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
                const sph_pre pre = wt_sphere_pre(r.o, s);
                float bq, Dq;
                const bool ok = wt_sphere_disc(pre, r.d, r.a4, bq, Dq);
                if (__builtin_amdgcn_ballot_w64(ok) == 0) continue;       /* nobody's line meets this one */
                float t;
                const bool hit = wt_sphere_root(bq, Dq, r.a2, t) && ok;
                if (hit && !(t >= tbest)) { tbest = t; best = (int)i; }
            }
        }
        for (unsigned i = 0; i < P.np; i++) {
            const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
            const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
            float t;
            const bool hit = wt_plane(r, n, p0, t);
            if (hit && !(t >= tbest)) { tbest = t; best = (int)(P.ns + i); }
        }
        if (best >= 0) {
            /* the winner, in the reference's arithmetic (a test that does not confirm the hit keeps the search's t) */
            const unsigned prim = (unsigned)best;
            bool textured = false;
            unsigned texpx = 0u;
            float tr;
            if (prim < P.ns) {
                const float4 s = wt_geom<GEOM_LDS>(P, sg, prim);
                if (ref_sphere(rv3(o), rv3(d), rv3(s), s.w, &tr)) tbest = tr;
                ip = wt_ref_hit_point(o, d, tbest);
                nrm = fv3(ref_hit_normal(0, rv3(ip), rv3(s)));
                id = prim;
            } else {
                const unsigned pi = prim - P.ns;
                const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * pi);
                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * pi + 1);
                if (ref_plane(rv3(o), rv3(d), rv3(n), rv3(p0), &tr)) tbest = tr;
                ip = wt_ref_hit_point(o, d, tbest);
                nrm = fv3(ref_hit_normal(1, rv3(ip), rv3(n)));
                id = WT_GB_KIND_PLANE | pi;
                if (n.w != 0.0f && G.albedo) {               /* texture_id >= 0: the texel of the pre-offset point (primitives.cl:377) */
                    texpx = wt_plane_texel_fetch(P, pi, ip);
                    textured = true;
                }
            }
            if (G.albedo) {
                const float4 a_ = wt_mat_f4(P, prim, 0u, P.ns);
                alb = textured ? wt_texel_rgb(texpx) : mk3(a_.x, a_.y, a_.z);
            }
            depth = tbest;
            ip = wt_ref_hit_offset(ip, nrm);                 /* the point shading uses */
        }
    }
    if (G.depth) G.depth[item] = depth;
    if (G.id) G.id[item] = id;
    wt_gb_store3(G.normal, item, nrm);
    wt_gb_store3(G.point, item, ip);
    wt_gb_store3(G.albedo, item, alb);
}
