/* whitted_cast.inc -- ray queries (hip_wrap_ext.h: clw_ray, clw_hit, clw_ext_cast_rays, clw_ext_occluded_rays, clw_ext_cast_rays_device): where a
 * CALLER's rays meet the scene.  wt_cast answers, for every ray of a linear range, the nearest primitive (ANY = false: a clw_hit) or whether
 * there is one at all within tmax (ANY = true: a byte).  Included by whitted_launch.inc behind whitted_ao.inc, so it exists in the fast and the
 * strict unit.  csrc/cast_host.c is its definition: the arithmetic below is that file's, operation for operation -- wt_gb_ref_dot's sums, IEEE
 * square root and divide, no fused operation (`#pragma clang fp contract(off)` wherever a float is computed) -- so both builds give the host's
 * bits.  No trace kernel and no other pass is touched.
 *
 * Mapping: one ray per lane, one wave per workgroup, no tiles, no camera.  A ray is two float4 loads, a hit two float4 stores, `blocked` a
 * byte.  The scene is staged by wt_stage_scene or read from global memory as in wt_gbuffer.  A wave serves A.batches consecutive batches of
 * 64 rays per staging (launch_plan.c: wt_plan_cast chooses the number; measured, one batch is best -- launch_plan.h, WT_CAST_BATCHES_LDS).
 * Flat scan: the primitives are the outer loop, fetched wave-uniformly with wt_geom; D < 0 leaves before the square root and the divides (the
 * definition's verdict is then `no hit` whatever t is), and a primitive no lane's line meets is skipped by ballot.  In ANY mode a wave whose
 * lanes are all blocked leaves the loops.
 * GRID: the spheres through the uniform grid (wt_cast_grid), planes and lights scanned as in every flavour. */

#define WT_CAST_SPHERES 1u
#define WT_CAST_PLANES 2u
#define WT_CAST_LIGHTS 4u
#define WT_CAST_OPAQUE 8u

struct wt_cast_args {
    const float4* rays;         /* 2 per ray: {origin, tmax}, {dir, bits(ignore)} */
    float4* hits;               /* nearest: 2 per ray: {t, bits(id), normal.xy}, {normal.z, point} */
    unsigned char* blocked;     /* any: 1 per ray */
    unsigned n, flags, batches;
};

/* the definition's sphere test, the invariants of the origin (v = o - c, cc = v.v - |r r|) and of the direction (a = d.d) already taken: the
 * operations of wt_gb_ref_sphere in its order.  true = a candidate (hit && t <= tmax), its parameter in t.  D < 0 leaves before the roots. */
__device__ __forceinline__ bool wt_cast_sphere(f3 v, float cc, f3 d, float a, float tmax, float& t) {
#pragma clang fp contract(off)
    const float b = wt_gb_ref_dot(v, d);
    const float D = b * b + (-(a * cc));
    if (D < 0) return false;
    const float sD = sqrtf(D);
    const float t0 = (-b - sD) / a;
    t = (t0 < 0) ? (-b + sD) / a : t0;
    return !(t <= 0) && t <= tmax;
}

struct wt_cast_best { float t; unsigned id; bool any; };

__device__ __forceinline__ void wt_cast_take(wt_cast_best& B, float t, unsigned id) {
    B.any = true;
    if (t < B.t) { B.t = t; B.id = id; }
}

/* The spheres of one ray through the uniform grid: the walk of wt_grid_nearest / wt_ao_grid_spheres with the definition's test per entry.
 * `ignore` and OPAQUE filter per entry (the index of an entry is fetched for a candidate only).  The walk may only SKIP tests -- its result is
 * the in-order scan's:
 *  (1) every entry is tested with the scan's operations on the scan's words (grid_geom[k] = geom[grid_items[k]]), so a sphere the walk tests
 *      gets the scan's verdict and the scan's t; equal t takes the lower grid_items index, as the scan's strict `t < tbest` keeps the earlier
 *      sphere; a sphere listed in several cells is tested again with the same outcome.
 *  (2) no sphere the scan would have taken is skipped: a sphere met at t is listed in the cell the ray is in at t (scene_prep.c lists it in
 *      every cell its box, padded by 1e-3 cell, touches), and the walk visits the cells of the ray in order.  It ends early in two places: where
 *      the best so far lies inside the cells walked (tbest <= texit: a nearer sphere would be listed in one of them) and where the rest of the
 *      walk lies beyond the ray's end (texit > tmax: a sphere met there is no candidate).  Both compare a cell boundary computed in the BUILD's
 *      arithmetic (one reciprocal per axis: v_rcp_f32 in the fast build) with a t or tmax in the REFERENCE's, which differ by rounding where D
 *      cancels; the padding covers an ulp of the boundary, not an error of t.  So once either condition holds the walk takes ONE MORE cell
 *      before it stops: a candidate whose computed t and true cell disagree about the boundary just passed is listed there.  For the same
 *      reason the walk starts unclipped (wt_grid_begin with +inf, as wt_grid_occluded): a tmax that ends near the grid's face must not decide
 *      whether the grid is entered at all.  A nearest query ends at the grid's far side like wt_grid_nearest.
 * A ray wt_ray_walkable rejects (NaN, infinite, all-zero direction: the unwalkable ones) has no cells: it takes the in-order scan. */
template <bool ANY>
__device__ __forceinline__ void wt_cast_grid(const whitted_params& P, f3 o, f3 d, float a, float tmax, unsigned ignore, bool opaque, wt_cast_best& B) {
    if (!wt_ray_walkable(o, d)) {
        /* An all-zero direction -- the ray built from the zero normal of a first query's miss -- is spared the scan: with d = 0 the test gives
         * A = 0, B = v.0 = 0 (NaN for an origin that is not finite), D = 0 * 0 + (-(0 * C)) = 0 or NaN, t0 = (-0 - 0) / 0 = NaN, and a NaN t is
         * never <= tmax: no sphere is a candidate, which is what returning here leaves.  (Measured: 6 % such rays among 2 M made the 10 000-
         * sphere scene's short-ray query 3.5 ms instead of 0.06: a wave waits for its one lane that scans every sphere.) */
        if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return;
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            if (i == ignore || (opaque && (__float_as_uint(s.w) >> 31))) continue;
            const f3 v = o - mk3(s.x, s.y, s.z);
            float t;
            if (wt_cast_sphere(v, wt_gb_ref_dot(v, v) - fabsf(s.w), d, a, tmax, t)) wt_cast_take(B, t, i);
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
            if (wt_cast_sphere(v, wt_gb_ref_dot(v, v) - fabsf(s.w), d, a, tmax, t) && !(t > B.t)) {
                const unsigned i = P.grid_items[k];
                if (i == ignore) continue;
                if (ANY) { B.any = true; return; }
                B.any = true;
                if (t < B.t || (t < INFINITY && i < B.id)) { B.t = t; B.id = i; }      /* (t == B.t here unless t < B.t) */
            }
        }
        if (!more) return;
        if ((B.any && B.t <= texit) || texit > tmax) ending = true;
        w = nw; cur = nxt;
    }
}

template <bool GEOM_LDS, bool GRID, bool ANY>
__global__ void __launch_bounds__(WT_BLOCK) wt_cast(const whitted_params P, const wt_cast_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;
    const bool opaque = (A.flags & WT_CAST_OPAQUE) != 0u;

    for (unsigned bt = 0; bt < A.batches; bt++) {      /* (wave-uniform) */
        const unsigned base = (blockIdx.x * A.batches + bt) * 64u;      /* (the launcher keeps groups * batches * 64 below 2^31) */
        if (base >= A.n) break;
        const bool valid = base + lane < A.n;
        const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last ray and tests nothing) */
        const float4 r0 = A.rays[2 * (size_t)k], r1 = A.rays[2 * (size_t)k + 1];
        const f3 o = mk3(r0.x, r0.y, r0.z), d = mk3(r1.x, r1.y, r1.z);
        const float tmax = r0.w;
        const unsigned ignore = __float_as_uint(r1.w);
        const float a = wt_gb_ref_dot(d, d);
        wt_cast_best B;
        B.t = INFINITY; B.id = WT_GB_ID_NONE; B.any = false;
        bool live = valid;      /* the lane still has tests to make */

        if (A.flags & WT_CAST_SPHERES) {
            if (GRID) {
                if (live) wt_cast_grid<ANY>(P, o, d, a, tmax, ignore, opaque, B);
                if (ANY) live = live && !B.any;
            }
            for (unsigned i = 0; !GRID && i < P.ns; i++) {
                if (ANY && __builtin_amdgcn_ballot_w64(live) == 0ull) break;      /* everybody is blocked */
                const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
                const f3 v = o - mk3(s.x, s.y, s.z);
                bool ok;
                float b, D;
                {
#pragma clang fp contract(off)
                    const float cc = wt_gb_ref_dot(v, v) - fabsf(s.w);
                    b = wt_gb_ref_dot(v, d);
                    D = b * b + (-(a * cc));
                    ok = live && i != ignore && !(opaque && (__float_as_uint(s.w) >> 31)) && !(D < 0);
                }
                if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;      /* nobody's line meets this one */
                if (ok) {
#pragma clang fp contract(off)
                    const float sD = sqrtf(D);
                    const float t0 = (-b - sD) / a;
                    const float t = (t0 < 0) ? (-b + sD) / a : t0;
                    if (!(t <= 0) && t <= tmax) { wt_cast_take(B, t, i); if (ANY) live = false; }
                }
            }
        }
        if (A.flags & WT_CAST_PLANES) {
            for (unsigned i = 0; i < P.np; i++) {
                if (ANY && __builtin_amdgcn_ballot_w64(live) == 0ull) break;
                const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                float t;
                if (live && (WT_GB_KIND_PLANE | i) != ignore && wt_gb_ref_plane(o, d, pn, p0, t) && t <= tmax) {
                    wt_cast_take(B, t, WT_GB_KIND_PLANE | i);
                    if (ANY) live = false;
                }
            }
        }
        if (A.flags & WT_CAST_LIGHTS) {
            for (unsigned i = 0; i < P.nl; i++) {
                if (ANY && __builtin_amdgcn_ballot_w64(live) == 0ull) break;
                const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * i);
                const f3 v = o - mk3(l0.x, l0.y, l0.z);
                float t;
                if (live && (WT_GB_KIND_LIGHT | i) != ignore && wt_cast_sphere(v, wt_gb_ref_dot(v, v) - fabsf(l0.w), d, a, tmax, t)) {
                    wt_cast_take(B, t, WT_GB_KIND_LIGHT | i);
                    if (ANY) live = false;
                }
            }
        }

        if (!valid) continue;
        if (ANY) { A.blocked[k] = B.any ? 1 : 0; continue; }
        f3 ip = mk3(0, 0, 0), nrm = mk3(0, 0, 0);
        if (B.id != WT_GB_ID_NONE) {      /* the winner's point and normal: wt_gbuffer's, without the EPSILON offset */
            const unsigned kind = B.id >> 30, index = B.id & 0x3FFFFFFFu;
            ip = wt_gb_ref_madd(d, B.t, o);
            if (kind == 1u) {
                const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * index);
                nrm = mk3(pn.x, pn.y, pn.z);      /* never flipped toward the ray */
            } else {
                const float4 s = wt_geom<GEOM_LDS>(P, sg, kind == 0u ? index : g_lgt + 2 * index);
                nrm = wt_gb_ref_normalize(ip - mk3(s.x, s.y, s.z));
            }
        }
        A.hits[2 * (size_t)k] = make_float4(B.t, __uint_as_float(B.id), nrm.x, nrm.y);
        A.hits[2 * (size_t)k + 1] = make_float4(nrm.z, ip.x, ip.y, ip.z);
    }
}
