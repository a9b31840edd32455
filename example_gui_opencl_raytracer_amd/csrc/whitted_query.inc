/* whitted_query.inc -- what the ray queries share: the one candidate scan of wt_cast (whitted_cast.inc) and wt_cast_layers
 * (whitted_layers.inc), and the sphere test that the ambient occlusion pass (whitted_ao.inc) makes too.  Included by whitted_launch.inc ahead of
 * those three, so it exists in the fast and the strict unit.  The arithmetic is csrc/ref_tests.h, the one text the host definitions
 * (cast_host.c) are compiled from too -- IEEE square root and divide, no fused operation -- so both builds give the host's bits.
 *
 * A query kernel loads a lane's ray (wt_query_load), hands it to wt_query_scan with a SINK, and stores what the sink holds.  The scan
 * enumerates the ray's candidates -- a primitive that takes part, is not `ignore`, is hit, and at t <= tmax -- and the sink decides what becomes
 * of a candidate (t, id): wt_cast keeps the nearest or raises a flag, wt_cast_layers keeps the K nearest.  A sink is a struct with
 *   FIRST              (constant) the first candidate settles the lane: it goes dead, a wave of dead lanes leaves each loop, the walk returns
 *   take(t, id)        a candidate of the in-order scan (ascending id)
 *   grid_wants(t)      the grid walk's prefilter: can a candidate at t matter?  Only then is its index fetched and compared with `ignore`
 *   grid_take(t, id)   a candidate of the grid walk that grid_wants has just passed, in whatever order the cells present it (and again from
 *                      every cell that lists it)
 *   grid_done(texit)   the walk holds everything that can matter to the sink among the cells up to parameter texit
 * passed by reference into force-inlined functions: what a sink holds stays in registers.
 *
 * Flat scan: the primitives are the outer loop, fetched wave-uniformly with wt_geom; D < 0 leaves before the square root and the divides (the
 * definition's verdict is then `no hit` whatever t is), and a sphere no lane's line meets is skipped by ballot.
 * GRID: the spheres through the uniform grid (wt_query_grid), planes and lights scanned as in every flavour. */

#define WT_CAST_SPHERES 1u
#define WT_CAST_PLANES 2u
#define WT_CAST_LIGHTS 4u
#define WT_CAST_OPAQUE 8u

/* the definition's sphere test of the ray (o, d), a = d.d already taken, against {c, +-r r} = s: ref_sphere_query over the origin's invariants.
 * true = a candidate (hit && t <= tmax), its parameter in t. */
__device__ __forceinline__ bool wt_query_sphere(f3 o, float4 s, f3 d, float a, float tmax, float& t) {
    const ref_v3 v = ref_sub(rv3(o), rv3(s));
    return ref_sphere_query(v, ref_sphere_cc(v, s.w), rv3(d), a, tmax, &t);
}

struct wt_query_ray { f3 o, d; float tmax; unsigned ignore; float a; };      /* a = d.d */

/* ray k of `rays`: 2 float4 per ray, {origin, tmax}, {dir, bits(ignore)} */
__device__ __forceinline__ wt_query_ray wt_query_load(const float4* rays, unsigned k) {
    const float4 r0 = rays[2 * (size_t)k], r1 = rays[2 * (size_t)k + 1];
    wt_query_ray r;
    r.o = mk3(r0.x, r0.y, r0.z); r.d = mk3(r1.x, r1.y, r1.z);
    r.tmax = r0.w;
    r.ignore = __float_as_uint(r1.w);
    r.a = wt_ref_dot(r.d, r.d);
    return r;
}

/* The spheres of one ray through the uniform grid: the walk of wt_grid_nearest / wt_ao_grid_spheres with the definition's test per entry.
 * OPAQUE and `ignore` filter per entry (the index of an entry is fetched for a candidate the sink wants only).  The walk may only SKIP tests --
 * what it leaves in the sink is what the in-order scan leaves:
 *  (1) every entry is tested with the scan's operations on the scan's words (grid_geom[k] = geom[grid_items[k]]), so a sphere the walk tests
 *      gets the scan's verdict and the scan's t.  A sphere listed in several cells is tested in each and yields the same t bits every time, and
 *      the cells present their spheres in no particular order, so a sink orders by the key (t, id): the nearest sink takes an equal t only
 *      from a lower index, as the scan's strict `t < best` keeps the earlier sphere, and meeting its holder again changes nothing; the list
 *      sink drops a (t, id) it already holds (wt_layers_insert<DEDUPE>), so a primitive appears once -- which is why the layered query has no
 *      total count: the walk cannot tell how many distinct candidates it dropped.
 *  (2) no sphere the sink would have kept is skipped: a sphere met at t is listed in the cell the ray is in at t (scene_prep.c lists it in
 *      every cell its box, padded by 1e-3 cell, touches), and the walk visits the cells of the ray in order.  It ends early in two places:
 *      where what the sink still accepts lies inside the cells walked (grid_done(texit) -- the nearest so far, or the K-th entry of a list
 *      that holds K, is at t <= texit: a sphere with a smaller key has a t no larger, so it is listed in one of them) and where the rest of the
 *      walk lies beyond the ray's end (texit > tmax: a sphere met there is no candidate).  Both compare a cell boundary computed in the BUILD's
 *      arithmetic (one reciprocal per axis: v_rcp_f32 in the fast build) with a t or tmax in the REFERENCE's, which differ by rounding where D
 *      cancels; the padding covers an ulp of the boundary, not an error of t.  So once either condition holds the walk takes ONE MORE cell
 *      before it stops: a candidate whose computed t and true cell disagree about the boundary just passed is listed there.  For the same
 *      reason the walk starts unclipped (wt_grid_begin with +inf, as wt_grid_occluded): a tmax that ends near the grid's face must not decide
 *      whether the grid is entered at all.  A query ends at the grid's far side like wt_grid_nearest.
 * A ray wt_ray_walkable rejects (NaN, infinite, all-zero direction: the unwalkable ones) has no cells: it takes the in-order scan. */
template <class SINK>
__device__ __forceinline__ void wt_query_grid(const whitted_params& P, const wt_query_ray& r, bool opaque, SINK& S) {
    const f3 o = r.o, d = r.d;
    if (!wt_ray_walkable(o, d)) {
        /* An all-zero direction -- the ray built from the zero normal of a first query's miss -- is spared the scan: with d = 0 the test gives
         * A = 0, B = v.0 = 0 (NaN for an origin that is not finite), D = 0 * 0 + (-(0 * C)) = 0 or NaN, t0 = (-0 - 0) / 0 = NaN, and a NaN t is
         * never <= tmax: no sphere is a candidate, which is what returning here leaves.  (Measured: 6 % such rays among 2 M made the 10 000-
         * sphere scene's short-ray query 3.5 ms instead of 0.06: a wave waits for its one lane that scans every sphere.) */
        if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return;
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            if (i == r.ignore || (opaque && (__float_as_uint(s.w) >> 31))) continue;
            float t;
            if (wt_query_sphere(o, s, d, r.a, r.tmax, t)) S.take(t, i);
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
            float t;
            if (wt_query_sphere(o, s, d, r.a, r.tmax, t) && S.grid_wants(t)) {
                const unsigned i = P.grid_items[k];      /* (fetched for a candidate the sink can use only) */
                if (i == r.ignore) continue;
                S.grid_take(t, i);
                /* (the constant, not a value grid_take returns: a run-time `return` here cost the other sinks 6 VGPRs and 4-9 % of their
                 * time on the 10 000-sphere grid, profiles/r21_query_refactor_ab.txt) */
                if constexpr (SINK::FIRST) return;
            }
        }
        if (!more) return;
        if (S.grid_done(texit) || texit > r.tmax) ending = true;
        w = nw; cur = nxt;
    }
}

/* every candidate of the ray into the sink: the spheres (the flat scan, or the grid), then the planes, then the lights, each kind if `flags`
 * (WT_CAST_*) asks for it.  `valid`: the lane has a ray of its own; a lane without one runs along and tests nothing. */
template <bool GEOM_LDS, bool GRID, class SINK>
__device__ __forceinline__ void wt_query_scan(const whitted_params& P, const float4* sg, const wt_query_ray& r, unsigned flags, bool valid, SINK& S) {
    const f3 o = r.o, d = r.d;
    const float a = r.a, tmax = r.tmax;
    const unsigned ignore = r.ignore;
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;
    const bool opaque = (flags & WT_CAST_OPAQUE) != 0u;
    bool live = valid;      /* the lane still has tests to make */

    if (flags & WT_CAST_SPHERES) {
        if (GRID) {
            if (live) wt_query_grid(P, r, opaque, S);
            if constexpr (SINK::FIRST) live = live && !S.any;
        }
        for (unsigned i = 0; !GRID && i < P.ns; i++) {
            if (SINK::FIRST && __builtin_amdgcn_ballot_w64(live) == 0ull) break;      /* everybody is settled */
            const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
            const ref_v3 v = ref_sub(rv3(o), rv3(s));
            float b, D;
            const bool met = ref_sphere_disc(v, ref_sphere_cc(v, s.w), rv3(d), a, &b, &D);
            const bool ok = live && i != ignore && !(opaque && (__float_as_uint(s.w) >> 31)) && met;
            if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;      /* nobody's line meets this one */
            if (ok) {      /* (ref_sphere_query's second half) */
                const float t = ref_sphere_root(b, D, a);
                if (ref_candidate(t, tmax)) { S.take(t, i); if (SINK::FIRST) live = false; }
            }
        }
    }
    if (flags & WT_CAST_PLANES) {
        for (unsigned i = 0; i < P.np; i++) {
            if (SINK::FIRST && __builtin_amdgcn_ballot_w64(live) == 0ull) break;
            const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
            const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
            float t;
            if (live && (WT_GB_KIND_PLANE | i) != ignore && ref_plane(rv3(o), rv3(d), rv3(pn), rv3(p0), &t) && t <= tmax) {
                S.take(t, WT_GB_KIND_PLANE | i);      /* (kind 1 ids follow every sphere's) */
                if (SINK::FIRST) live = false;
            }
        }
    }
    if (flags & WT_CAST_LIGHTS) {
        for (unsigned i = 0; i < P.nl; i++) {
            if (SINK::FIRST && __builtin_amdgcn_ballot_w64(live) == 0ull) break;
            const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * i);
            float t;
            if (live && (WT_GB_KIND_LIGHT | i) != ignore && wt_query_sphere(o, l0, d, a, tmax, t)) {
                S.take(t, WT_GB_KIND_LIGHT | i);
                if (SINK::FIRST) live = false;
            }
        }
    }
}
