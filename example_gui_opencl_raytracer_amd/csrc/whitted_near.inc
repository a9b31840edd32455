/* whitted_near.inc -- proximity queries (hip_wrap_ext.h: clw_probe, clw_ext_nearest_surface, clw_ext_within_reach, clw_ext_near_surfaces,
 * clw_ext_probe_device, clw_ext_near_surfaces_device): what lies around a CALLER's points.  wt_near answers, for every probe {p, reach} of a
 * linear range, the nearest surface (MODE 0: a clw_hit), whether any surface is within reach (MODE 1: a byte) or the K nearest surfaces (MODE 4
 * and 8: the compiled list capacity).  Included by whitted_launch.inc behind whitted_layers.inc, so it exists in the fast and the strict unit.
 * csrc/near_host.c is the definition; the arithmetic is csrc/ref_tests.h (ref_near_*), the one text the definition is compiled from too.  The
 * sinks are the ray queries' own, unchanged: wt_sink_nearest, wt_sink_any (whitted_cast.inc), wt_sink_list<C> (whitted_layers.inc), with the
 * distance d where a ray has its parameter t.  No trace kernel and no other pass is touched.
 *
 * Mapping: wt_cast's -- one probe per lane, one wave per workgroup, one batch of 64 probes; a probe is one float4 load (and one word of
 * `ignore`, if the caller gave any); a lane past the end tests nothing and stores nothing.  The scene is staged by wt_stage_scene, read from
 * global memory, or, for the spheres, read through the uniform grid.  The winner's normal and point are evaluated once, after the scan.
 *
 * Flat scan (wt_near_scan): the primitives are the outer loop, fetched wave-uniformly with wt_geom; a primitive that is no lane's candidate is
 * skipped by ballot; in the ANY mode a wave whose lanes are all settled leaves each loop.
 *
 * GRID (wt_near_grid): the spheres of a probe through the cells of its BOX, planes and lights scanned as in every flavour.  With
 *     reach+ = max(reach, 0),  pad_a = 1e-5 * (reach+ + |p_a|),  R_a = reach+ + pad_a            (float32, each operation rounded once)
 * the box spans, on axis a, the cells cell_a(p_a - R_a) .. cell_a(p_a + R_a), where cell_a(x) = clamp(floor((x - gmin_a) * inv_a), 0, res_a - 1)
 * is scene_prep.c's own cell_index, in its operations.  The cells present their spheres in no order and list a sphere several times: the sinks'
 * grid_wants / grid_take order by the key (d, id) and drop repeats (whitted_query.inc, (1)), so what the box leaves in a sink is what the
 * in-order scan leaves, PROVIDED every candidate sphere is listed in some cell of the box.  (grid_done is not used: nothing is walked.)
 *
 * Claim: a sphere {c, r} that is a candidate of the probe (d <= reach) is listed in a cell of the probe's box.  Needed of the scene: every
 * prepared word r * r is finite (the host checks it and plans the flat scan otherwise: with r * r = +inf, d = -inf for every finite p however
 * far away).  Needed of the probe: p and reach finite (a probe that is not takes the in-order scan or, with a finite reach and a point that is
 * not finite, has no sphere candidate at all: v has an infinite or NaN component, so m and d are +inf or NaN).
 * Proof.  u = 2^-24.  scene_prep.c lists the sphere in the product of the per-axis ranges cell_a(xlo_a) .. cell_a(xhi_a),
 * xhi_a = fl(fl(c_a + r) + pad_s), xlo_a = fl(fl(c_a - r) - pad_s), pad_s >= fl(1e-3 cell_a + 1e-5 (|c_a| + r)), and the box is a product of
 * per-axis ranges too, so they share a cell iff their ranges meet on every axis.  cell_a is monotone (a rounded subtraction of a constant, a
 * rounded product with inv_a > 0, floor and the clamp all are), so the ranges meet if fl(p_a - R_a) <= xhi_a and xlo_a <= fl(p_a + R_a); by
 * symmetry the first is shown.
 *  (i)   The sphere's side.  fl(c_a + r) >= c_a + r - u (|c_a| + r), and adding pad_s loses at most u of the sum, so
 *        xhi_a >= c_a + r + 0.97e-5 (|c_a| + r) + 0.99e-3 cell_a                                   (1e-5 and 1e-3 dwarf the few u).
 *  (ii)  The candidate.  d = fl(m - r') <= reach with r' = sqrtf(fl(r r)) <= r (1 + 2u) and m the computed |p - c|: three component
 *        differences, three products, two sums, one root -- at most four roundings of relative size u act on the way to m, so the true
 *        distance D = |p - c| <= m (1 + 4u).  The last subtraction is exact to u |m - r'|, so m <= r' + reach + u |m - r'|.  Together, with
 *        reach <= reach+:   |p_a - c_a| <= D <= (r + reach+) (1 + 8u) + e,   e = 1e-18 for the products and the r r that underflow.
 *        THIS is the rounding the pad must cover -- that of d against reach, relative to r + reach+, not an ulp of a cell boundary: its
 *        r-part, 8u r = 4.8e-7 r, is covered by the sphere's own 0.97e-5 r, its reach-part by the probe's 1e-5 reach+, and e by 0.99e-3 cell_a
 *        (a grid's bounds are padded by 1e-3 on each side and an axis has at most 1024 cells, so cell_a > 1e-6).
 *  (iii) The probe's side.  R_a >= (reach+ + 0.99e-5 (reach+ + |p_a|)) (1 - u), and fl(p_a - R_a) <= p_a - R_a + u (|p_a| + R_a), so
 *        fl(p_a - R_a) <= p_a - reach+ - 0.98e-5 reach+ - 0.98e-5 |p_a| + u |p_a| + 2u reach+ <= p_a - reach+ (1 + 8u)
 *                      <= c_a + r (1 + 8u) + e <= xhi_a.                                                                    qed
 *  A probe inside a sphere (d < 0, the negative reaches' only candidates) is the case reach+ = 0: p itself lies in the sphere's padded box.
 *  An infinite R_a (a reach near FLT_MAX) gives the whole axis.
 *
 * Probes that take the in-order scan over all spheres instead (per lane, as an unwalkable ray does in wt_query_grid): one whose reach is +-inf
 * (no box), and one whose box covers more than A.box_cells cells (launch_plan.h: WT_NEAR_BOX_CELLS; the answer is the same on both sides of the
 * cap, only the cost differs).  A NaN reach meets nothing and tests nothing.  The scanning lanes of a wave share ONE pass over the spheres,
 * fetched wave-uniformly like the flat scan: a wave with at least one such lane pays ns fetches and tests on top of its largest box, during
 * which the lanes that took their box idle -- so a few scattered unlimited probes among 2 M cost every wave they sit in a full scan, and a
 * caller who has many does better to sort them together (or to ask with a finite reach). */

struct wt_near_args {
    const float4* probes;       /* 1 per probe: {point, reach} */
    const unsigned* ignore;     /* 1 word per probe, or null = nothing is ignored */
    float4* hits;               /* MODE 0: 2 per probe: {d, bits(id), normal.xy}, {normal.z, point} */
    unsigned char* within;      /* MODE 1: 1 per probe */
    float* d;                   /* MODE 4, 8: K * n, layer-major */
    unsigned* id;               /* MODE 4, 8: K * n, layer-major */
    unsigned n, flags, K, box_cells;
};

struct wt_near_probe { f3 p; float reach; unsigned ignore; };

/* scene_prep.c's cell_index of floor((x - gmin) * inv) on axis a, in its operations */
__device__ __forceinline__ int wt_near_cell(const whitted_params& P, int a, float x) {
    const float f = floorf((x - P.grid_min[a]) * P.grid_inv[a]);
    return !(f >= 0.0f) ? 0 : (f >= (float)P.grid_res[a] ? P.grid_res[a] - 1 : (int)f);
}

/* The spheres of one probe through the cells of its box (the header's proof).  false = the probe has no box to enumerate (its reach is
 * infinite, or the box covers more than `box_cells` cells): the caller scans every sphere for it.  The cell index is x-fastest and cell c
 * holds the entries grid_start[c] .. grid_start[c + 1], so a row of the box along x is ONE run of entries: two fetches of the start table
 * per row, not per cell. */
template <class SINK>
__device__ __forceinline__ bool wt_near_grid(const whitted_params& P, const wt_near_probe& q, bool opaque, unsigned box_cells, SINK& S) {
    const f3 p = q.p;
    const float reach = q.reach;
    if (reach != reach) return true;                                   /* a NaN reach: no candidate */
    if (!(fabsf(reach) < INFINITY)) return false;
    if (!(fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY)) return true;      /* d is +inf or NaN for every sphere: none <= a finite reach */
    const float rp = fmaxf(reach, 0.0f);
    const float pc[3] = {p.x, p.y, p.z};
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float R = rp + 1e-5f * (rp + fabsf(pc[a]));
        lo[a] = wt_near_cell(P, a, pc[a] - R);
        hi[a] = wt_near_cell(P, a, pc[a] + R);
    }
    /* (at most 1024 cells per axis: the product fits 32 bits) */
    const unsigned cells = (unsigned)(hi[0] - lo[0] + 1) * (unsigned)(hi[1] - lo[1] + 1) * (unsigned)(hi[2] - lo[2] + 1);
    if (cells > box_cells) return false;
    const ref_v3 rp3 = rv3(p);
    for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++) {
            const unsigned row = ((unsigned)z * (unsigned)P.grid_res[1] + (unsigned)y) * (unsigned)P.grid_res[0];
            const unsigned b = P.grid_start[row + (unsigned)lo[0]], e = P.grid_start[row + (unsigned)hi[0] + 1u];
            for (unsigned k = b; k < e; k++) {
                const float4 s = ((const float4*)P.grid_geom)[k];
                if (opaque && (__float_as_uint(s.w) >> 31)) continue;
                const float d = ref_near_sphere(ref_sub(rp3, rv3(s)), s.w);
                if (ref_near_candidate(d, reach) && S.grid_wants(d)) {
                    const unsigned i = P.grid_items[k];      /* (fetched for a candidate the sink can use only) */
                    if (i == q.ignore) continue;
                    S.grid_take(d, i);
                    if constexpr (SINK::FIRST) return true;      /* (the constant: whitted_query.inc, wt_query_grid) */
                }
            }
        }
    return true;
}

/* every candidate of the probe into the sink: the spheres (the flat scan, or the grid), then the planes, then the lights, each kind if `flags`
 * (WT_CAST_*) asks for it.  `valid`: the lane has a probe of its own; a lane without one runs along and tests nothing. */
template <bool GEOM_LDS, bool GRID, class SINK>
__device__ __forceinline__ void wt_near_scan(const whitted_params& P, const float4* sg, const wt_near_probe& q, unsigned flags, unsigned box_cells,
                                             bool valid, SINK& S) {
    const ref_v3 p = rv3(q.p);
    const float reach = q.reach;
    const unsigned ignore = q.ignore;
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;
    const bool opaque = (flags & WT_CAST_OPAQUE) != 0u;
    bool live = valid;      /* the lane still has tests to make */

    if (flags & WT_CAST_SPHERES) {
        bool scans = live;      /* the lane takes the in-order scan over all spheres */
        if (GRID) scans = live && !wt_near_grid(P, q, opaque, box_cells, S);
        if (!GRID || __builtin_amdgcn_ballot_w64(scans) != 0ull)
            for (unsigned i = 0; i < P.ns; i++) {
                if (SINK::FIRST && __builtin_amdgcn_ballot_w64(scans) == 0ull) break;      /* everybody is settled */
                const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
                const float d = ref_near_sphere(ref_sub(p, rv3(s)), s.w);
                const bool ok = scans && i != ignore && !(opaque && (__float_as_uint(s.w) >> 31)) && ref_near_candidate(d, reach);
                if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;      /* nobody's candidate */
                if (ok) { S.take(d, i); if (SINK::FIRST) scans = false; }
            }
        if constexpr (SINK::FIRST) live = live && !S.any;
    }
    if (flags & WT_CAST_PLANES) {
        for (unsigned i = 0; i < P.np; i++) {
            if (SINK::FIRST && __builtin_amdgcn_ballot_w64(live) == 0ull) break;
            const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
            const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
            const float d = fabsf(ref_near_plane_s(p, rv3(pn), rv3(p0)));
            if (live && (WT_GB_KIND_PLANE | i) != ignore && ref_near_candidate(d, reach)) {
                S.take(d, WT_GB_KIND_PLANE | i);      /* (kind 1 ids follow every sphere's) */
                if (SINK::FIRST) live = false;
            }
        }
    }
    if (flags & WT_CAST_LIGHTS) {
        for (unsigned i = 0; i < P.nl; i++) {
            if (SINK::FIRST && __builtin_amdgcn_ballot_w64(live) == 0ull) break;
            const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * i);
            const float d = ref_near_sphere(ref_sub(p, rv3(l0)), l0.w);
            if (live && (WT_GB_KIND_LIGHT | i) != ignore && ref_near_candidate(d, reach)) {
                S.take(d, WT_GB_KIND_LIGHT | i);
                if (SINK::FIRST) live = false;
            }
        }
    }
}

/* the sink of a MODE: 0 the nearest, 1 any, 4 / 8 the list of that capacity (K is the list's length; the other two do not read it) */
struct wt_near_nearest : wt_sink_nearest { __device__ __forceinline__ explicit wt_near_nearest(unsigned) {} };
struct wt_near_any : wt_sink_any { __device__ __forceinline__ explicit wt_near_any(unsigned) {} };
template <int MODE> struct wt_near_sink { typedef wt_sink_list<MODE> type; };
template <> struct wt_near_sink<0> { typedef wt_near_nearest type; };
template <> struct wt_near_sink<1> { typedef wt_near_any type; };

template <bool GEOM_LDS, bool GRID, int MODE>
__global__ void __launch_bounds__(WT_BLOCK) wt_near(const whitted_params P, const wt_near_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;

    const unsigned base = blockIdx.x * 64u;      /* (the launcher keeps groups * 64 below 2^31) */
    if (base >= A.n) return;
    const bool valid = base + lane < A.n;
    const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last probe, tests nothing and stores nothing) */
    const float4 r0 = A.probes[k];
    wt_near_probe q;
    q.p = mk3(r0.x, r0.y, r0.z); q.reach = r0.w;
    q.ignore = A.ignore ? A.ignore[k] : WT_GB_ID_NONE;
    typename wt_near_sink<MODE>::type B(A.K);
    wt_near_scan<GEOM_LDS, GRID>(P, sg, q, A.flags, A.box_cells, valid, B);

    if (!valid) return;
    if constexpr (MODE == 1) A.within[k] = B.any ? 1 : 0;
    else if constexpr (MODE == 0) {
        f3 ip = mk3(0, 0, 0), nrm = mk3(0, 0, 0);
        if (B.id != WT_GB_ID_NONE) {      /* the winner: one fetch of the plane's two words, or of the sphere's or light's */
            const unsigned kind = B.id >> 30, index = B.id & 0x3FFFFFFFu;
            const unsigned at = kind == 0u ? index : P.ns + 2 * index + (kind == 1u ? 0u : 2 * P.np);
            const float4 g = wt_geom<GEOM_LDS>(P, sg, at);
            if (kind == 1u) {
                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, at + 1u);
                nrm = mk3(g.x, g.y, g.z);
                ip = fv3(ref_near_plane_point(rv3(q.p), rv3(g), ref_near_plane_s(rv3(q.p), rv3(g), rv3(p0))));
            } else {
                ref_v3 N, point;
                ref_near_sphere_point(rv3(q.p), rv3(g), g.w, &N, &point);
                nrm = fv3(N); ip = fv3(point);
            }
        }
        A.hits[2 * (size_t)k] = make_float4(B.t, __uint_as_float(B.id), nrm.x, nrm.y);
        A.hits[2 * (size_t)k + 1] = make_float4(nrm.z, ip.x, ip.y, ip.z);
    } else {
#pragma unroll
        for (int j = 0; j < MODE; j++)
            if ((unsigned)j < B.K) {
                A.d[(size_t)j * A.n + k] = B.lt[j];
                A.id[(size_t)j * A.n + k] = B.li[j];
            }
    }
}
