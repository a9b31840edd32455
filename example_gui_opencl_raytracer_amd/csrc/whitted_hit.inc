/* whitted_hit.inc -- one path segment up to the shaded hit (textually included twice by whitted_trace.inc).
 * In: o, d, f, rgb, rng-independent.  Out: `ended` (light hit / sky miss added to rgb) or `shade` with
 * ip, nrm, m, view, ks, kd set.  findLightIntersection + findSolidIntersection + the miss branch of the
 * reference's loop (raytracing.cl:48-84, primitives.cl:262-394).
 * What a segment ADDS to its path's radiance goes through two macros, so that the tree-parallel tail (whitted_tpt.inc) can record
 * the terms instead and add them later, in the reference's order:
 *   WT_HIT_COLOUR(c)      a light sphere seen / the skybox texel of a miss:  rgb = c * f + rgb
 *   WT_HIT_AMBIENT(cf, a) the ambient term of a hit (cf = colour x throughput): rgb = cf * a + rgb
 * Spheres are read through wt_sphere_at with WT_MOTION: the lane's own scene time in the per-lane loop, none in the tail (whitted_terms.inc). */
            cost++;
            if (COUNT) {
                c_iter++;   /* lane-iterations; the first live lane books 64 per wave-iteration */
                unsigned long long live = __builtin_amdgcn_ballot_w64(true);
                if (lane == (unsigned)__builtin_ctzll(live)) c_witer += 64u;
            }
            /* P.unit_dirs (wave-uniform, set by the shim per SCENE so that the grid walk and the linear scan of one scene
             * share their arithmetic): the rays are this library's own and the scene is small -- see wt_rayq */
            /* LDS-geometry launches with rays generated in the kernel are unit-direction launches by construction (the shim stages
             * only scenes of <= 256 spheres): there a = 1 is a compile-time constant and its multiplies fold away */
            const rayq r = UNIT_CT ? wt_rayq<true>(o, d) : wt_rayq<false>(o, d, P.unit_dirs != 0u);

            /* ---- findLightIntersection (primitives.cl:262-318) ------------------------- */
            if (COUNT) c_probe++;
            bool lit = false;
            float tl = INFINITY;
            f3 lcol = mk3(0, 0, 0);
            /* four lights at a time: their float4s are fetched together (one wait), the four discriminants are
             * independent chains, and ONE ballot decides whether anybody needs the root half at all (a light sphere is
             * rarely in view).  Hits are then taken in index order, as in the reference's loop. */
            /* (a scene's last chunk may hold fewer than four lights -- render.map has three: its size is a wave-uniform switch, so
             * no discriminant is computed for a light that does not exist) */
            auto probe_chunk = [&](auto nc, const unsigned base) {
                constexpr int N = decltype(nc)::value;
                float4 l0[N]; float bq[N], Dq[N]; bool ok[N]; bool any = false;
#pragma unroll
                for (int k = 0; k < N; k++) l0[k] = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (base + k));
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const sph_pre pre = wt_sphere_pre(r.o, l0[k]);
                    ok[k] = wt_sphere_disc(pre, r.d, r.a4, bq[k], Dq[k]);
                    any |= ok[k];
                }
                if (__builtin_amdgcn_ballot_w64(any)) {
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        float t;
                        const bool hit = wt_sphere_root(bq[k], Dq[k], r.a2, t) && ok[k];
                        if (hit && !(t >= tl)) {
                            float4 l1 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (base + k) + 1);
                            tl = t;
                            f3 hp = wt_madd3(d, t, o);
                            float dist = wt_sqrt(dot3(o - hp, o - hp));
                            /* "(1/d*d)" = (1/d)*d, not inverse-square: kept (primitives.cl:287) */
                            lcol = mk3(l1.x, l1.y, l1.z) * (1 / dist * dist);
                            lit = true;
                        }
                    }
                }
            };
            /* (a tile whose primary rays all miss the line test of every light skips the chunks in its first iteration: the cull table, wave-uniform) */
            if (!(CULL && (cullb & WT_CULL_LIGHTS)))
            for (unsigned base = 0; base < SH::nl(P); base += 4u) {
                const unsigned left = SH::nl(P) - base;
                if (left >= 4u) probe_chunk(wt_int<4>{}, base);
                else if (left == 3u) probe_chunk(wt_int<3>{}, base);
                else if (left == 2u) probe_chunk(wt_int<2>{}, base);
                else probe_chunk(wt_int<1>{}, base);
            }
            if (__builtin_amdgcn_ballot_w64(lit)) { /* rare: a light sphere is in view */
                if (lit) {
                    if (GRID) {
                        if (wt_grid_occluded(P, r, tl)) lit = false;
                    }
                    for (unsigned i = 0; !GRID && i < SH::ns(P); i++) {
                        float4 s = wt_sphere_at<GEOM_LDS>(P, sg, i, WT_MOTION);
                        float t;
                        bool hit = wt_sphere(r, s, t);
                        if (hit && t <= tl && !(__float_as_uint(s.w) >> 31)) lit = false;
                    }
                    for (unsigned i = 0; i < SH::np(P); i++) {
                        float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                        float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                        float t;
                        bool hit = wt_plane(r, n, p0, t);
                        if (hit && t <= tl) lit = false;
                    }
                }
            }
            WT_STAMP(WT_ST_PROBE);
            if (lit) {
                WT_HIT_COLOUR(lcol);                                            /* raytracing.cl:52: rgb += colour x throughput */
                ended = true;
            } else {
                /* ---- findSolidIntersection (primitives.cl:322-394): nearest wins, strict
                 *      `_t >= t` keeps the earlier primitive on ties, spheres before planes */
                if (COUNT) c_seg++;
                float tbest = INFINITY;
                int best = -1;
                if (GRID) {
                    best = wt_grid_nearest(P, r, tbest);
                } else if (!(CULL && (cullb & WT_CULL_SPHERES))) {               /* (the cull table again: no lane's line meets any sphere) */
                    for (unsigned base = 0; base < SH::ns(P); base += 4u) {      /* four spheres at a time, see the light probe */
                        float4 s4[4]; float bq[4], Dq[4]; bool ok[4]; bool any = false;
#pragma unroll
                        for (int k = 0; k < 4; k++) s4[k] = wt_sphere_at<GEOM_LDS>(P, sg, min(base + k, SH::ns(P) - 1u), WT_MOTION);
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const sph_pre pre = wt_sphere_pre(r.o, s4[k]);
                            ok[k] = wt_sphere_disc(pre, r.d, r.a4, bq[k], Dq[k]) && (base + k < SH::ns(P));
                            any |= ok[k];
                        }
                        if (__builtin_amdgcn_ballot_w64(any)) {
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                if (__builtin_amdgcn_ballot_w64(ok[k]) == 0) continue;   /* nobody's line meets this one */
                                float t;
                                const bool hit = wt_sphere_root(bq[k], Dq[k], r.a2, t) && ok[k];
                                if (hit && !(t >= tbest)) { tbest = t; best = (int)(base + k); }
                            }
                        }
                    }
                }
                for (unsigned i = 0; i < SH::np(P); i++) {
                    float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                    float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                    float t;
                    bool hit = wt_plane(r, n, p0, t);
                    if (hit && !(t >= tbest)) { tbest = t; best = (int)(SH::ns(P) + i); }
                }
                WT_STAMP(WT_ST_NEAREST);
                if (best < 0) {
                    /* ---- miss: skybox (raytracing.cl:61-81) ------------------------------ */
                    if (COUNT) c_sky++;
                    WT_HIT_COLOUR(wt_texel_rgb(wt_skybox_fetch(P, d)));
                    ended = true;
                } else {
                    ip = wt_madd3(d, tbest, o);
                    prim = (unsigned)best;
                    textured = false;
                    if ((unsigned)best < SH::ns(P)) {
                        float4 s = wt_sphere_at<GEOM_LDS>(P, sg, (unsigned)best, WT_MOTION);
                        nrm = wt_normalize(ip - mk3(s.x, s.y, s.z));
                    } else {
                        unsigned pi = (unsigned)best - SH::ns(P);
                        float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * pi);
                        nrm = mk3(n.x, n.y, n.z);               /* never flipped toward the ray */
                        if (n.w != 0.0f) {                       /* texture_id >= 0 */
                            if (COUNT) c_tex++;
                            texpx = wt_plane_texel_fetch(P, pi, ip);   /* pre-offset point (primitives.cl:377) */
                            textured = true;
                        }
                    }
                    /* material of the winner, gathered from the raw arrays */
                    wt_mat_set_b(m, wt_mat_f4(P, prim, 1u, SH::ns(P)));
                    {
                        const float4 a_ = wt_mat_f4(P, prim, 0u, SH::ns(P));
                        m.rgb = mk3(a_.x, a_.y, a_.z);
                        wt_mat_set_c(m, wt_mat_f4(P, prim, 2u, SH::ns(P)));
                    }
                    ip = wt_madd3(nrm, WT_EPSILON, ip);
                    cost += 3u;
                    {   /* the ambient term (raytracing.cl:83-84): material colour -- for a textured plane its texel -- x throughput x ambient */
                        const f3 c_ = textured ? wt_texel_rgb(texpx) : m.rgb;
                        WT_HIT_AMBIENT(c_ * f, m.ambient);
                    }
                    view = wt_normalize(o - ip);
                    /* A surface whose specular and diffuse coefficients are both zero (glass) receives exactly
                     * +0 from every light whatever the shadow term is, provided the factors it multiplies are
                     * finite: its shadow rays are not traced (the RNG still advances).  Checked per light. */
                    ks = f * m.specular; kd = f * m.diffuse;
                    shade = true;
                }
            }
        