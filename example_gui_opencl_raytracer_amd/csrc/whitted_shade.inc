/* whitted_shade.inc -- Phong + soft shadows of one shaded hit (raytracing.cl:83-136); textually included by the per-lane loop of
 * whitted_trace.inc and by the shading pass of the tree-parallel tail (whitted_tpt.inc).
 * In: ip, nrm, view, m.shininess, ks, kd, rng.  The RNG stream is drawn in the reference's order (4 numbers per light, whether
 * or not its rays are traced).  What a light contributes goes through WT_SHADE_ADD(light, l1, soft, dl, spec, diff) -- the per-lane
 * loop adds it to rgb at once (wt_light_add), the tail stores the factors and adds them in its replay, in the same order. */
            if (GRID) {
                /* Big scenes: shadow rays walk the grid -- the two samples of a light together where the grid allows (P.grid_pair), else each on
                 * its own -- so there is nothing more to batch.  Lights and
                 * samples are REAL loops here -- one copy of the walk in the code instead of six (instruction cache,
                 * registers).  Same draws in the same order, same arithmetic per ray and the same order of additions
                 * to `rgb` as the batched form in the else-branch. */
#pragma unroll 1
                for (unsigned li = 0; li < P.nl; li++) {
                    const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * li);
                    const float4 l1 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * li + 1);
                    const light_terms L = wt_light_terms(l0, ip, nrm, view, m.shininess, ks, kd);
                    const bool need = L.need;
                    const bool wave_need = __builtin_amdgcn_ballot_w64(need) != 0;
                    float soft = 0.0f;
                    if (WT_SOFT == 2 && P.grid_pair) {
                        /* the two samples of the light share ONE walk, along the ray to the light's centre (wt_grid_shadow_pair) */
                        const float u1a = wt_xorshift(rng), u2a = wt_xorshift(rng), u1b = wt_xorshift(rng), u2b = wt_xorshift(rng);
                        if (COUNT) c_shadow += 2u;
                        float opp[2] = {0.0f, 0.0f};
                        if (wave_need) {
                            f3 rdp[2]; float tlp[2], a4p[2], a2p[2];
                            rdp[0] = wt_light_sample_dir(l0, l1, u1a, u2a, ip, tlp[0]);
                            rdp[1] = wt_light_sample_dir(l0, l1, u1b, u2b, ip, tlp[1]);
#pragma unroll
                            for (int q = 0; q < 2; q++) { const rayq rq = wt_shadow_rayq_scene<GEOM_LDS>(P, ip, rdp[q]); a4p[q] = rq.a4; a2p[q] = rq.a2; opp[q] = need ? 1.0f : 0.0f; }
                            if (COUNT && need) c_traced += 2u;
                            if (need) {
                                float lc;
                                const f3 dc = wt_normalize_len(mk3(l0.x, l0.y, l0.z) - ip, lc);
                                wt_grid_shadow_pair(P, ip, dc, lc, rdp, a4p, a2p, tlp, opp);
                            }
                            for (unsigned i = 0; i < P.np; i++) {
                                if (__builtin_amdgcn_ballot_w64(opp[0] != 0.0f || opp[1] != 0.0f) == 0) break;
                                const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                                const float num = wt_plane_pre(ip, n, p0);
                                if (wt_plane_blocks(num, n, rdp[0], tlp[0])) opp[0] = 0.0f;
                                if (wt_plane_blocks(num, n, rdp[1], tlp[1])) opp[1] = 0.0f;
                            }
                        }
                        soft += opp[0];
                        soft += opp[1];
                    } else
#pragma unroll 1
                    for (int j = 0; j < WT_SOFT; j++) {
                        const float u1 = wt_xorshift(rng), u2 = wt_xorshift(rng);
                        if (COUNT) c_shadow++;
                        float opq = 0.0f;
                        if (wave_need) {
                            float tlq;
                            const f3 rdq = wt_light_sample_dir(l0, l1, u1, u2, ip, tlq);
                            const rayq rq = wt_shadow_rayq_scene<GEOM_LDS>(P, ip, rdq);      /* big scene: the full quadratic */
                            opq = need ? 1.0f : 0.0f;
                            if (COUNT && need) c_traced++;
                            if (opq != 0.0f) opq = wt_grid_shadow(P, ip, rdq, rq.a4, rq.a2, tlq);
                            for (unsigned i = 0; i < P.np; i++) {
                                if (__builtin_amdgcn_ballot_w64(opq != 0.0f) == 0) break;
                                const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                                if (wt_plane_blocks(wt_plane_pre(ip, n, p0), n, rdq, tlq)) opq = 0.0f;
                            }
                        }
                        soft += opq;
                    }
                    WT_SHADE_ADD(li, l1, soft, L.dl, L.spec, L.diff);
                }
                WT_STAMP(WT_ST_SHADOW);     /* samples, walks and the lights' terms of a grid build, all under "shadow" */
            } else
            for (unsigned lb = 0; lb < SH::nl(P); lb += LCH) {
                f3 rd[NR];
                float tl[NR], a4[NR], a2[NR], op[NR], dl[LCH], spec[LCH], diff[LCH], opu[LCH];
                bool needk[LCH], known[LCH];
#pragma unroll
                for (int k = 0; k < LCH; k++) {
                    dl[k] = 1.0f; spec[k] = 0.0f; diff[k] = 0.0f; needk[k] = false; known[k] = false; opu[k] = 1.0f;
                    if (lb + k < SH::nl(P)) {                                   /* wave-uniform */
                        const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k));
                        const light_terms L = wt_light_terms(l0, ip, nrm, view, m.shininess, ks, kd);
                        dl[k] = L.dl; spec[k] = L.spec; diff[k] = L.diff; needk[k] = L.need;
                    }
                }
                /* which of these lights have the same shadow factor for every sample (wt_light_vis): their rays are not traced */
                bool chk[LCH];
                float opc[LCH];
#pragma unroll
                for (int k = 0; k < LCH; k++) { chk[k] = false; opc[k] = 0.0f; }
                if (CLASSES && P.vis != 0u) {
                    bool anyw = false;
#pragma unroll
                    for (int k = 0; k < LCH; k++) anyw |= needk[k];
                    if (__builtin_amdgcn_ballot_w64(anyw) != 0)
                        wt_light_vis<GEOM_LDS, LCH>(P, sg, g_pln, g_lgt, lb, ip, needk, LCH == 3 ? lb / 3u : ~0u, known, opu, WT_MOTION);
                    if (COUNT) {
#pragma unroll
                        for (int k = 0; k < LCH; k++) if (known[k]) c_known++;
                        if (P.vis == 2u) {                                  /* verification: classify AND trace */
#pragma unroll
                            for (int k = 0; k < LCH; k++) { chk[k] = known[k]; opc[k] = opu[k]; known[k] = false; }
                        }
                    }
                }
                /* which spheres can this wave's rays of the batch meet at all (wt_sphere_candidates)?  Asked BEFORE the samples exist: fewer registers are live here */
                unsigned long long cand = ~0ull;
                /* (not in a moving launch: the choice is made per WAVE from centres that are then per-lane values; testing every sphere gives the same factors) */
                if (SPHCULL && !WT_MOTION.on && P.ns >= WT_CULL_MIN_SPHERES && P.ns <= 64u) {  /* wave-uniform: C3's 64 spheres, not render.map's 4 */
                    bool part = false;
#pragma unroll
                    for (int k = 0; k < LCH; k++) part |= needk[k] && !known[k];
                    if (__builtin_amdgcn_ballot_w64(part) != 0) {
                        cand = wt_sphere_candidates<GEOM_LDS, LCH>(P, sg, g_lgt, lb, ip, part, s_cull, lane);
                        cand = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)cand)) |
                               ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(cand >> 32)) << 32);
                    }
                }
                bool any_sample = false;
#pragma unroll
                for (int k = 0; k < LCH; k++) {
                    const bool ex = lb + k < SH::nl(P);                     /* wave-uniform */
                    const bool sample = needk[k] && !known[k];
                    const bool wave_sample = __builtin_amdgcn_ballot_w64(sample) != 0;
                    any_sample |= wave_sample;
#pragma unroll
                    for (int j = 0; j < WT_SOFT; j++) {
                        const int q = k * WT_SOFT + j;
                        rd[q] = mk3(0, 0, 0); tl[q] = 0.0f; a4[q] = 0.0f; a2[q] = 0.0f; op[q] = 0.0f;
                        if (ex) {
                            /* xorshift in [0,4); the two angle products are fp64 multiplies rounded
                             * to fp32 (M_PI is a double constant, raytracing.cl:99-100) */
                            const float u1 = wt_xorshift(rng), u2 = wt_xorshift(rng);
                            if (COUNT) c_shadow++;
                            if (wave_sample) {
                                const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k));
                                const float4 l1 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k) + 1);
                                rd[q] = wt_light_sample_dir(l0, l1, u1, u2, ip, tl[q]);
                                const rayq rq = wt_shadow_rayq_scene<GEOM_LDS>(P, ip, rd[q]);
                                a4[q] = rq.a4; a2[q] = rq.a2;
                                op[q] = sample ? 1.0f : 0.0f;
                                if (COUNT && sample) c_traced++;
                            }
                        }
                    }
                }
                WT_STAMP(WT_ST_LIGHTS);
                /* (not in the high-occupancy deep flavour: its register cap turns the table's four values into spills, +3 % at C3) */
                /* (wt_trace_cull: in a tile's first iteration `cullb` carries the sphere classes no shadow ray of this shade can meet) */
                if (any_sample)
                    wt_shadow_batch<GEOM_LDS, NR, !(DEEP && wt_cfg<FLAGS>::occ), SPHCULL, FLAGS, CULL>(P, sg, g_pln, ip, rd, tl, a4, a2, op, LCH == 3 ? lb / 3u : ~0u, dl, cand, WT_MOTION,
                                                                                                    CULL ? (cullb >> WT_CULLB_SHADOW_SHIFT) & 15u : 0u);
                WT_STAMP(WT_ST_SHADOW);
#pragma unroll
                for (int k = 0; k < LCH; k++) {
                    if (lb + k < SH::nl(P)) {
                        const float4 l1 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k) + 1);
                        float soft = 0.0f;
#pragma unroll
                        for (int j = 0; j < WT_SOFT; j++) soft += known[k] ? opu[k] : op[k * WT_SOFT + j];
                        if (COUNT && chk[k]) {
                            bool bad = false;
#pragma unroll
                            for (int j = 0; j < WT_SOFT; j++) bad |= __float_as_uint(op[k * WT_SOFT + j]) != __float_as_uint(opc[k]);
                            if (bad) c_visbad++;
                        }
                        WT_SHADE_ADD(lb + k, l1, soft, dl[k], spec[k], diff[k]);
                    }
                }
                WT_STAMP(WT_ST_ADD);
            }
