/* whitted_bounce.inc -- Fresnel, reflection and the refraction child of a shaded hit (raytracing.cl:139-179);
 * textually included twice by whitted_trace.inc.  WT_BOUNCE_PUSH(rec) takes the parent record (the reflected continuation): the per-lane
 * loop stores it on the lane's DFS stack, the tree-parallel tail makes it a node of its own. */
            /* ---- Fresnel, reflection, refraction child (raytracing.cl:139-179) --- */
            /* On a path's last level (WT_BOUNCE_LAST: depth >= D after the step below) no child is pushed, and whitted_pop.inc then overwrites
             * o, d, depth, n1 and f from the parent's record or ends the lane: nothing the block computes is read again, and a wave none of whose
             * lanes goes further branches over it.  (`o = ip` stays in front of the branch: the old origin then dies on both paths; with the move
             * inside the block the shaped kernel spilled five more registers, one of them inside the loop.) */
            o = ip;
            depth++;
            if (!(WT_BOUNCE_LAST)) {
            const f3 incident = d;
            float n2 = (n1 == WT_DEFAULT_N) ? m.n : WT_DEFAULT_N;   /* binary media model */
            float ra = m.reflectivity;
            if (m.dielectric) ra = m.reflectivity + (1.0f - m.reflectivity) * wt_schlick(n1, n2, incident, nrm);
            const float old_f = f;
            f *= ra;
            d = wt_reflect(d, nrm);
            /* a child pushed at depth == D would end at once and add nothing: skip it */
            if (m.transparent && sp + 1 < D && ra < 1.0f && depth < D) {
                f3 co = o, cn = nrm;
                if (n1 < n2) co = co - nrm * (2 * WT_EPSILON);   /* entering */
                else cn = nrm * -1.0f;                           /* exiting: flip after the reflection was built */
                f3 cd;
                if (wt_refract(n1, n2, incident, cn, cd)) {      /* TIR drops the child */
                    if (COUNT) c_push++;
                    /* save the parent (the reflected continuation) */
                    float rec[WT_REC] = {o.x, o.y, o.z, d.x, d.y, d.z, rgb.x, rgb.y, rgb.z,
                                         __int_as_float(depth), n1, f};
                    WT_BOUNCE_PUSH(rec);
                    o = co; d = cd;                               /* (the child's sum starts at 0: part of WT_BOUNCE_PUSH) */
                    n1 = n2; f = old_f * (1.0f - ra);
                }
            }
            }
