/* whitted_terms.inc -- what a segment adds to its path's radiance (whitted_hit.inc, whitted_shade.inc) and where a pushed parent goes
 * (whitted_bounce.inc), in the forms of the per-lane loop: added to `rgb` at once, parent on the lane's DFS stack (the child's sum then starts at 0).  The
 * tree-parallel tail (whitted_tpt.inc) redefines the macros around its own inclusions and re-includes this file after them.
 * WT_BOUNCE_LAST (read after depth++): the segment ends its path at the depth limit, so nothing its bounce computes is read again (whitted_bounce.inc). */
#undef WT_HIT_COLOUR
#undef WT_HIT_AMBIENT
#undef WT_SHADE_ADD
#undef WT_BOUNCE_PUSH
#undef WT_BOUNCE_LAST
#undef WT_MOTION
#define WT_MOTION mv        /* the scene time spheres are read at (wt_sphere_at): the lane's own; the tail, which moving launches do not enter, reads them unmoved */
#define WT_HIT_COLOUR(c) rgb = wt_madd3((c), f, rgb)
#define WT_HIT_AMBIENT(cf, a) rgb = wt_madd3((cf), (a), rgb)
#define WT_SHADE_ADD(li, l1, soft, dl, spec, diff) rgb = wt_light_add(rgb, (l1), (soft), (dl), (spec), (diff), ks, kd)
#define WT_BOUNCE_PUSH(rec) do { \
        if (SCRL == 0 || sp < LDSL) { _Pragma("unroll") for (int w_ = 0; w_ < WT_REC; w_++) s_stk[(sp * WT_REC + w_) * WT_BLOCK + tid] = (rec)[w_]; } \
        else { _Pragma("unroll") for (int w_ = 0; w_ < WT_REC; w_++) deep[(sp - LDSL) * WT_REC + w_] = (rec)[w_]; } \
        sp++; rgb = mk3(0, 0, 0); } while (0)
#define WT_BOUNCE_LAST (depth >= D && !P.untrimmed)
