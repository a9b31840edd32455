/* whitted_ao.inc -- ray-traced ambient occlusion over the primary-hit buffers (hip_wrap_ext.h: clw_ao, clw_ext_render_ao): wt_ao_trace counts,
 * for every pixel of a range of whole rows, how many of K short any-hit rays over the hemisphere of its normal stay open; wt_ao_resolve turns
 * the counts into pixels.  Included by whitted_launch.inc behind whitted_query.inc, so both exist in the fast and the strict unit.
 * csrc/ao_host.c is their definition: its arithmetic and this file's are csrc/ref_tests.h, the one text both are compiled from -- IEEE square
 * root and divide, no fused operation -- so both builds give the host's bits.
 *
 * wt_ao_trace: one wave = one 8 x 8 tile = one workgroup, tiles row-major over the range (8 x 8 holds each of the 16 interleave patterns four
 * times).  The scene is staged by wt_stage_scene or read from global memory as in wt_gbuffer; the 16 K directions of the table follow it in LDS
 * (at most 8 KiB behind at most 16 KiB of geometry).  A lane builds its basis once and traces its rays in batches of WT_AO_BATCH = 8: the
 * batch's directions and their d.d live in registers (32 VGPRs -- all of K = 32 would be 128), its verdicts in one bit mask.  In the flat scan
 * the spheres are the outer loop and the batch the inner one: a wave-uniform wt_geom fetch and one v = o - c, v.v - r r per lane serve 64 x 8
 * tests.  Rays already occluded skip their tests; a wave with no open ray left in the batch leaves the loops.
 * With GRID a lane traces one ray at a time (a walk shares nothing with the lane's other rays): the ray walks the cells within `radius`
 * (wt_grid_begin / wt_grid_next, as wt_grid_occluded walks them) and applies the same test to the entries of grid_geom; a ray wt_ray_walkable
 * rejects takes the in-order scan.  Planes are scanned in both flavours. */

#define WT_AO_BATCH 8
#define WT_AO_FILTER 1u
#define WT_AO_COMPOSE 2u
#define WT_AO_TILE_W 32
#define WT_AO_TILE_H 8
#define WT_AO_LDS_W (WT_AO_TILE_W + 3)       /* halo: 2 to the left and above, 1 to the right and below */
#define WT_AO_LDS_H (WT_AO_TILE_H + 3)
#define WT_AO_ABSENT 0xFFFFFFFFu

struct wt_ao_args {
    const float* point;         /* 3 per pixel of the range */
    const float* normal;        /* 3 */
    const unsigned* ids;        /* 1 */
    const float4* dirs;         /* [16][K] */
    unsigned char* open;        /* 1 per pixel: rays not occluded */
    unsigned width, rows, first_row, tiles_per_row;
    unsigned K;                 /* 1..32 */
    float radius;               /* > 0, +inf = unlimited */
};

/* the definition's two tests with the origin's invariants already taken (ref_tests.h: ref_sphere_query, ref_plane_rest): met at t <= radius? */
__device__ __forceinline__ bool wt_ao_sphere(ref_v3 v, float cc, f3 d, float a, float radius) {
    float t;
    return ref_sphere_query(v, cc, rv3(d), a, radius, &t);
}
__device__ __forceinline__ bool wt_ao_plane(float num, float4 pn, f3 d, float radius) {
    float t;
    return ref_plane_rest(num, rv3(pn), rv3(d), &t) && t <= radius;
}

/* is some sphere met at t <= radius?  The walk of wt_grid_occluded, ended where the cells lie beyond `radius`: a sphere met at t <= radius is
 * listed in the cell the ray is in at t, and that cell is entered at a parameter <= radius.  Any material occludes. */
__device__ __forceinline__ bool wt_ao_grid_spheres(const whitted_params& P, f3 o, f3 d, float a, float radius) {
    if (!wt_ray_walkable(o, d)) {      /* no cells to walk: the in-order scan, whose comparisons define what such a ray meets */
        bool hit = false;
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            const ref_v3 v = ref_sub(rv3(o), rv3(s));
            if (wt_ao_sphere(v, ref_sphere_cc(v, s.w), d, a, radius)) hit = true;
        }
        return hit;
    }
    grid_walk w;
    if (!wt_grid_begin(P, o, d, radius, w)) return false;
    grid_cellrange cur = wt_grid_range(P, wt_grid_cell(P, w));
    for (;;) {
        const float texit = w.texit;
        grid_walk nw = w;
        const bool more = wt_grid_next(P, nw) && !(texit > radius);      /* the rest of the walk lies beyond the radius */
        grid_cellrange nxt; nxt.b = 0u; nxt.e = 0u;
        if (more) nxt = wt_grid_range(P, wt_grid_cell(P, nw));           /* in flight while this cell is tested */
        for (unsigned k = cur.b; k < cur.e; k++) {
            const float4 s = ((const float4*)P.grid_geom)[k];
            const ref_v3 v = ref_sub(rv3(o), rv3(s));
            if (wt_ao_sphere(v, ref_sphere_cc(v, s.w), d, a, radius)) return true;
        }
        if (!more) return false;
        w = nw; cur = nxt;
    }
}

template <bool GEOM_LDS, bool GRID>
__global__ void __launch_bounds__(WT_BLOCK) wt_ao_trace(const whitted_params P, const wt_ao_args A) {
    extern __shared__ float4 s_geom[];
    float4* s_dirs = s_geom + (GEOM_LDS ? P.geom_f4 : 0u);
    const unsigned lane = threadIdx.x & 63u;
    for (unsigned i = lane; i < 16u * A.K; i += WT_BLOCK) s_dirs[i] = A.dirs[i];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);      /* (ends in the barrier that covers the table too) */
    else __syncthreads();
    const float4* sg = s_geom;

    const unsigned x = (blockIdx.x % A.tiles_per_row) * 8u + (lane & 7u), y = (blockIdx.x / A.tiles_per_row) * 8u + (lane >> 3);
    const bool valid = x < A.width && y < A.rows;
    const size_t p = valid ? (size_t)y * A.width + x : 0u;      /* (a lane outside the range reads pixel 0 and traces nothing) */
    const unsigned id = A.ids[p], kind = id >> 30, index = id & 0x3FFFFFFFu;
    const bool surface = valid && ((kind == 0u && index < P.ns) || (kind == 1u && index < P.np));
    const f3 o = mk3(A.point[3 * p], A.point[3 * p + 1], A.point[3 * p + 2]);
    const f3 n = mk3(A.normal[3 * p], A.normal[3 * p + 1], A.normal[3 * p + 2]);
    ref_v3 bt, bu;
    ref_ao_basis(rv3(n), &bt, &bu);
    const float4* ld = s_dirs + ((x & 3u) | (((A.first_row + y) & 3u) << 2)) * A.K;
    const float radius = A.radius;
    const unsigned g_pln = P.ns;
    unsigned open = 0u;

    if (GRID) {
        /* a ray at a time: a walk shares nothing with the lane's other rays, and a batch's 32 registers are better left to the walk */
#pragma unroll 1
        for (unsigned i = 0; i < A.K; i++) {
            const float4 l = ld[i];
            const f3 d = fv3(ref_ao_dir(bt, bu, rv3(n), l.x, l.y, l.z));
            const float a = wt_ref_dot(d, d);
            bool hit = false;
            if (surface) {
                hit = wt_ao_grid_spheres(P, o, d, a, radius);
                for (unsigned k = 0; k < P.np && !hit; k++) {
                    const float4 pn = ((const float4*)P.geom)[g_pln + 2 * k];
                    const float4 p0 = ((const float4*)P.geom)[g_pln + 2 * k + 1];
                    hit = wt_ao_plane(ref_plane_num(rv3(o), rv3(pn), rv3(p0)), pn, d, radius);
                }
            }
            open += hit ? 0u : 1u;
        }
    }
    for (unsigned base = 0; !GRID && base < A.K; base += WT_AO_BATCH) {      /* (wave-uniform) */
        const unsigned nb = A.K - base < WT_AO_BATCH ? A.K - base : WT_AO_BATCH;
        f3 d[WT_AO_BATCH];
        float a[WT_AO_BATCH];
        float amax = 0.0f;      /* the largest d.d of the batch (a NaN one is left out: such a ray is never occluded) */
#pragma unroll
        for (int r = 0; r < WT_AO_BATCH; r++) {
            const float4 l = ld[base + ((unsigned)r < nb ? (unsigned)r : 0u)];
            d[r] = fv3(ref_ao_dir(bt, bu, rv3(n), l.x, l.y, l.z));
            a[r] = wt_ref_dot(d[r], d[r]);
            if ((unsigned)r < nb && a[r] > amax) amax = a[r];
        }
        unsigned live = surface ? (1u << nb) - 1u : 0u;      /* bit r: ray base + r is not occluded yet */

        {   /* ---- the spheres: the outer loop, the batch the inner one ---- */
            /* R bounds how far from o a ray of the batch can be occluded: a hit at t <= radius lies at distance t |d| <= radius sqrt(amax) */
            const float R = radius * sqrtf(amax);
            for (unsigned i = 0; i < P.ns; i++) {
                if (__builtin_amdgcn_ballot_w64(live != 0u) == 0ull) break;      /* nobody has an open ray left */
                const float4 s = wt_geom<GEOM_LDS>(P, sg, i);
                const ref_v3 v = ref_sub(rv3(o), rv3(s));
                const float vv = ref_dot(v, v), cc = ref_sphere_cc(v, s.w);      /* (v.v is taken once: the same operations on the same words) */
                /* The reach check: can a ray of this lane, of length <= radius, touch the sphere at all?  With r = the radius and |v| the
                 * distance of its centre, a ray that meets it does so no nearer than |v| - r, so it cannot when |v| - r > R.  The verdict
                 * skipped is the FLOAT test's, whose t carries rounding: v.v, v.d, d.d and v.v - r r are each within a few ulp of |v|^2
                 * |d|^2 scale, so D is off by at most ~16 ulp of (|v| |d|)^2 and its root -- and with it t |d| -- by at most 4 sqrt(ulp)
                 * |v| < 2^-9 |v| (the worst case is a grazing ray, D near 0).  The check therefore asks for |v| (1 - 2^-7) > r + R, four
                 * times that allowance and its own roundings (three ulp on either side), as v.v * 0.98 > (r + R)^2 with 0.98 < (1 - 2^-7)^2
                 * = 0.9844.  When it holds, o is outside the sphere by more than the allowance (no negative near root to confuse with the
                 * far one) and every computed t, if any, exceeds radius: the verdict is `not occluded`, which skipping leaves.  A NaN on
                 * either side compares false (nothing skipped); R = +inf (an unlimited radius, an overflowed d.d) never skips; v.v = +inf
                 * makes C infinite and D negative or NaN: not occluded either way. */
                float rr;
                {
#pragma clang fp contract(off)
                    rr = sqrtf(fabsf(s.w)) + R;
                    rr = rr * rr;
                }
                const bool reach = live != 0u && !(vv * 0.98f > rr);
                if (__builtin_amdgcn_ballot_w64(reach) == 0ull) continue;      /* wave vote: no lane's rays can reach this sphere */
                if (reach) {
#pragma unroll
                    for (int r = 0; r < WT_AO_BATCH; r++)
                        if (((live >> r) & 1u) && wt_ao_sphere(v, cc, d[r], a[r], radius)) live &= ~(1u << r);
                }
            }
        }

        for (unsigned i = 0; i < P.np; i++) {
            if (__builtin_amdgcn_ballot_w64(live != 0u) == 0ull) break;
            const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
            const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
            const float num = ref_plane_num(rv3(o), rv3(pn), rv3(p0));
#pragma unroll
            for (int r = 0; r < WT_AO_BATCH; r++)
                if (((live >> r) & 1u) && wt_ao_plane(num, pn, d[r], radius)) live &= ~(1u << r);
        }
        open += (unsigned)__builtin_popcount(live);
    }
    if (valid) A.open[p] = (unsigned char)(surface ? open : A.K);
}

/* ---- counts -> pixels: integers only (ref_tests.h: ref_ao_level, _grey, _compose), as in csrc/ao_host.c: clw_host_ao_resolve --------------------------------
 * One work-item per pixel, a workgroup of 256 per tile of 32 x 8 pixels as the overlay's.  With FILTER the counts and ids of the tile and of
 * its halo -- 2 to the left and above, 1 to the right and below: 35 x 11 entries -- are staged in LDS, an absent pixel as WT_AO_ABSENT in the
 * count plane; a pixel then sums the entries of its 4 x 4 window that are present and carry its id.  Without it a pixel reads its own count. */
struct wt_ao_resolve_args {
    const unsigned char* open;
    const unsigned* ids;
    const unsigned* frame;      /* read with COMPOSE only */
    unsigned* out;
    unsigned width, rows, tiles_per_row;
    unsigned K, strength, compose;
};

template <bool FILTER>
__global__ void __launch_bounds__(WT_AO_TILE_W * WT_AO_TILE_H) wt_ao_resolve(const wt_ao_resolve_args A) {
    __shared__ unsigned s_cnt[FILTER ? WT_AO_LDS_H : 1][FILTER ? WT_AO_LDS_W : 1];
    __shared__ unsigned s_id[FILTER ? WT_AO_LDS_H : 1][FILTER ? WT_AO_LDS_W : 1];
    const unsigned tid = threadIdx.x;
    const unsigned lx = tid & (WT_AO_TILE_W - 1u), ly = tid / WT_AO_TILE_W;
    const unsigned x0 = (blockIdx.x % A.tiles_per_row) * WT_AO_TILE_W, y0 = (blockIdx.x / A.tiles_per_row) * WT_AO_TILE_H;
    const unsigned x = x0 + lx, y = y0 + ly;
    if (FILTER) {
        for (unsigned e = tid; e < WT_AO_LDS_W * WT_AO_LDS_H; e += WT_AO_TILE_W * WT_AO_TILE_H) {
            const unsigned tx = e % WT_AO_LDS_W, ty = e / WT_AO_LDS_W;
            /* pixel (gx, gy) of the range; coordinates left of or above it wrap to huge values and fail the same compare */
            const unsigned gx = x0 + tx - 2u, gy = y0 + ty - 2u;
            const bool present = gx < A.width && gy < A.rows;
            const size_t q = present ? (size_t)gy * A.width + gx : 0u;
            s_cnt[ty][tx] = present ? (unsigned)A.open[q] : WT_AO_ABSENT;
            s_id[ty][tx] = present ? A.ids[q] : 0u;
        }
        __syncthreads();
    }
    if (!(x < A.width && y < A.rows)) return;
    const size_t p = (size_t)y * A.width + x;
    unsigned S, m;
    if (FILTER) {
        const unsigned id = s_id[ly + 2u][lx + 2u];
        S = 0u; m = 0u;
#pragma unroll
        for (unsigned j = 0; j < 4u; j++)
#pragma unroll
            for (unsigned i = 0; i < 4u; i++) {
                const unsigned c = s_cnt[ly + j][lx + i];
                if (c != WT_AO_ABSENT && s_id[ly + j][lx + i] == id) { S += c; m++; }
            }
    } else {
        S = A.open[p]; m = 1u;
    }
    const unsigned vs = ref_ao_level(S, m, A.K, A.strength);
    A.out[p] = A.compose ? ref_ao_compose(A.frame[p], vs) : ref_ao_grey(vs);
}
