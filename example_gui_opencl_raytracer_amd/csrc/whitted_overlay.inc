/* whitted_overlay.inc -- the selection overlay (hip_wrap_ext.h: clw_overlay, clw_ext_render_overlay): outline, tint and object edges composed
 * from the traced frame and the id channel of the primary-hit pass.  Included by whitted_launch.inc behind whitted_gbuffer.inc, so it exists in
 * the fast and the strict unit; it uses nothing of either -- integers only, the same bits in both.  csrc/overlay_host.c is its definition.
 *
 * One work-item per output pixel of a width x rows range, a workgroup of 256 per tile of 32 x 8 pixels: a wavefront is two rows of 32 pixels,
 * lanes along x, so a wave's frame, id and output accesses are two runs of 128 contiguous bytes.
 * With OUTLINE or EDGES the ids of the tile and of a halo -- `radius` pixels all round for OUTLINE, one more column and row to the right and
 * below for EDGES alone: at most 40 x 16 words -- are staged in LDS, a staged row per wavefront per round (lanes 0 .. TW-1: one run of at most
 * 160 contiguous bytes).  An id is classified against the selection once, there: the selection travels in the kernel arguments, so the search
 * is a loop of scalar loads and one vector compare per listed id, and the ballot of a staged row's 40 verdicts IS the row's 64-bit mask.
 * The window test is separable on those masks: OR the 2 radius + 1 masks around a pixel's row (a column of the window per bit), then test the
 * 2 radius + 1 bits around its column -- at most 9 LDS reads per pixel, every one the same address in the 32 lanes of a row (a broadcast).
 * LDS banks: an id row is 40 words, but a 4-byte access conflicts only inside a half-wave, and a half-wave here reads or writes consecutive
 * words of ONE row -- 32 distinct banks -- so the row stride needs no padding.
 * A flag that is off is compiled out: no EDGES = no neighbour reads, no OUTLINE = no halo and no masks, FILL alone = no LDS at all (the pixel
 * classifies its own id). */

#define WT_OV_OUTLINE 1
#define WT_OV_FILL 2
#define WT_OV_EDGES 4
#define WT_OV_TILE_W 32
#define WT_OV_TILE_H 8
#define WT_OV_LDS_W (WT_OV_TILE_W + 8)       /* halo of at most 4 on both sides */
#define WT_OV_LDS_H (WT_OV_TILE_H + 8)

struct wt_overlay_args {
    const unsigned* frame;      /* width x rows packed pixels */
    const unsigned* ids;        /* width x rows ids */
    unsigned* out;
    unsigned width, rows;
    unsigned tiles_per_row;     /* ceil(width / 32) */
    unsigned radius;            /* 1..4 with OUTLINE */
    unsigned outline_rgb, fill_rgb, fill_alpha, edge_rgb;      /* colours already masked to 24 bits */
    unsigned count;             /* ids listed: 0..64 */
    unsigned sel[64];
};

/* wave-uniform loop over the kernel arguments: scalar loads, one v_cmp per listed id */
__device__ __forceinline__ bool wt_ov_selected(const wt_overlay_args& A, unsigned id) {
    bool hit = false;
    for (unsigned k = 0; k < A.count; k++) hit |= (id == A.sel[k]);
    return hit;
}

__device__ __forceinline__ unsigned wt_ov_blend(unsigned c, unsigned t, unsigned a) {
    unsigned out = 0u;
#pragma unroll
    for (int shift = 0; shift < 24; shift += 8) {
        const unsigned cc = (c >> shift) & 255u, tc = (t >> shift) & 255u;
        out |= ((cc * (256u - a) + tc * a + 128u) >> 8) << shift;
    }
    return out;
}

template <int FLAGS>
__global__ void __launch_bounds__(WT_OV_TILE_W * WT_OV_TILE_H) wt_overlay(const wt_overlay_args A) {
    constexpr bool OUTLINE = (FLAGS & WT_OV_OUTLINE) != 0, FILL = (FLAGS & WT_OV_FILL) != 0, EDGES = (FLAGS & WT_OV_EDGES) != 0;
    constexpr bool STAGED = OUTLINE || EDGES;
    __shared__ unsigned s_id[STAGED ? WT_OV_LDS_H : 1][STAGED ? WT_OV_LDS_W : 1];
    __shared__ unsigned long long s_mask[OUTLINE ? WT_OV_LDS_H : 1];

    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned lx = tid & (WT_OV_TILE_W - 1u), ly = tid / WT_OV_TILE_W;
    const unsigned x0 = (blockIdx.x % A.tiles_per_row) * WT_OV_TILE_W, y0 = (blockIdx.x / A.tiles_per_row) * WT_OV_TILE_H;
    const unsigned x = x0 + lx, y = y0 + ly;
    const bool valid = x < A.width && y < A.rows;
    const unsigned r = OUTLINE ? (A.radius < 4u ? A.radius : 4u) : 0u;      /* the halo to the left and above */

    if (STAGED) {
        const unsigned hi = (EDGES && r == 0u) ? 1u : r;                     /* ... and to the right and below */
        const unsigned tw = WT_OV_TILE_W + r + hi, th = WT_OV_TILE_H + r + hi;      /* <= 40 x 16 */
        for (unsigned ty = wave; ty < th; ty += 4u) {                        /* wave-uniform: every lane reaches the ballot */
            /* pixel (gx, gy) of the range; coordinates left of or above it wrap to huge values and fail the same compare */
            const unsigned gx = x0 + lane - r, gy = y0 + ty - r;
            const bool present = lane < tw && gx < A.width && gy < A.rows;
            const unsigned id = present ? A.ids[(size_t)gy * A.width + gx] : 0u;
            if (lane < tw) s_id[ty][lane] = id;
            if (OUTLINE) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(present && wt_ov_selected(A, id));
                if (lane == 0u) s_mask[ty] = m;
            }
        }
        __syncthreads();
    }
    if (!valid) return;

    const size_t p = (size_t)y * A.width + x;
    const unsigned tx = lx + r, ty = ly + r;
    unsigned c = A.frame[p] & 0x00FFFFFFu;
    const unsigned id = STAGED ? s_id[ty][tx] : (FILL ? A.ids[p] : 0u);
    if (EDGES) {
        /* an absent neighbour was staged as 0: the range tests decide, not its value */
        const bool dx = x + 1u < A.width && id != s_id[ty][tx + 1u];
        const bool dy = y + 1u < A.rows && id != s_id[ty + 1u][tx];
        if (dx || dy) c = A.edge_rgb;
    }
    bool sel = false;
    if (OUTLINE) sel = (s_mask[ty] >> tx) & 1ull;
    else if (FILL) sel = wt_ov_selected(A, id);
    if (FILL && sel) c = wt_ov_blend(c, A.fill_rgb, A.fill_alpha);
    if (OUTLINE) {
        unsigned long long m = 0ull;
        for (unsigned j = 0; j <= 2u * r; j++) m |= s_mask[ly + j];          /* rows y - r .. y + r: staged rows ly .. ly + 2 r <= 15 */
        const unsigned long long window = (2ull << (2u * r)) - 1ull;         /* 2 r + 1 bits: columns x - r .. x + r = staged columns lx .. */
        if (!sel && ((m >> lx) & window)) c = A.outline_rgb;
    }
    A.out[p] = c;
}
