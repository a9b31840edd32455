/* whitted_objects.inc -- the visible-object table (hip_wrap_ext.h: clw_object_stat, clw_ext_object_stats): per-id pixel count, bounding box,
 * depth range and coordinate sums of the pixels inside a rectangle, reduced from the id and depth channels of the primary-hit pass.  Included
 * by whitted_launch.inc behind whitted_overlay.inc, so it exists in the fast and the strict unit; it uses nothing of either -- integers only,
 * the same bits in both.  csrc/objects_host.c is its definition.
 *
 * The slot table in global memory is direct-indexed: the slot of an id is its index plus the counts of the kinds before it, CLW_ID_NONE
 * takes the last one -- no hashing, and slot order is id order.  A slot is 48 bytes whose all-zero state means "no pixel yet": minima are
 * kept as bitwise complements and folded with max, so ONE memset clears the table, and every fold is an integer atomic that returns
 * nothing -- the result cannot depend on arrival order.
 *
 * wt_objects_reduce: a workgroup of 256 takes one tile of 32 x 8 pixels of the CLIPPED rectangle at a time (no tile outside it is visited); a
 * wavefront is two rows of 32 pixels, lanes along x, so its id and depth reads are two runs of 128 contiguous bytes, each word read once.
 * A launch of more than WT_OBJ_MAX_GROUPS tiles gives every workgroup a run of consecutive tiles (row-major: neighbours along x), which it
 * walks with the next tile's words already on their way, keeping its LDS table across the run: the global atomics on a hot slot -- the floor,
 * the sky -- are serialised by the memory system at some 8 ns each (measured: 0.61 ms for the 8100 sets of a 1920 x 1080 frame with a workgroup
 * per tile), so their number, not the bytes read, is what the pass costs.  Aggregation is on chip, in two steps:
 *   1. across the lanes of a wave, a loop over the DISTINCT slots the wave shows: readlane picks the slot of the first lane not yet served,
 *      the ballot of "my slot is that one" is its pixel mask -- and because a lane's x and y are fixed by its number, count, bounding box and
 *      both coordinate sums fall out of that 64-bit mask in scalar arithmetic (popcounts, count-leading/trailing-zeros); only the two depth
 *      extremes take a butterfly over the lanes.  A sky or floor wave runs the loop once.
 *   2. across the four waves and the tiles of the run, lane 0 of each wave folds its per-slot aggregate into a keyed table of 256 entries in
 *      LDS (LDS atomics; the key is claimed by compare-and-swap, linear probing, at most 8 probes).  After the barrier one lane per occupied
 *      entry issues the entry's set of global atomics: a workgroup whose tiles show one id issues ONE set, one that sees k distinct ids k sets.
 *      Overflow fallback: a wave aggregate that finds no entry within its 8 probes (more than 256 ids in a run, or a crowded neighbourhood)
 *      goes to global memory directly -- still one set per (wave, tile, id), never one per pixel.
 *   The two summary counters (pixels inside the rectangle, pixels with an id that is not known) are wave ballots' popcounts, kept in scalar
 *   registers over the run and added in LDS, one global add each per workgroup.  An id is range-checked BEFORE it indexes anything.
 * wt_objects_compact: ONE workgroup of 1024 walks the slots in order, 1024 per round; ballot + popcount prefix the occupied slots inside a
 * wave, the 16 wave totals go through LDS, the offset is carried across rounds; occupied slots are decoded and written densely, in slot order.
 * The kernel boundary orders it behind the reduce: no fence protocol. */

#define WT_OBJ_TILE_W 32
#define WT_OBJ_TILE_H 8
#define WT_OBJ_TABLE 256u       /* LDS entries per workgroup (a power of two: 2^WT_OBJ_TABLE_LG) */
#define WT_OBJ_TABLE_LG 8
#define WT_OBJ_MAX_GROUPS 512u  /* workgroups of a launch: two per compute unit */
#define WT_OBJ_PROBES 8u
#define WT_OBJ_CHUNK 1024
#define WT_OBJ_NONE 0xFFFFFFFFu /* CLW_ID_NONE */

struct wt_obj_slot {            /* 48 bytes; all-zero = empty */
    unsigned pixels;
    unsigned nx0, ny0;          /* ~x0, ~y0: folded with max */
    unsigned x1, y1;
    unsigned ndmin, dmax;       /* ~(smallest depth bits), largest depth bits */
    unsigned pad;
    unsigned long long sum_x, sum_y;
};
struct wt_obj_head { unsigned foreign, pixels, pad[2]; };      /* 16 bytes in front of the slots, cleared with them */
struct wt_obj_record {          /* clw_object_stat */
    unsigned id, pixels, x0, y0, x1, y1, dmin, dmax;
    unsigned long long sum_x, sum_y;
};
static_assert(sizeof(wt_obj_slot) == 48 && sizeof(wt_obj_record) == 48 && sizeof(wt_obj_head) == 16, "the table's layouts");

struct wt_objects_args {
    const unsigned* ids;        /* width x rows ids */
    const unsigned* depth;      /* width x rows depth bit patterns, or null */
    wt_obj_head* head;
    wt_obj_slot* slots;         /* c0 + c1 + c2 + 1 of them */
    unsigned width, first_row;
    unsigned cx, cy, cw, ch;    /* the clipped rectangle: first column, first row OF THE RANGE, columns, rows */
    unsigned tiles_per_row;     /* ceil(cw / 32) */
    unsigned tiles;             /* tiles_per_row * ceil(ch / 8) */
    unsigned tiles_per_group;   /* consecutive tiles a workgroup walks: ceil(tiles / workgroups) */
    unsigned c0, c1, c2;        /* spheres, planes, lights */
};

/* the sum of the positions of the set bits of a 32-bit mask */
__device__ __forceinline__ unsigned wt_obj_bit_positions(unsigned m) {
    return __builtin_popcount(m & 0xAAAAAAAAu) + 2u * __builtin_popcount(m & 0xCCCCCCCCu) + 4u * __builtin_popcount(m & 0xF0F0F0F0u) +
           8u * __builtin_popcount(m & 0xFF00FF00u) + 16u * __builtin_popcount(m & 0xFFFF0000u);
}

/* one set of global atomics on a slot; nothing is returned */
__device__ __forceinline__ void wt_obj_fold_global(wt_obj_slot* g, bool has_depth, unsigned pixels, unsigned nx0, unsigned ny0, unsigned x1, unsigned y1,
                                                   unsigned ndmin, unsigned dmax, unsigned long long sx, unsigned long long sy) {
    atomicAdd(&g->pixels, pixels);
    atomicMax(&g->nx0, nx0); atomicMax(&g->ny0, ny0); atomicMax(&g->x1, x1); atomicMax(&g->y1, y1);
    if (has_depth) { atomicMax(&g->ndmin, ndmin); atomicMax(&g->dmax, dmax); }
    atomicAdd(&g->sum_x, sx); atomicAdd(&g->sum_y, sy);
}

/* this lane's id and depth words of tile t (row-major tiles of the clipped rectangle) -> whether the lane lies inside the rectangle there */
__device__ __forceinline__ bool wt_obj_fetch(const wt_objects_args& A, unsigned t, unsigned wave, unsigned lane, bool has_depth, unsigned& id, unsigned& d) {
    const unsigned rx = (t % A.tiles_per_row) * WT_OBJ_TILE_W + (lane & 31u), ry = (t / A.tiles_per_row) * WT_OBJ_TILE_H + wave * 2u + (lane >> 5);
    const bool valid = rx < A.cw && ry < A.ch;
    const size_t p = (size_t)(A.cy + ry) * A.width + (A.cx + rx);
    id = valid ? A.ids[p] : 0u;
    d = (valid && has_depth) ? A.depth[p] : 0u;
    return valid;
}

__global__ void __launch_bounds__(WT_OBJ_TILE_W * WT_OBJ_TILE_H) wt_objects_reduce(const wt_objects_args A) {
    __shared__ unsigned s_key[WT_OBJ_TABLE];                /* slot + 1; 0 = free */
    __shared__ unsigned s_pix[WT_OBJ_TABLE], s_nx0[WT_OBJ_TABLE], s_ny0[WT_OBJ_TABLE], s_x1[WT_OBJ_TABLE], s_y1[WT_OBJ_TABLE];
    __shared__ unsigned s_ndmin[WT_OBJ_TABLE], s_dmax[WT_OBJ_TABLE];
    __shared__ unsigned long long s_sx[WT_OBJ_TABLE], s_sy[WT_OBJ_TABLE];
    __shared__ unsigned s_cnt[2];                           /* foreign, pixels */

    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool has_depth = A.depth != nullptr;
    static_assert(WT_OBJ_TABLE == WT_OBJ_TILE_W * WT_OBJ_TILE_H, "an LDS entry per thread");
    {
        s_key[tid] = 0u; s_pix[tid] = 0u; s_nx0[tid] = 0u; s_ny0[tid] = 0u; s_x1[tid] = 0u; s_y1[tid] = 0u; s_ndmin[tid] = 0u; s_dmax[tid] = 0u;
        s_sx[tid] = 0ull; s_sy[tid] = 0ull;
    }
    if (tid < 2u) s_cnt[tid] = 0u;
    __syncthreads();

    const unsigned t_first = blockIdx.x * A.tiles_per_group;
    if (t_first >= A.tiles) return;                         /* (workgroup-uniform; the launcher's grid has no such workgroup) */
    const unsigned t_end = A.tiles - t_first < A.tiles_per_group ? A.tiles : t_first + A.tiles_per_group;
    unsigned n_foreign = 0u, n_valid = 0u;                  /* of this wave, over the run */

    /* the first tile's words; inside the loop, the next tile's are asked for before this tile's are used */
    unsigned id_next = 0u, d_next = 0u;
    bool valid_next = wt_obj_fetch(A, t_first, wave, lane, has_depth, id_next, d_next);
    for (unsigned t = t_first; t < t_end; t++) {            /* workgroup-uniform */
        const unsigned id = id_next, d = d_next;
        const bool valid = valid_next;
        if (t + 1u < t_end) valid_next = wt_obj_fetch(A, t + 1u, wave, lane, has_depth, id_next, d_next);

        /* the slot, range-checked: an id that is not known indexes nothing */
        const unsigned kind = id >> 30, index = id & 0x3FFFFFFFu;
        bool known = false;
        unsigned slot = 0u;
        if (id == WT_OBJ_NONE) { known = true; slot = A.c0 + A.c1 + A.c2; }
        else if (kind == 0u && index < A.c0) { known = true; slot = index; }
        else if (kind == 1u && index < A.c1) { known = true; slot = A.c0 + index; }
        else if (kind == 2u && index < A.c2) { known = true; slot = A.c0 + A.c1 + index; }
        const bool mine = valid && known;

        n_valid += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
        n_foreign += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid && !known));
        unsigned long long todo = __builtin_amdgcn_ballot_w64(mine);
        /* frame coordinates of the wave's lane 0 in this tile */
        const unsigned wx0 = A.cx + (t % A.tiles_per_row) * WT_OBJ_TILE_W, wy0 = A.first_row + A.cy + (t / A.tiles_per_row) * WT_OBJ_TILE_H + wave * 2u;

        while (todo) {      /* wave-uniform: one round per distinct slot of the wave */
            const unsigned s = __builtin_amdgcn_readlane(slot, (int)__builtin_ctzll(todo));
            const bool match = mine && slot == s;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(match);
            todo &= ~m;
            const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32), cols = lo | hi;      /* the wave's first and second row; cols != 0 */
            const unsigned n = __builtin_popcountll(m), n_hi = __builtin_popcount(hi);
            const unsigned x0 = wx0 + (unsigned)__builtin_ctz(cols), x1 = wx0 + 31u - (unsigned)__builtin_clz(cols);
            const unsigned y0 = wy0 + (lo ? 0u : 1u), y1 = wy0 + (hi ? 1u : 0u);
            const unsigned long long sx = (unsigned long long)wx0 * n + wt_obj_bit_positions(lo) + wt_obj_bit_positions(hi);
            const unsigned long long sy = (unsigned long long)wy0 * n + n_hi;
            unsigned dmin = match ? d : 0xFFFFFFFFu, dmax = match ? d : 0u;
            if (has_depth) {
#pragma unroll
                for (int k = 1; k < 64; k <<= 1) {
                    const unsigned a = (unsigned)__shfl_xor((int)dmin, k, 64), b = (unsigned)__shfl_xor((int)dmax, k, 64);
                    dmin = a < dmin ? a : dmin; dmax = b > dmax ? b : dmax;
                }
            }
            if (lane == 0u) {
                const unsigned h = (s * 0x9E3779B1u) >> (32 - WT_OBJ_TABLE_LG);
                bool placed = false;
                for (unsigned k = 0; k < WT_OBJ_PROBES && !placed; k++) {
                    const unsigned e = (h + k) & (WT_OBJ_TABLE - 1u);
                    const unsigned old = atomicCAS(&s_key[e], 0u, s + 1u);
                    if (old == 0u || old == s + 1u) {
                        atomicAdd(&s_pix[e], n);
                        atomicMax(&s_nx0[e], ~x0); atomicMax(&s_ny0[e], ~y0); atomicMax(&s_x1[e], x1); atomicMax(&s_y1[e], y1);
                        if (has_depth) { atomicMax(&s_ndmin[e], ~dmin); atomicMax(&s_dmax[e], dmax); }
                        atomicAdd(&s_sx[e], sx); atomicAdd(&s_sy[e], sy);
                        placed = true;
                    }
                }
                if (!placed) wt_obj_fold_global(&A.slots[s], has_depth, n, ~x0, ~y0, x1, y1, ~dmin, dmax, sx, sy);      /* the overflow fallback */
            }
        }
    }
    if (lane == 0u) {
        if (n_foreign) atomicAdd(&s_cnt[0], n_foreign);
        if (n_valid) atomicAdd(&s_cnt[1], n_valid);
    }
    __syncthreads();

    {      /* WT_OBJ_TABLE == the workgroup's size: an entry per thread */
        const unsigned key = s_key[tid];
        if (key) wt_obj_fold_global(&A.slots[key - 1u], has_depth, s_pix[tid], s_nx0[tid], s_ny0[tid], s_x1[tid], s_y1[tid], s_ndmin[tid], s_dmax[tid],
                                    s_sx[tid], s_sy[tid]);
    }
    if (tid == 0u) {
        if (s_cnt[0]) atomicAdd(&A.head->foreign, s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&A.head->pixels, s_cnt[1]);
    }
}

__global__ void __launch_bounds__(WT_OBJ_CHUNK) wt_objects_compact(const wt_obj_head* head, const wt_obj_slot* slots, unsigned nslots, unsigned c0,
                                                                   unsigned c1, unsigned c2, unsigned has_depth, unsigned* summary,
                                                                   wt_obj_record* out) {
    __shared__ unsigned s_wave[WT_OBJ_CHUNK / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned carry = 0u;                                   /* records written by the rounds before this one */
    for (unsigned base = 0; base < nslots; base += WT_OBJ_CHUNK) {      /* workgroup-uniform: every thread reaches both barriers */
        const unsigned k = base + tid;
        const bool live = k < nslots && slots[k].pixels != 0u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
        if (lane == 0u) s_wave[wave] = (unsigned)__builtin_popcountll(m);
        __syncthreads();
        unsigned before = 0u, total = 0u;
        for (unsigned w = 0; w < WT_OBJ_CHUNK / 64; w++) {
            const unsigned c = s_wave[w];
            total += c;
            if (w < wave) before += c;
        }
        if (live) {
            const wt_obj_slot s = slots[k];
            wt_obj_record r;
            r.id = k < c0 ? k : k < c0 + c1 ? (1u << 30) | (k - c0) : k < c0 + c1 + c2 ? (2u << 30) | (k - c0 - c1) : WT_OBJ_NONE;
            r.pixels = s.pixels;
            r.x0 = ~s.nx0; r.y0 = ~s.ny0; r.x1 = s.x1; r.y1 = s.y1;
            r.dmin = has_depth ? ~s.ndmin : 0u; r.dmax = has_depth ? s.dmax : 0u;
            r.sum_x = s.sum_x; r.sum_y = s.sum_y;
            out[carry + before + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = r;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0u) { summary[0] = carry; summary[1] = head->pixels; summary[2] = head->foreign; summary[3] = 0u; }
}
