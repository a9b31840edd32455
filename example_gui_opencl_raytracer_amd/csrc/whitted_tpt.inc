/* whitted_tpt.inc -- the tree-parallel tail of a deep launch (textually included once by wt_trace_body, wave-uniform context).
 *
 * Why.  In the reference's loop (raytracing.cl:40-190) a pixel is ONE serial chain: hit, shade, push the reflected continuation, follow the
 * refracted child, pop.  At depth 15 a pixel inside stacked glass walks a tree of a hundred and more segments, and a launch waits for
 * the few tiles that hold such pixels (800x600 depth 15: 0.57 ms, of which 0.56 are one tile's chain).  But only two things in that
 * loop are truly sequential per pixel, and neither is geometry:
 *   - the xorshift stream (raytracing.cl:33,99-100) feeds the shadow samples ONLY: exactly 4 * light_num numbers per shaded hit, whether
 *     or not a ray is traced -- so the state at the k-th shaded hit in depth-first order is xorshift^(4 nl k)(state at entry);
 *   - the order of the float additions into a path's radiance (ambient, then per light, then the refracted child's sum, :83-136,183-190).
 * Every decision that SHAPES the tree (nearest hit, Schlick, push or total internal reflection, :139-179) needs neither.
 *
 * What.  Once at most P.tpt_max lanes of the tile are alive, everything they still owe -- the segment each is about to trace and the
 * reflected continuations waiting on its DFS stack -- becomes a forest of NODES in the tile's slice of P.tpt_pool (HBM / L2; a node is a
 * path segment), and the whole wave works on it, 64 nodes at a time, whichever pixel they belong to:
 *   A  expansion   every lane takes an untraced node, runs the same hit phase (whitted_hit.inc) and the same Fresnel / refraction step
 *                  (whitted_bounce.inc) as the per-lane loop and appends the children: reflected continuation, refracted child.  What the
 *                  segment would have ADDED to its path is recorded in the node instead (colour of a light / the skybox, ambient term).
 *   B  order       subtree sizes bottom-up, depth-first positions top-down (refracted subtree before reflected continuation, as the
 *                  reference's stack discipline visits them), batch by batch: children always lie in a later batch than their parent;
 *   C  RNG         one lane per PIXEL walks its nodes in depth-first order and leaves the xorshift state each shaded hit starts from;
 *   D  shading     every lane takes a shaded hit -- any pixel, any order -- and runs the same six-ray batch (whitted_shade.inc);
 *                  the lights' factors are stored per node;
 *   E  replay      one lane per pixel adds everything up in the reference's order: per node the recorded terms, a saved sum per open
 *                  refraction level (raytracing.cl:183-190: parent + child).
 * A/D run at full lane occupancy whatever the shape of the trees; the serial parts left (C, E) cost a few dozen instructions per node.
 * Same arithmetic per ray and the same additions in the same order: the strict build stays bit-identical to the oracle, the fast build
 * to its own per-lane loop (tests/test_gpu_parity.py runs whole frames with tpt_max = 64, i.e. EVERYTHING through the tail).
 *
 * Memory.  Nodes live in blocks of 64, field-major inside a block (a batch reads and writes 256 contiguous bytes per field), in a SLOT of
 * P.tpt_pool that the wave holds while it is in here.  Slots are handed out per XCD -- P.tpt_slots of them for each value of the
 * hardware's XCC_ID, more than an XCD's CUs can hold wavefronts -- by a compare-and-swap on a flag word, tried first at the index the
 * wave's own place in the machine hashes to (HW_ID: SE, SH, CU, SIMD, wave slot), so two resident waves rarely even probe the same word.
 * Per XCD because a slot is recycled WITHIN the launch: its next owner must run behind the same L2 (the L2s of different XCDs are not
 * coherent with each other); and a wave only ever loads words it has stored itself since it took the slot, so what an earlier owner left
 * in this CU's L1 is never read.  If the trees outgrow the slot (or the batch list its LDS table, or no slot is free) the tail gives up
 * BEFORE it has changed any lane state -- the lanes' registers are parked in the slot on entry -- and the per-lane loop finishes the tile.
 *
 * In scope: P, sg, lane, tid, wg, D, the lane state (o, d, rgb, depth, n1, f, sp, rng, active), s_stk / deep (the DFS stack), the counters. */
{
    enum { TK_UNTRACED = 0, TK_COLOUR = 2, TK_HIT = 3, TK_VIRTUAL = 4 };
    /* node fields (words); after a node is traced O/D/N1 hold the hit's ip / normal / shininess */
    enum { T_O = 0, T_D = 3, T_N1 = 6, T_F = 7, T_META = 8, T_KIDS = 9, T_V = 10, T_KS = 13, T_KD = 14, T_A = 15, T_AMB = 18,
           T_POS = 19,     /* nodes | shaded hits << 16: of the subtree first, then before the node in depth-first order */
           T_RS = 20,      /* by hit ordinal (depth-first, wave-wide): the xorshift state the hit starts from */
           T_ORDER = 21,   /* by POSITION: node | kind << 16 | level << 19 | has refracted child << 25 | has continuation << 26 */
           T_HITS = 22,    /* by order of discovery: the shaded hits' nodes */
           T_PA = 23,      /* by position: the node's recorded term (T_A) ... */
           T_PS = 26,      /* ... and its scalar: the ambient coefficient of a hit, the throughput of a colour node */
           T_PK = 27,      /* strict only, by position: ks, kd of a hit */
           T_W = WT_STRICT ? 29 : 27 };   /* by position, per light: fast 1 word (its weight), strict 4 (soft, dl, spec, diff) */
    /* META: kind (bits 0-2) | depth (3-8) | pixel lane (9-14) | refraction level = parents on the reference's stack (15-20) */
    constexpr unsigned T_NONE = 0xFFFFu;
    constexpr unsigned T_LW = WT_STRICT ? 4u : 1u;
    /* field `fld` of node (or position, or hit ordinal) i: blocks of 64 nodes, field-major inside a block -- a batch reads and writes 256
     * contiguous bytes per field, and everything about 64 nodes lies within T_NF x 256 contiguous bytes (with whole arrays per field,
     * 40 KB apart in a 1 MB slot, a batch touched forty pages: the expansion pass spent most of its time in address translation) */
    const unsigned T_CAP = P.tpt_cap;
    const unsigned T_NF = T_W + T_LW * P.nl;
#define TN(i) (TS + (size_t)(((i) >> 6) * (T_NF * 64u) + ((i) & 63u)))          /* node i's word of field 0; field f is 64 f words on: ONE 64-bit address per node, */
#define TB(nb, fld) (nb)[(fld) * 64u]                                               /* the fields are immediate offsets (per access the compiler kept an address pair each: 250 VGPRs) */
#define TF(fld, i) TB(TN(i), fld)
    const unsigned long long t_lt = (1ull << lane) - 1ull;
    const bool t_alive = active;

    /* is there enough left to pay the tail's fixed costs?  pending paths = the current segment + the continuations on the stack */
    unsigned t_pend = t_alive ? (unsigned)sp + 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) t_pend += (unsigned)__shfl_xor((int)t_pend, off);
    bool t_abort = t_pend < (part_lg != 0u ? 1u : P.tpt_min);

    /* ---- a slot of the pool ------------------------------------------------------------------------------------------------------- */
    const unsigned t_xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u;             /* HW_REG_XCC_ID[3:0] */
    unsigned t_slot = 0xFFFFFFFFu;
    if (!t_abort) {
        if (lane == 0) {
            const unsigned hw = __builtin_amdgcn_s_getreg(4 | (15 << 11));             /* HW_REG_HW_ID[15:0]: wave, SIMD, pipe, CU, SH, SE */
            const unsigned h0 = (hw & 0x3Fu) | (((hw >> 8) & 0xFFu) << 6);
            for (unsigned probe = 0; probe < 256u; probe++) {
                const unsigned sl = (h0 + probe) % P.tpt_slots;
                if (atomicCAS(P.tpt_flags + t_xcc * P.tpt_slots + sl, 0u, 1u) == 0u) { t_slot = sl; break; }
            }
        }
        t_slot = (unsigned)__builtin_amdgcn_readfirstlane((int)t_slot);
        if (t_slot == 0xFFFFFFFFu) t_abort = true;
    }

    /* DIAGNOSTIC (P.tpt_clock): where the time goes, in ticks of 10 ns summed over the tiles (counter words 10-15: roots, expansion, order, RNG,
     * shading, replay; 16-19: batches, most batches, most nodes, longest stay; 20-25: the longest of each phase) */
    const bool t_clock = P.tpt_clock != 0u;           /* (wave-uniform; any build: clw_ext_set_tpt_clock) */
    unsigned long long t_clk = t_clock ? __builtin_amdgcn_s_memrealtime() : 0ull;
    unsigned t_ph[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#define T_PHASE(k) do { if (t_clock) { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); t_ph[k] += (unsigned)(n_ - t_clk); t_clk = n_; } } while (0)
    if (!t_abort) {
    unsigned* const TS = P.tpt_pool + (size_t)(t_xcc * P.tpt_slots + t_slot) * P.tpt_slice_words;
    unsigned* const T_SAVE = TS + (size_t)T_NF * ((T_CAP + 63u) & ~63u);    /* parked lane state: [word][lane], 25 words */
    unsigned* const T_RSTK = T_SAVE + (25u + 3u * WT_REC) * 64u;           /* replay: saved sums, [level][3][lane] (behind the parked registers and LDS stack levels) */
    /* ---- park the lane state ------------------------------------------------------------------------------------------------ */
    {
        const unsigned sv[14] = {__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(d.x), __float_as_uint(d.y),
                                 __float_as_uint(d.z), __float_as_uint(rgb.x), __float_as_uint(rgb.y), __float_as_uint(rgb.z), (unsigned)depth,
                                 __float_as_uint(n1), __float_as_uint(f), (unsigned)sp, rng};
#pragma unroll
        for (int w = 0; w < 14; w++) T_SAVE[w * 64 + lane] = sv[w];
        if (COUNT) {
            const unsigned cv[11] = {c_seg, c_shadow, c_probe, c_sky, c_tex, c_push, c_iter, c_witer, c_traced, c_known, c_visbad};
#pragma unroll
            for (int w = 0; w < 11; w++) T_SAVE[(14 + w) * 64 + lane] = cv[w];
        }
    }
    /* the LDS levels of the DFS stack are parked too: once the roots are out, the expansion uses that LDS as its forwarding window */
    for (int w = 0; w < LDSL * WT_REC; w++) T_SAVE[(25 + w) * 64 + lane] = __float_as_uint(s_stk[w * WT_BLOCK + tid]);
    const unsigned t_rng0 = rng;
    auto t_load_rec = [&](int k, float (&rec)[WT_REC]) {
        if (SCRL == 0 || k < LDSL) {
#pragma unroll
            for (int w = 0; w < WT_REC; w++) rec[w] = s_stk[(k * WT_REC + w) * WT_BLOCK + tid];
        } else {
#pragma unroll
            for (int w = 0; w < WT_REC; w++) rec[w] = deep[(k - LDSL) * WT_REC + w];
        }
    };

    /* ---- roots: the lane's stack and its current segment as a chain of nodes ---------------------------------------------------
     * Record k of the stack (raytracing.cl:171-176: the reflected continuation of a hit, with the radiance its path had gathered) is the
     * parent of everything above it, so the forest of a pixel is ONE tree:
     *   V_k  (virtual: "the path's sum is rec_k.rgb here")  refracted child: V_k+1 ... or W;  continuation: C_k = rec_k's ray, if its depth allows
     *   W    (virtual: "the path's sum is the lane's rgb")  continuation: R = the segment the lane was about to trace.
     * The virtual nodes come first, one batch per stack level (a child always lies in a later batch than its parent); behind them ALL the
     * segments to trace -- every lane's R, then the C_k -- as one run of nodes that the expansion cuts into batches of 64. */
    unsigned t_count = 0u, t_nb = 0u, t_nh = 0u;     /* nodes, batches, shaded hits (wave-uniform) */
    if (lane == 0) s_tpt_bs[0] = 0;
    const int t_nsp = t_alive ? sp : -1;
    int t_maxsp = t_nsp;
    for (int off = 32; off > 0; off >>= 1) t_maxsp = max(t_maxsp, __shfl_xor(t_maxsp, off));
    unsigned t_root = T_NONE, t_wid = T_NONE;
    for (int j = 0; j <= t_maxsp; j++) {             /* level j: V_j of the lanes with deeper stacks, W of those whose stack ends here */
        const bool has = t_nsp >= j;
        const unsigned long long mj = __builtin_amdgcn_ballot_w64(has);
        const unsigned cj = (unsigned)__builtin_popcountll(mj);
        if (t_count + cj > T_CAP || t_nb + 1u > WT_TPT_MAX_BATCHES) { t_abort = true; break; }
        if (has) {
            const unsigned id = t_count + (unsigned)__builtin_popcountll(mj & t_lt);
            f3 init = rgb;
            if (t_nsp > j) {                         /* rec_j.rgb */
                if (SCRL == 0 || j < LDSL) init = mk3(s_stk[(j * WT_REC + 6) * WT_BLOCK + tid], s_stk[(j * WT_REC + 7) * WT_BLOCK + tid], s_stk[(j * WT_REC + 8) * WT_BLOCK + tid]);
                else init = mk3(deep[(j - LDSL) * WT_REC + 6], deep[(j - LDSL) * WT_REC + 7], deep[(j - LDSL) * WT_REC + 8]);
            } else t_wid = id;
            unsigned* const nb = TN(id);
            TB(nb, T_META) = TK_VIRTUAL | (lane << 9) | ((unsigned)j << 15);
            TB(nb, T_A + 0) = __float_as_uint(init.x); TB(nb, T_A + 1) = __float_as_uint(init.y); TB(nb, T_A + 2) = __float_as_uint(init.z);
            if (j == 0) t_root = id;
        }
        t_count += cj; t_nb++;
        if (lane == 0) s_tpt_bs[t_nb] = (unsigned short)t_count;
    }
    const unsigned t_nvb = t_nb;                     /* the expansion starts behind the virtual batches */
    unsigned t_closed = t_count;                     /* = s_tpt_bs[t_nb]: the nodes from here on are not in a batch yet */
    __syncthreads();                                 /* (lane 0's table) */
    if (!t_abort) {                                  /* R of every lane */
        const unsigned long long mr = __builtin_amdgcn_ballot_w64(t_alive);
        const unsigned cr = (unsigned)__builtin_popcountll(mr);
        if (t_count + cr > T_CAP) t_abort = true;
        else if (t_alive) {
            const unsigned id = t_count + (unsigned)__builtin_popcountll(mr & t_lt);
            unsigned* const nb = TN(id);
            TB(nb, T_META) = TK_UNTRACED | ((unsigned)depth << 3) | (lane << 9) | ((unsigned)t_nsp << 15);
            TB(nb, T_O + 0) = __float_as_uint(o.x); TB(nb, T_O + 1) = __float_as_uint(o.y); TB(nb, T_O + 2) = __float_as_uint(o.z);
            TB(nb, T_D + 0) = __float_as_uint(d.x); TB(nb, T_D + 1) = __float_as_uint(d.y); TB(nb, T_D + 2) = __float_as_uint(d.z);
            TB(nb, T_N1) = __float_as_uint(n1); TB(nb, T_F) = __float_as_uint(f);
            TF(T_KIDS, t_wid) = T_NONE | (id << 16);
        }
        t_count += cr;
    }
    for (int k = 0; k < t_maxsp && !t_abort; k++) {  /* C_k, and what V_k's children are */
        const bool hasv = t_nsp > k;
        float rc[WT_REC];
        bool hasc = false;
        if (hasv) { t_load_rec(k, rc); hasc = __float_as_int(rc[9]) < D; }
        const unsigned long long mc = __builtin_amdgcn_ballot_w64(hasc);
        const unsigned cc = (unsigned)__builtin_popcountll(mc);
        if (t_count + cc > T_CAP) { t_abort = true; break; }
        /* this lane's nodes of levels k and k + 1: level j's batch starts at s_tpt_bs[j] and holds the lanes with nsp >= j in lane order */
        const unsigned vk = s_tpt_bs[k] + (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(t_nsp >= k) & t_lt);
        const unsigned vk1 = s_tpt_bs[k + 1] + (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(t_nsp >= k + 1) & t_lt);
        const unsigned idc = t_count + (unsigned)__builtin_popcountll(mc & t_lt);
        if (hasc) {
            unsigned* const nb = TN(idc);
            TB(nb, T_META) = TK_UNTRACED | ((unsigned)__float_as_int(rc[9]) << 3) | (lane << 9) | ((unsigned)k << 15);
#pragma unroll
            for (int w = 0; w < 6; w++) TB(nb, T_O + w) = __float_as_uint(rc[w]);
            TB(nb, T_N1) = __float_as_uint(rc[10]); TB(nb, T_F) = __float_as_uint(rc[11]);
        }
        if (hasv) TF(T_KIDS, vk) = vk1 | ((hasc ? idc : T_NONE) << 16);
        t_count += cc;
    }

    T_PHASE(0);
    /* ---- A: expansion ------------------------------------------------------------------------------------------------------------ */
#undef WT_HIT_COLOUR
#undef WT_HIT_AMBIENT
#undef WT_BOUNCE_PUSH
#undef WT_BOUNCE_LAST
#define WT_BOUNCE_LAST false            /* the tail runs the whole bounce on every node, as before */
#undef WT_MOTION
#define WT_MOTION (wt_motion{false, 0.0f, 0u})   /* moving launches never enter the tail (the shim sets tpt_cap = 0): a node is traced by whichever lane takes it */
#define WT_HIT_COLOUR(c) t_col = (c)
#define WT_HIT_AMBIENT(cf, a) do { t_col = (cf); t_ambk = (a); } while (0)
#define WT_BOUNCE_PUSH(rec) do { t_pushed = true; _Pragma("unroll") for (int w_ = 0; w_ < WT_REC; w_++) t_prec[w_] = (rec)[w_]; } while (0)
    /* A segment's children are stored as nodes (global memory) AND, the first 64 of a batch's, handed on through LDS (the parked DFS
     * stack's): a batch made only of the children of the batch before it -- every batch of a chain of reflections -- starts from LDS
     * and waits for no store.  Word w of window entry i: s_stk[w * 64 + i]. */
    unsigned t_s0 = t_closed, t_fw = 0xFFFFFFFFu;    /* first node not in a batch yet; first node of the window */
    while (t_s0 < t_count && !t_abort) {
        if (t_nb == WT_TPT_MAX_BATCHES) { t_abort = true; break; }
        const unsigned s0 = t_s0, e0 = min(t_s0 + 64u, t_count);
        t_nb++;
        if (lane == 0) s_tpt_bs[t_nb] = (unsigned short)e0;
        t_s0 = e0;
        const bool from_lds = WT_TPT_FORWARD && t_fw != 0xFFFFFFFFu && s0 >= t_fw && e0 - t_fw <= 64u;
        if (!from_lds) __syncthreads();              /* the nodes earlier batches stored */
        const unsigned node = s0 + lane;
        const bool tr = node < e0;                   /* (every node behind the virtual batches is a segment to trace) */
        unsigned meta = 0u;
        bool ended = false, shade = false, t_pushed = false;
        f3 ip = mk3(0, 0, 0), nrm = mk3(0, 0, 1), view = mk3(0, 0, 1), t_col = mk3(0, 0, 0);
        mat_t m;
        m.rgb = mk3(0, 0, 0); m.ambient = m.diffuse = m.specular = m.shininess = 0.0f;
        m.transparent = m.dielectric = 0u; m.n = 1.0f; m.reflectivity = 0.0f;
        float ks = 0.0f, kd = 0.0f, t_ambk = 0.0f;
        float t_prec[WT_REC];
        unsigned prim = 0u, texpx = 0u;
        bool textured = false;
        if (tr) {
            if (from_lds) {
                const unsigned i_ = node - t_fw;
                o = mk3(s_stk[0 * 64 + i_], s_stk[1 * 64 + i_], s_stk[2 * 64 + i_]);
                d = mk3(s_stk[3 * 64 + i_], s_stk[4 * 64 + i_], s_stk[5 * 64 + i_]);
                n1 = s_stk[6 * 64 + i_]; f = s_stk[7 * 64 + i_]; meta = __float_as_uint(s_stk[8 * 64 + i_]);
            } else {
                const unsigned* const nb = TN(node);
                meta = TB(nb, T_META);
                o = mk3(__uint_as_float(TB(nb, T_O + 0)), __uint_as_float(TB(nb, T_O + 1)), __uint_as_float(TB(nb, T_O + 2)));
                d = mk3(__uint_as_float(TB(nb, T_D + 0)), __uint_as_float(TB(nb, T_D + 1)), __uint_as_float(TB(nb, T_D + 2)));
                n1 = __uint_as_float(TB(nb, T_N1)); f = __uint_as_float(TB(nb, T_F));
            }
            depth = (int)((meta >> 3) & 63u); sp = (int)((meta >> 15) & 63u);
#include "whitted_hit.inc"
            if (shade) {
#include "whitted_bounce.inc"
            }
        }
        (void)prim; (void)ended;
        /* children: after the bounce (o, d, n1, f, depth) is the segment the per-lane loop would follow next -- the refracted child if the
         * continuation was pushed (then t_prec holds the continuation), else the continuation itself, which exists while depth < D */
        const bool k_refr = shade && t_pushed;
        const bool k_refl = shade && (t_pushed || depth < D);
        const unsigned long long mt = __builtin_amdgcn_ballot_w64(k_refr), mr = __builtin_amdgcn_ballot_w64(k_refl),
                                 mh = __builtin_amdgcn_ballot_w64(shade);
        const unsigned ct = (unsigned)__builtin_popcountll(mt), cr = (unsigned)__builtin_popcountll(mr);
        if (t_count + ct + cr > T_CAP) { t_abort = true; break; }
        const unsigned idt = t_count + (unsigned)__builtin_popcountll(mt & t_lt);
        const unsigned idr = t_count + ct + (unsigned)__builtin_popcountll(mr & t_lt);
        const unsigned pix = meta & (63u << 9), lvl = (meta >> 15) & 63u;
        auto t_child = [&](unsigned id, f3 co_, f3 cd_, float cn1, float cf, unsigned cmeta) {
            unsigned* const cb = TN(id);
            TB(cb, T_META) = cmeta;
            TB(cb, T_O + 0) = __float_as_uint(co_.x); TB(cb, T_O + 1) = __float_as_uint(co_.y); TB(cb, T_O + 2) = __float_as_uint(co_.z);
            TB(cb, T_D + 0) = __float_as_uint(cd_.x); TB(cb, T_D + 1) = __float_as_uint(cd_.y); TB(cb, T_D + 2) = __float_as_uint(cd_.z);
            TB(cb, T_N1) = __float_as_uint(cn1); TB(cb, T_F) = __float_as_uint(cf);
            const unsigned i_ = id - t_count;        /* (t_count: still the first child of this batch) */
            if (WT_TPT_FORWARD && i_ < 64u) {
                s_stk[0 * 64 + i_] = co_.x; s_stk[1 * 64 + i_] = co_.y; s_stk[2 * 64 + i_] = co_.z;
                s_stk[3 * 64 + i_] = cd_.x; s_stk[4 * 64 + i_] = cd_.y; s_stk[5 * 64 + i_] = cd_.z;
                s_stk[6 * 64 + i_] = cn1; s_stk[7 * 64 + i_] = cf; s_stk[8 * 64 + i_] = __uint_as_float(cmeta);
            }
        };
        if (k_refr) t_child(idt, o, d, n1, f, TK_UNTRACED | ((unsigned)depth << 3) | pix | ((lvl + 1u) << 15));
        if (k_refl) {
            if (t_pushed) t_child(idr, mk3(t_prec[0], t_prec[1], t_prec[2]), mk3(t_prec[3], t_prec[4], t_prec[5]), t_prec[10], t_prec[11],
                                  TK_UNTRACED | ((unsigned)__float_as_int(t_prec[9]) << 3) | pix | (lvl << 15));
            else t_child(idr, o, d, n1, f, TK_UNTRACED | ((unsigned)depth << 3) | pix | (lvl << 15));
        }
        t_fw = t_count;
        if (tr) {                                    /* what this segment found */
            unsigned* const ob = TN(node);
            TB(ob, T_A + 0) = __float_as_uint(t_col.x); TB(ob, T_A + 1) = __float_as_uint(t_col.y); TB(ob, T_A + 2) = __float_as_uint(t_col.z);
            TB(ob, T_KIDS) = (k_refr ? idt : T_NONE) | ((k_refl ? idr : T_NONE) << 16);
            TB(ob, T_META) = (meta & ~7u) | (shade ? (unsigned)TK_HIT : (unsigned)TK_COLOUR);
            if (shade) {
                TB(ob, T_O + 0) = __float_as_uint(ip.x); TB(ob, T_O + 1) = __float_as_uint(ip.y); TB(ob, T_O + 2) = __float_as_uint(ip.z);
                TB(ob, T_D + 0) = __float_as_uint(nrm.x); TB(ob, T_D + 1) = __float_as_uint(nrm.y); TB(ob, T_D + 2) = __float_as_uint(nrm.z);
                TB(ob, T_V + 0) = __float_as_uint(view.x); TB(ob, T_V + 1) = __float_as_uint(view.y); TB(ob, T_V + 2) = __float_as_uint(view.z);
                TB(ob, T_N1) = __float_as_uint(m.shininess);
                TB(ob, T_KS) = __float_as_uint(ks); TB(ob, T_KD) = __float_as_uint(kd);
                TB(ob, T_AMB) = __float_as_uint(t_ambk);
                TF(T_HITS, t_nh + (unsigned)__builtin_popcountll(mh & t_lt)) = node;
            }
        }
        t_nh += (unsigned)__builtin_popcountll(mh);
        t_count += ct + cr;
    }
#include "whitted_terms.inc"

    T_PHASE(1);
    if (!t_abort) {
    /* ---- B: subtree sizes (bottom-up), depth-first positions (top-down) ----------------------------------------------------------
     * One word per node carries two counts: nodes (low half) and shaded hits (high half) -- of the subtree first, then before the node in
     * its pixel's depth-first order, offset by everything the lanes before this pixel's hold: position and hit ordinal are wave-wide
     * indices.  The second sweep also lays out, BY POSITION, what the replay will add for the node (T_ORDER, T_PA, T_PS ...): the
     * replay then streams through consecutive addresses it knows in advance instead of chasing node ids. */
    __syncthreads();
    /* Small pools (most of them) keep that word in LDS -- the DFS stack's levels, free since the roots are out: a sweep step is then one
     * round trip (the node's own fields) instead of three (fields, the children's counts, the store to be seen by the next batch). */
    const bool t_small = t_count <= (unsigned)(LDSL * WT_REC * WT_BLOCK);
    auto t_cnt = [&](unsigned i) -> unsigned { return t_small ? __float_as_uint(s_stk[i]) : TF(T_POS, i); };
    auto t_cnt_set = [&](unsigned i, unsigned v) { if (t_small) s_stk[i] = __uint_as_float(v); else TF(T_POS, i) = v; };
    for (int b = (int)t_nb - 1; b >= 0; b--) {
        const unsigned s0 = s_tpt_bs[b], e0 = s_tpt_bs[b + 1];
        const unsigned node = s0 + lane;
        if (node < e0) {
            unsigned* const nb = TN(node);
            const unsigned kids = TB(nb, T_KIDS), meta = TB(nb, T_META);
            unsigned sz = 1u + (((meta & 7u) == (unsigned)TK_HIT ? 1u : 0u) << 16);
            if ((kids & 0xFFFFu) != T_NONE) sz += t_cnt(kids & 0xFFFFu);
            if ((kids >> 16) != T_NONE) sz += t_cnt(kids >> 16);
            t_cnt_set(node, sz);
        }
        if (!t_small) __syncthreads();
    }
    const unsigned t_total = t_alive ? t_cnt(t_root) : 0u;          /* nodes | hits << 16 of this lane's pixel */
    unsigned t_base = t_total;                       /* exclusive prefix sum over the lanes (both halves at once: the sums stay below 2^16) */
    for (int off = 1; off < 64; off <<= 1) { const unsigned v = (unsigned)__shfl_up((int)t_base, off); if ((int)lane >= off) t_base += v; }
    t_base -= t_total;
    if (!t_small) __syncthreads();
    if (t_alive) t_cnt_set(t_root, t_base);
    if (!t_small) __syncthreads();
    for (unsigned b = 0; b < t_nb; b++) {
        const unsigned s0 = s_tpt_bs[b], e0 = s_tpt_bs[b + 1];
        const unsigned node = s0 + lane;
        if (node < e0) {
            unsigned* const nb = TN(node);
            const unsigned pw = t_cnt(node), kids = TB(nb, T_KIDS), meta = TB(nb, T_META);
            const unsigned kt = kids & 0xFFFFu, kr = kids >> 16, kind = meta & 7u, pos = pw & 0xFFFFu;
            unsigned* const pb = TN(pos);
            const unsigned nxt = pw + 1u + ((kind == (unsigned)TK_HIT ? 1u : 0u) << 16);
            unsigned szt = 0u;
            if (kt != T_NONE) { szt = t_cnt(kt); t_cnt_set(kt, nxt); }                 /* the refracted subtree comes first */
            if (kr != T_NONE) t_cnt_set(kr, nxt + szt);
            TB(pb, T_ORDER) = node | (kind << 16) | (((meta >> 15) & 63u) << 19) | ((kt != T_NONE ? 1u : 0u) << 25) | ((kr != T_NONE ? 1u : 0u) << 26);
            TB(pb, T_PA + 0) = TB(nb, T_A + 0); TB(pb, T_PA + 1) = TB(nb, T_A + 1); TB(pb, T_PA + 2) = TB(nb, T_A + 2);
            TB(pb, T_PS) = kind == (unsigned)TK_HIT ? TB(nb, T_AMB) : TB(nb, T_F);
#if WT_STRICT
            if (kind == (unsigned)TK_HIT) { TB(pb, T_PK + 0) = TB(nb, T_KS); TB(pb, T_PK + 1) = TB(nb, T_KD); }
#endif
        }
        if (!t_small) __syncthreads();
    }

    T_PHASE(2);
    /* ---- C: the xorshift state of every shaded hit: 4 numbers per light and hit, drawn or not (raytracing.cl:96-100).  One lane per pixel
     *      steps through its pixel's hits in order -- arithmetic and stores only, nothing to wait for -- and leaves the states by hit ordinal */
    {
        /* xorshift32 is linear over GF(2): the state k hits on is M^k x the state now (M = one hit's 4 nl steps; P.tpt_jump holds M^(2^i) as columns).
         * With few pixels left -- the deep trees this tail exists for -- a pixel's hits are dealt over a GROUP of G = 2^lg lanes: lane j of the group
         * jumps to hit j (the set bits of j), stores every G-th state and strides by M^G; with more than 32 pixels a lane steps through its own. */
        const unsigned long long am = __builtin_amdgcn_ballot_w64(t_alive);
        const unsigned na = (unsigned)__builtin_popcountll(am), steps = 2u * WT_SOFT * P.nl;
        unsigned lg = 0u;
        while (lg < 6u && (na << (lg + 1u)) <= 64u) lg++;
        if (lg == 0u) {
            if (t_alive) {
                unsigned st = t_rng0;
                const unsigned h0 = t_base >> 16, h1 = h0 + (t_total >> 16);
                for (unsigned h = h0; h < h1; h++) {
                    TF(T_RS, h) = st;
                    for (unsigned i = 0; i < steps; i++) { st ^= st << 13; st ^= st >> 17; st ^= st << 5; }
                }
            }
        } else {
            if (t_alive) {
                const unsigned r_ = (unsigned)__builtin_popcountll(am & t_lt);
                s_tpt_px[3u * r_] = t_rng0; s_tpt_px[3u * r_ + 1u] = t_base >> 16; s_tpt_px[3u * r_ + 2u] = t_total >> 16;
            }
            auto t_matvec = [&](const unsigned* Mx, unsigned x) {
                unsigned acc = 0u;
#pragma unroll
                for (int b_ = 0; b_ < 32; b_++) acc ^= (0u - ((x >> b_) & 1u)) & Mx[b_];
                return acc;
            };
            const unsigned grp = lane >> lg, j = lane & ((1u << lg) - 1u);
            if (grp < na) {
                unsigned st = s_tpt_px[3u * grp];
                const unsigned h0 = s_tpt_px[3u * grp + 1u], nh = s_tpt_px[3u * grp + 2u];
                for (unsigned i = 0; i < lg; i++) {                    /* wave-uniform trip count: M^j by the set bits of j */
                    const unsigned nx = t_matvec(P.tpt_jump + 32u * i, st);
                    if ((j >> i) & 1u) st = nx;
                }
                unsigned mg[32];                                      /* M^G, read once */
#pragma unroll
                for (int b_ = 0; b_ < 32; b_++) mg[b_] = P.tpt_jump[32u * lg + (unsigned)b_];
                for (unsigned h = j; h < nh; h += 1u << lg) {
                    TF(T_RS, h0 + h) = st;
                    st = t_matvec(mg, st);
                }
            }
        }
    }
    __syncthreads();

    T_PHASE(3);
    /* ---- D: shading, one hit per lane; the lights' factors go where the replay will look for them: at the hit's position -------------- */
#undef WT_MOTION
#define WT_MOTION (wt_motion{false, 0.0f, 0u})
#undef WT_SHADE_ADD
#if WT_STRICT
#define WT_SHADE_ADD(li, l1, soft, dl, spec, diff) do { const unsigned w_ = T_W + 4u * (li); (void)(l1); \
        TB(wb_, w_) = __float_as_uint(soft); TB(wb_, w_ + 1u) = __float_as_uint(dl); \
        TB(wb_, w_ + 2u) = __float_as_uint(spec); TB(wb_, w_ + 3u) = __float_as_uint(diff); } while (0)
#else   /* wt_light_add's fast form is rgb = l1 * (spec * soft) + rgb: the product travels */
#define WT_SHADE_ADD(li, l1, soft, dl, spec, diff) do { (void)(l1); (void)(dl); (void)(diff); TB(wb_, T_W + (li)) = __float_as_uint((spec) * (soft)); } while (0)
#endif
    for (unsigned hb = 0; hb < t_nh; hb += 64u) {
        if (hb + lane < t_nh) {
            const unsigned t_node = TF(T_HITS, hb + lane);
            const unsigned* const hb_ = TN(t_node);
            const unsigned t_pw = t_cnt(t_node), t_pos = t_pw & 0xFFFFu;
            const f3 ip = mk3(__uint_as_float(TB(hb_, T_O + 0)), __uint_as_float(TB(hb_, T_O + 1)), __uint_as_float(TB(hb_, T_O + 2)));
            const f3 nrm = mk3(__uint_as_float(TB(hb_, T_D + 0)), __uint_as_float(TB(hb_, T_D + 1)), __uint_as_float(TB(hb_, T_D + 2)));
            const f3 view = mk3(__uint_as_float(TB(hb_, T_V + 0)), __uint_as_float(TB(hb_, T_V + 1)), __uint_as_float(TB(hb_, T_V + 2)));
            mat_t m;
            m.shininess = __uint_as_float(TB(hb_, T_N1));
            const float ks = __uint_as_float(TB(hb_, T_KS)), kd = __uint_as_float(TB(hb_, T_KD));
            rng = TF(T_RS, t_pw >> 16);
            unsigned* const wb_ = TN(t_pos);
#include "whitted_shade.inc"
        }
    }
#include "whitted_terms.inc"
    __syncthreads();

    T_PHASE(4);
    /* ---- E: replay -- the additions of raytracing.cl:52,78,83-84,112-135,183-190 per pixel, in the reference's order.  Eight positions
     *      (WT_TPT_RC; strict: two) at a time: everything they will add is requested before the first addition waits for it. -------------------------- */
    if (t_alive) {
        f3 acc = mk3(0, 0, 0);
        unsigned cur = 0u;                           /* open refraction levels = saved sums */
        bool ended_path = false;
        constexpr int RC = WT_STRICT ? 2 : WT_TPT_RC, RW = 3 * (int)T_LW;   /* positions per round; weight words preloaded per position (scenes of <= 3 lights) */
        const unsigned p_end = (t_base & 0xFFFFu) + (t_total & 0xFFFFu);
        const bool few = P.nl <= 3u;
        /* the saved sums: the first levels in LDS (the DFS stack's, free by now), deeper ones in the slot -- a pop is a dependent load */
        constexpr unsigned RL = WT_TPT_RSTK_LDS ? (unsigned)(LDSL * WT_REC / 3) : 0u;
        auto t_save = [&](unsigned lv_, f3 v) {
            if (lv_ < RL) { s_stk[(lv_ * 3u + 0u) * 64u + lane] = v.x; s_stk[(lv_ * 3u + 1u) * 64u + lane] = v.y; s_stk[(lv_ * 3u + 2u) * 64u + lane] = v.z; }
            else { T_RSTK[(lv_ * 3u + 0u) * 64u + lane] = __float_as_uint(v.x); T_RSTK[(lv_ * 3u + 1u) * 64u + lane] = __float_as_uint(v.y); T_RSTK[(lv_ * 3u + 2u) * 64u + lane] = __float_as_uint(v.z); }
        };
        auto t_saved = [&](unsigned lv_) {
            if (lv_ < RL) return mk3(s_stk[(lv_ * 3u + 0u) * 64u + lane], s_stk[(lv_ * 3u + 1u) * 64u + lane], s_stk[(lv_ * 3u + 2u) * 64u + lane]);
            return mk3(__uint_as_float(T_RSTK[(lv_ * 3u + 0u) * 64u + lane]), __uint_as_float(T_RSTK[(lv_ * 3u + 1u) * 64u + lane]), __uint_as_float(T_RSTK[(lv_ * 3u + 2u) * 64u + lane]));
        };
        struct t_round { unsigned e[RC], wq[RC][RW]; f3 a[RC]; float sc[RC], pks[RC], pkd[RC]; };
        auto t_fetch = [&](unsigned p0, t_round& r) {
#pragma unroll
            for (int i = 0; i < RC; i++) {
                const unsigned q = min(p0 + (unsigned)i, p_end - 1u);
                const unsigned* const qb = TN(q);
                r.e[i] = TB(qb, T_ORDER);
                r.a[i] = mk3(__uint_as_float(TB(qb, T_PA + 0)), __uint_as_float(TB(qb, T_PA + 1)), __uint_as_float(TB(qb, T_PA + 2)));
                r.sc[i] = __uint_as_float(TB(qb, T_PS));
                r.pks[i] = r.pkd[i] = 0.0f;
#if WT_STRICT
                r.pks[i] = __uint_as_float(TB(qb, T_PK + 0)); r.pkd[i] = __uint_as_float(TB(qb, T_PK + 1));
#endif
#pragma unroll
                for (int k = 0; k < RW; k++) r.wq[i][k] = (few && (unsigned)k < T_LW * P.nl) ? TB(qb, T_W + k) : 0u;
            }
        };
        float4 l1c[3];                                   /* the lights' colours, read once (scenes of <= 3 lights) */
#pragma unroll
        for (int k = 0; k < 3; k++) l1c[k] = (few && (unsigned)k < P.nl) ? wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (unsigned)k + 1) : make_float4(0, 0, 0, 0);
        for (unsigned p0 = t_base & 0xFFFFu; p0 < p_end; p0 += RC) {
            t_round cu;
            t_fetch(p0, cu);
            const unsigned (&e)[RC] = cu.e; const unsigned (&wq)[RC][RW] = cu.wq; const f3 (&a)[RC] = cu.a;
            const float (&sc)[RC] = cu.sc; const float (&pks)[RC] = cu.pks; const float (&pkd)[RC] = cu.pkd;
#pragma unroll
            for (int i = 0; i < RC; i++) {
                if (p0 + (unsigned)i < p_end) {
                    const unsigned kind = (e[i] >> 16) & 7u, lv = (e[i] >> 19) & 63u;
                    if (ended_path) {                /* the paths that ended hand their sums down: parent + child */
                        while (cur > lv) {
                            cur--;
                            acc = t_saved(cur) + acc;
                        }
                        ended_path = false;
                    }
                    if (kind == (unsigned)TK_VIRTUAL) {
                        acc = a[i];
                    } else if (kind == (unsigned)TK_HIT) {
                        acc = wt_madd3(a[i], sc[i], acc);
                        for (unsigned li = 0; li < P.nl; li++) {
                            const float4 l1 = few ? (li == 0u ? l1c[0] : (li == 1u ? l1c[1] : l1c[2])) : wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * li + 1);
#if WT_STRICT
                            float w4[4];
#pragma unroll
                            for (int k = 0; k < 4; k++) w4[k] = __uint_as_float(few ? (li == 0u ? wq[i][k] : (li == 1u ? wq[i][4 + k] : wq[i][8 + k])) : TF(T_W + 4u * li + (unsigned)k, p0 + (unsigned)i));
                            acc = wt_light_add(acc, l1, w4[0], w4[1], w4[2], w4[3], pks[i], pkd[i]);
#else
                            const float w1 = __uint_as_float(few ? (li == 0u ? wq[i][0] : (li == 1u ? wq[i][1] : wq[i][2])) : TF(T_W + li, p0 + (unsigned)i));
                            acc = wt_madd3(mk3(l1.x, l1.y, l1.z), w1, acc);
#endif
                        }
                    } else {
                        acc = wt_madd3(a[i], sc[i], acc);
                    }
                    if ((e[i] >> 25) & 1u) {         /* a refracted child follows: the path's sum waits (raytracing.cl:171-176) */
                        t_save(cur, acc);
                        acc = mk3(0, 0, 0); cur++;
                    } else if (!((e[i] >> 26) & 1u)) {
                        ended_path = true;
                    }
                }
            }
        }
        while (cur > 0u) {
            cur--;
            acc = t_saved(cur) + acc;
        }
        rgb = acc;
    }
    active = false;
    tpt_done = true;
    __syncthreads();
    T_PHASE(5);
    if (COUNT && lane == 0) { c_tptrun++; c_tptnodes += t_count; }
    if (t_clock && lane == 0) {
#pragma unroll
        for (int k_ = 0; k_ < 6; k_++) { atomicAdd(P.counters + 10 + k_, (unsigned long long)t_ph[k_]); atomicMax(P.counters + 20 + k_, (unsigned long long)t_ph[k_]); }
        atomicAdd(P.counters + 16, (unsigned long long)t_nb);                         /* batches */
        atomicMax(P.counters + 17, (unsigned long long)t_nb);
        atomicMax(P.counters + 18, (unsigned long long)t_count);
        unsigned tot_ = 0u; for (int k_ = 0; k_ < 6; k_++) tot_ += t_ph[k_];
        atomicMax(P.counters + 19, (unsigned long long)tot_);                         /* the longest stay, ticks of 10 ns */
    }
    }   /* !t_abort after the expansion */

    if (t_abort) {                                   /* the per-lane loop takes over from the parked state */
        __syncthreads();
        o = mk3(__uint_as_float(T_SAVE[0 * 64 + lane]), __uint_as_float(T_SAVE[1 * 64 + lane]), __uint_as_float(T_SAVE[2 * 64 + lane]));
        d = mk3(__uint_as_float(T_SAVE[3 * 64 + lane]), __uint_as_float(T_SAVE[4 * 64 + lane]), __uint_as_float(T_SAVE[5 * 64 + lane]));
        rgb = mk3(__uint_as_float(T_SAVE[6 * 64 + lane]), __uint_as_float(T_SAVE[7 * 64 + lane]), __uint_as_float(T_SAVE[8 * 64 + lane]));
        depth = (int)T_SAVE[9 * 64 + lane];
        n1 = __uint_as_float(T_SAVE[10 * 64 + lane]); f = __uint_as_float(T_SAVE[11 * 64 + lane]);
        sp = (int)T_SAVE[12 * 64 + lane]; rng = T_SAVE[13 * 64 + lane];
        for (int w = 0; w < LDSL * WT_REC; w++) s_stk[w * WT_BLOCK + tid] = __uint_as_float(T_SAVE[(25 + w) * 64 + lane]);
        if (COUNT) {
            c_seg = T_SAVE[14 * 64 + lane]; c_shadow = T_SAVE[15 * 64 + lane]; c_probe = T_SAVE[16 * 64 + lane]; c_sky = T_SAVE[17 * 64 + lane];
            c_tex = T_SAVE[18 * 64 + lane]; c_push = T_SAVE[19 * 64 + lane]; c_iter = T_SAVE[20 * 64 + lane]; c_witer = T_SAVE[21 * 64 + lane];
            c_traced = T_SAVE[22 * 64 + lane]; c_known = T_SAVE[23 * 64 + lane]; c_visbad = T_SAVE[24 * 64 + lane];
            if (lane == 0) c_tptfail++;
        }
    }
    __syncthreads();                                 /* every lane's loads and stores of the slot are done: hand it back */
    if (lane == 0) atomicExch(P.tpt_flags + t_xcc * P.tpt_slots + t_slot, 0u);
    }   /* enough pending paths, and a slot */
#undef TF
#undef TB
#undef TN
#undef T_PHASE
}
