/* whitted_projection.inc -- the camera models beside the pinhole (hip_wrap_ext.h: clw_projection; projection_host.h): the orthographic view
 * and the equirectangular panorama.  Included by whitted_launch.inc behind whitted_gbuffer.inc, so it exists in the fast and the strict unit.
 * THE definition of a model's rays is the host's (projection_host.c: clw_host_projection_rays); the host resolves a projection once per
 * (camera, frame, projection) into the scalar terms of wt_projection and, for the panorama, a column and a row table -- every sine, cosine and
 * double operation happens there -- and wt_proj_ray below performs on them the float operations wt_projection_ray performs, both compiled from
 * the one text of csrc/ref_tests.h, one rounding each (no contraction, IEEE square root and divide, in both units): host and device agree to
 * the bit.
 * A projected launch is never fused: wt_raygen_proj writes the 64-byte records the ray-buffer flavours (WT_F_RAYS) of wt_trace read, and the
 * primary-hit pass (wt_gbuffer) calls wt_proj_ray where it calls wt_primary_dir(_xy) for the pinhole.  The trace kernels know nothing of it. */

/* the ray of pixel (x, y) of the frame (T.model != CLW_PROJ_PERSPECTIVE): wt_projection_ray of projection_host.c with the device's table
 * addressing, the arithmetic being the one text of both (ref_tests.h) */
__device__ __forceinline__ void wt_proj_ray(const wt_projection& T, unsigned x, unsigned y, f3& o, f3& d) {
    if (T.model == CLW_PROJ_EQUIRECT) {
        /* (an index past a table cannot be: the shim sizes both for the frame the ids come from; the clamp keeps a stray id inside them) */
        const float4 c = ((const float4*)T.col)[x < T.width ? x : T.width - 1u];      /* coalesced along a row of the frame */
        const float4 r = ((const float4*)T.row)[y < T.height ? y : T.height - 1u];    /* one entry per lane; a block spans few rows */
        o = fv3(ref_ld(T.origin));
        d = fv3(ref_normalize(ref_madd(rv3(c), r.x, ref_mk(r.y, r.z, r.w))));
    } else {
        /* ORTHO: the image-plane vector the pinhole raygen would normalise is the origin's offset */
        o = fv3(ref_add(ref_ld(T.origin), ref_image_plane(ref_ld(T.corner), ref_ld(T.right), ref_ld(T.up), T.w_factor, T.h_factor, x, y)));
        d = fv3(ref_ld(T.dir));
    }
}

/* ---- the twin of wt_raygen for the two models: the same work-item -> id mapping (id offset, row bands), the same transposition through LDS,
 *      so that every store instruction of a wave writes 1 KiB of contiguous memory.  Store-bound like its twin (64 B per ray): the column
 *      table is read coalesced (16 B per lane), the row entry is one 16-byte load per lane from at most 256 / W + 2 rows of the table. ---- */
__global__ void __launch_bounds__(WT_RG_BLOCK) wt_raygen_proj(const raygen_params P, const wt_projection T) {
    constexpr int RS = WT_RG_BLOCK + 1;            /* padded row: conflict-free both ways */
    __shared__ float4 s_rec[4 * RS];               /* [part][ray] */
    const unsigned tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * WT_RG_BLOCK;
    const size_t item = base + tid;
    float4 r0 = make_float4(0, 0, 0, 0), r1 = r0;
    if (item < P.n_items) {
        unsigned long long gid = P.id_offset + item;
        if (P.band_stride > 1u) {
            const unsigned y = (unsigned)(item / P.width), x = (unsigned)(item % P.width);
            gid = (unsigned long long)(((y >> 3) * P.band_stride + P.band_phase) * 8u + (y & 7u)) * P.width + x;
        }
        f3 o, d;
        wt_proj_ray(T, (unsigned)gid % P.width, (unsigned)gid / P.width, o, d);
        r0 = make_float4(o.x, o.y, o.z, 0.0f);
        r1 = make_float4(d.x, d.y, d.z, 0.0f);
    }
    /* record = {origin, dir, rgb = 0, depth = 0 + pad}; rows 2,3 are zero */
    s_rec[0 * RS + tid] = r0;
    s_rec[1 * RS + tid] = r1;
    s_rec[2 * RS + tid] = make_float4(0, 0, 0, 0);
    s_rec[3 * RS + tid] = make_float4(0, 0, 0, 0);
    __syncthreads();
    float4* dst = (float4*)P.rays + base * 4;
    const size_t limit = ((size_t)P.n_items - base < WT_RG_BLOCK ? (size_t)P.n_items - base : WT_RG_BLOCK) * 4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        size_t q = (size_t)k * WT_RG_BLOCK + tid;      /* float4 index inside the block's 16 KiB */
        if (q < limit) dst[q] = s_rec[(q & 3) * RS + (q >> 2)];
    }
}
