/* whitted_cull.inc -- the device builder of the cull table: the primary byte (primary_cull_host.h: the rule, its margin and wt_cull_tile, THE
 * arithmetic, compiled here a second time from the same text) and above it the bounce byte (bounce_cull_host.h: wt_bc_tile, likewise) of every
 * tile, one 16-bit entry each; wt_trace_cull reads the table (whitted_trace.inc, whitted_hit.inc).  One thread per 8x8 tile of the launch's tile
 * grid, row-major as wt_trace_body numbers its tiles; the prepared geometry is read from global memory (a few float4, the same for every
 * thread).  The shim runs it on the launch stream ahead of the trace, and only when the camera, the scene, the frame or the row range changed
 * since the table was built (hip_wrap.cpp: bind_primary_cull). */
struct wt_cull_args {
    wt_cull_view V;
    wt_bc_scene S;                                  /* geom, geom + 4 ns, geom + 4 (ns + 2 np); the raw planes; the counts and the launch's depth */
    unsigned tiles, tpr, parts;                     /* parts: WT_BC_PART_* of the bounce byte to compute */
    unsigned char* table;                           /* 2 * `tiles` bytes (the allocation is rounded up to whole words: the kernel reads words) */
};
__global__ void __launch_bounds__(256) wt_primary_cull_build(const wt_cull_args A) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= A.tiles) return;
    const uint8_t prim = wt_cull_tile(&A.V, t % A.tpr, t / A.tpr, A.S.spheres, A.S.ns, A.S.lights, A.S.nl);
    A.table[2u * t] = prim;
    A.table[2u * t + 1u] = wt_bc_tile(&A.V, t % A.tpr, t / A.tpr, prim, &A.S, A.parts);
}
