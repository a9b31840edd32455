/* whitted_cull.inc -- the device builder of the primary-ray cull table (primary_cull_host.h: the rule, its margin and wt_cull_tile, THE
 * arithmetic, compiled here a second time from the same text; whitted_hit.inc reads the table).  One thread per 8x8 tile of the launch's tile
 * grid, row-major as wt_trace_body numbers its tiles; the prepared geometry is read from global memory (a few float4, the same for every
 * thread).  The shim runs it on the launch stream ahead of the trace, and only when the camera, the scene, the frame or the row range changed
 * since the table was built (hip_wrap.cpp: bind_primary_cull). */
struct wt_cull_args {
    wt_cull_view V;
    const float* spheres; const float* lights;      /* geom, geom + 4 (ns + 2 np) */
    unsigned ns, nl, tiles, tpr;
    unsigned char* table;                           /* `tiles` bytes (the allocation is rounded up to whole words: the kernel reads words) */
};
__global__ void __launch_bounds__(256) wt_primary_cull_build(const wt_cull_args A) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= A.tiles) return;
    A.table[t] = wt_cull_tile(&A.V, t % A.tpr, t / A.tpr, A.spheres, A.ns, A.lights, A.nl);
}
