// rr_query_multi.hip -- multi-hit ray queries (rr_query_rays_multi[_device]) for gfx950.
//
// The DXR multi-hit idiom (an any-hit shader that records every candidate and calls IgnoreHit) as one walk per ray: the query
// kernels' traversal (trace_scene<..., QUERY>) with the MultiHits policy of rr_device.h instead of the closest hit.  The slots
// hold the KB first accepted triangles in (t, inst, prim) order; the attributes of each are computed after the walk, with the
// closest-hit path's operations on the ray in the slot's instance space, so t, u, v, prim and inst have the bits a closest-hit
// query reports for that triangle.
#include <hip/hip_runtime.h>
#include "rr_device.h"
#include "rr_launch.h"

namespace rr {

constexpr uint32_t HIT_KIND_FRONT = 0xFEu, HIT_KIND_BACK = 0xFFu;      // DXR HIT_KIND_TRIANGLE_FRONT_FACE / _BACK_FACE

// KB: slot capacity (the host picks the smallest of 1, 2, 4, 8, 16 that holds k); COUNT: counts[i] receives the number of
// accepted triangles (the walk is not pruned by the slots).  inst0_mask: as k_query_rays.
template <int STACK, bool TLAS, int KB, bool COUNT>
__global__ __launch_bounds__(256) void k_query_multi(SceneDev sc, const rr_ray_dev* rays, uint32_t n, uint32_t k, rr_hit_dev* hits,
                                                     uint32_t* counts, uint32_t inst0_mask)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t* stk = lds + wave * (STACK * 64) + lane;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(rays + i);
    const uint4 o = q[0], d = q[1], f = q[2];                   // f: flags, instance_mask, pad[2]
    const uint32_t mask = TLAS ? f.y : (f.y & inst0_mask);
    const f3 O = mk3(__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z));
    const f3 D = mk3(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    const float tmax = __uint_as_float(d.w);
    MultiHits<KB, COUNT> m;
    TravCounters cnt; cnt.nodes = 0; cnt.tris = 0;
    // RAY_FLAG_ACCEPT_FIRST_HIT is ignored: a multi-hit any-hit shader commits nothing, so there is nothing to end the search on
    trace_scene<false, TLAS, uint32_t, GlobalNodes, true>(sc, O, D, __uint_as_float(o.w), tmax, f.x, m, stk, cnt, Diag{ nullptr },
                                                          GlobalNodes{}, mask, false);
    if (COUNT) counts[i] = m.count;
    rr_hit_dev* out = hits + (size_t)i * k;
    const TriRec* __restrict__ tris = TLAS ? sc.pool_tris : sc.blas0.tris;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        if ((uint32_t)j >= k) continue;                         // (not break: a loop with two exits is not unrolled at KB = 16)
        rr_hit_dev r;
        if (m.t[j] < tmax) {                                    // a filled slot (an empty one holds tmax)
            HitRec h;
            h.leaf = m.leaf[j];
            f3 Oh = O, Dh = D;
            bool ccw = false;
            if (TLAS) {
                const InstDev in = inst_record(sc.insts, m.inst[j]);
                ray_in_instance(in, O, D, Oh, Dh);
                ccw = (in.flags & 0x2u) != 0u;                  // RR_INSTANCE_FLAG_TRIANGLE_FRONT_COUNTERCLOCKWISE swaps the faces
            }
            const float det = hit_attributes(tris, Oh, Dh, h);
            r.t = m.t[j];
            r.u = h.U / h.ad;
            r.v = h.V / h.ad;
            r.prim = h.prim; r.inst = m.inst[j];
            r.hit = ((det > 0.0f) != ccw) ? HIT_KIND_FRONT : HIT_KIND_BACK;
        } else {                                                // the closest-hit query's miss record
            r.t = tmax; r.u = 0.0f; r.v = 0.0f; r.prim = 0u; r.inst = 0u; r.hit = 0u;
        }
        out[j] = r;
    }
}

template <int STACK, bool TLAS, int KB>
static void launch_multi_st(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, uint32_t k, rr_hit_dev* hits, uint32_t* counts,
                            uint32_t inst0_mask, hipStream_t s)
{
    const dim3 grid((n + 255u) / 256u);
    const size_t lds = (size_t)4 * STACK * 64 * 4;
    if (counts) hipLaunchKernelGGL((k_query_multi<STACK, TLAS, KB, true>), grid, dim3(256), lds, s, sc, rays, n, k, hits, counts, inst0_mask);
    else        hipLaunchKernelGGL((k_query_multi<STACK, TLAS, KB, false>), grid, dim3(256), lds, s, sc, rays, n, k, hits, counts, inst0_mask);
}

template <int STACK, bool TLAS>
static void launch_multi_kb(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, uint32_t k, rr_hit_dev* hits, uint32_t* counts,
                            uint32_t inst0_mask, hipStream_t s)
{
    if (k <= 1)      launch_multi_st<STACK, TLAS, 1>(sc, rays, n, k, hits, counts, inst0_mask, s);
    else if (k <= 2) launch_multi_st<STACK, TLAS, 2>(sc, rays, n, k, hits, counts, inst0_mask, s);
    else if (k <= 4) launch_multi_st<STACK, TLAS, 4>(sc, rays, n, k, hits, counts, inst0_mask, s);
    else if (k <= 8) launch_multi_st<STACK, TLAS, 8>(sc, rays, n, k, hits, counts, inst0_mask, s);
    else             launch_multi_st<STACK, TLAS, 16>(sc, rays, n, k, hits, counts, inst0_mask, s);
}

hipError_t launch_query_multi(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, uint32_t k, rr_hit_dev* hits, uint32_t* counts,
                              uint32_t inst0_mask, int stack, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (k > RR_QUERY_MULTI_MAX_K || (k == 0 && !counts)) return hipErrorInvalidValue;
    if (stack <= 31) { if (sc.single_identity) launch_multi_kb<31, false>(sc, rays, n, k, hits, counts, inst0_mask, s);
                       else                    launch_multi_kb<31, true>(sc, rays, n, k, hits, counts, inst0_mask, s); }
    else             { if (sc.single_identity) launch_multi_kb<64, false>(sc, rays, n, k, hits, counts, inst0_mask, s);
                       else                    launch_multi_kb<64, true>(sc, rays, n, k, hits, counts, inst0_mask, s); }
    return hipGetLastError();
}

} // namespace rr
