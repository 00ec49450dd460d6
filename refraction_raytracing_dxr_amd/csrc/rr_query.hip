// rr_query.hip -- one stage of the pipeline on caller input: Miss (k_env_lookup) and TraceRay (k_trace_rays, k_query_rays) in
// isolation.  The K-nearest form of the query is rr_query_multi.hip.
#include <hip/hip_runtime.h>
#include "rr_device.h"
#include "rr_launch.h"

namespace rr {

// Miss in isolation, for the parity tests (rr_env_lookup): dirs / rgb are n x 3 floats
__global__ __launch_bounds__(256) void k_env_lookup(SceneDev sc, const float* dirs, uint32_t n, float* rgb)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 e = env_lookup(sc, mk3(dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]));
    rgb[i * 3] = e.x; rgb[i * 3 + 1] = e.y; rgb[i * 3 + 2] = e.z;
}

// TraceRay in isolation, for the parity tests (rr_trace_rays)
template <int STACK, bool TLAS>
__global__ __launch_bounds__(256) void k_trace_rays(SceneDev sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits,
                                                    uint32_t* error_flag)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    uint32_t* stk = lds + wave * (STACK * 64) + lane;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4* q = reinterpret_cast<const float4*>(rays + i);
    float4 o = q[0], d = q[1];
    uint32_t flags = rays[i].flags;
    HitRec h;
    TravCounters cnt; cnt.nodes = 0; cnt.tris = 0;
    trace_scene<false, TLAS>(sc, mk3(o.x, o.y, o.z), mk3(d.x, d.y, d.z), o.w, d.w, flags, h, stk, cnt);
    rr_hit_dev r;
    r.hit = h.hit ? 1u : 0u;
    r.t = h.hit ? h.t : d.w;
    r.u = h.hit ? h.U / h.ad : 0.0f;
    r.v = h.hit ? h.V / h.ad : 0.0f;
    r.prim = h.prim; r.inst = h.inst;
    hits[i] = r;
}

// TraceRay(Scene, flags, instance_mask, ...) on caller rays (rr_query_rays, rr_query_rays_device): the trace kernel with the
// ray's InstanceInclusionMask and RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH read per lane, so one launch may mix first-hit and
// closest-hit rays (an instantiation without the per-lane test was measured no faster on closest-hit batches: DESIGN 5.4).
// inst0_mask: the InstanceMask of the one instance of a TLAS = false scene (a kernel argument rather than a SceneDev field:
// the render kernels' register allocation follows SceneDev's layout).
template <int STACK, bool TLAS>
__global__ __launch_bounds__(256) void k_query_rays(SceneDev sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t inst0_mask)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t* stk = lds + wave * (STACK * 64) + lane;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(rays + i);
    const uint4 o = q[0], d = q[1], f = q[2];                   // f: flags, instance_mask, pad[2]
    const uint32_t flags = f.x;
    const uint32_t mask = TLAS ? f.y : (f.y & inst0_mask);
    const bool any = (flags & RAY_FLAG_ACCEPT_FIRST_HIT) != 0u;
    HitRec h;
    TravCounters cnt; cnt.nodes = 0; cnt.tris = 0;
    trace_scene<false, TLAS, uint32_t, GlobalNodes, true>(sc, mk3(__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z)),
                                                          mk3(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z)),
                                                          __uint_as_float(o.w), __uint_as_float(d.w), flags, h, stk, cnt,
                                                          Diag{ nullptr }, GlobalNodes{}, mask, any);
    rr_hit_dev r;
    r.hit = h.hit ? 1u : 0u;
    r.t = h.hit ? h.t : __uint_as_float(d.w);
    r.u = h.hit ? h.U / h.ad : 0.0f;
    r.v = h.hit ? h.V / h.ad : 0.0f;
    r.prim = h.prim; r.inst = h.inst;
    hits[i] = r;
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_env_lookup(const SceneDev& sc, const float* dirs, uint32_t n, float* rgb, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_env_lookup, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, dirs, n, rgb);
    return hipGetLastError();
}

template <int STACK, bool TLAS>
static void launch_trace_st(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t* err, hipStream_t s)
{
    hipLaunchKernelGGL((k_trace_rays<STACK, TLAS>), dim3((n + 255u) / 256u), dim3(256), 4 * STACK * 64 * 4, s, sc, rays, n, hits, err);
}

hipError_t launch_trace_rays(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t* err,
                             int stack, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (stack <= 31) { if (sc.single_identity) launch_trace_st<31, false>(sc, rays, n, hits, err, s); else launch_trace_st<31, true>(sc, rays, n, hits, err, s); }
    else             { if (sc.single_identity) launch_trace_st<64, false>(sc, rays, n, hits, err, s); else launch_trace_st<64, true>(sc, rays, n, hits, err, s); }
    return hipGetLastError();
}

template <int STACK, bool TLAS>
static void launch_query_st(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t inst0_mask, hipStream_t s)
{
    hipLaunchKernelGGL((k_query_rays<STACK, TLAS>), dim3((n + 255u) / 256u), dim3(256), 4 * STACK * 64 * 4, s, sc, rays, n, hits, inst0_mask);
}

hipError_t launch_query_rays(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t inst0_mask, int stack,
                             hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (stack <= 31) { if (sc.single_identity) launch_query_st<31, false>(sc, rays, n, hits, inst0_mask, s); else launch_query_st<31, true>(sc, rays, n, hits, inst0_mask, s); }
    else             { if (sc.single_identity) launch_query_st<64, false>(sc, rays, n, hits, inst0_mask, s); else launch_query_st<64, true>(sc, rays, n, hits, inst0_mask, s); }
    return hipGetLastError();
}

} // namespace rr
