// rr_shade_rays.hip -- radiance queries (rr_shade_rays[_device]) for gfx950: the shader's whole ray tree on caller rays.
//
// A RayGen shader of the caller's own: where k_render_fused starts a lane on GenerateCameraRay's ray of its pixel, a lane here
// starts on the 48-byte record the caller wrote (origin, tmin, dir, tmax as they are; flags, mask and pad are not read), as
// RayGen's payload {colour 0, weight 1, outside, count 0}, and from there on runs render_pixel's loop (rr_render_common.h:
// trace_scene, then shade_ray -- ClosestHit / Miss, the refracted child followed, the reflected one parked
// in registers).  The arithmetic is that shared device code and nothing else, so the colour of a ray has the bits a dispatch
// gives the pixel with that primary ray.  One lane per ray, a wave is 64 consecutive rays: what coherence the batch has is the
// caller's order (DESIGN 5.5 has the cost of the orders measured).
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_common.h"

namespace rr {

// a: only what shade_ray and store_pixel read (bounce limits, ior, secondary interval, tonemap; compact_out = 0).
// Each output is written only if its pointer is given (wave-uniform branches on kernel arguments).
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays(SceneDev sc, DispatchDev a, const rr_ray_dev* rays, uint32_t n,
                                                                                         float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(rays + i);
    const uint4 o = q[0], d = q[1];                             // (q[2]: flags, instance_mask, pad -- the shader's TraceRay calls fix them)
    RayState r;
    r.O = mk3(__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z));
    r.D = mk3(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    r.tmin = __uint_as_float(o.w); r.tmax = __uint_as_float(d.w);
    r.w = 1.0f; r.count = 0; r.outside = true;                  // RayGen's payload (RayTracing.hlsl:57-60)
    LaneStats st;
    RegPark<PEND> park;
    const f3 acc = ray_tree<TLAS, E>(sc, a, r, stk, park, st);
    if (out_f32) out_f32[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
    if (out_rgba8) store_pixel(a, out_rgba8, nullptr, i, acc);
    if (out_n) out_n[i] = st.rays;
}

// stack, pend, stack16: a FusedVariant of the scene, through the ray-tree kernels' ladder (for_tree_variant, rr_choice.h)
hipError_t launch_shade_rays(const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* rays, uint32_t n, float4* f32, uint32_t* rgba8,
                             uint32_t* n_rays, int stack, int pend, bool stack16, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (stack > 64 || pend > 8) return hipErrorInvalidValue;
    return for_tree_variant(sc.single_identity != 0u, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_shade_rays<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n + 255u) / 256u), dim3(256), T::lds_bytes, s, sc, a, rays,
                           n, f32, rgba8, n_rays);
        return hipGetLastError();
    });
}

} // namespace rr
