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
#include "rr_render_frame.h"

namespace rr {

// a: only what shade_ray and store_pixel read (bounce limits, ior, secondary interval, tonemap; compact_out = 0).
// Each output is written only if its pointer is given (wave-uniform branches on kernel arguments).
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays(SceneDev sc, DispatchDev a, const rr_ray_dev* rays, uint32_t n,
                                                                                         float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    shade_caller_ray<STACK, E>(a, rays, n, out_f32, out_rgba8, out_n, [&](const RayState& r, E* stk, LaneStats& st) {
        RegPark<PEND> park;
        return ray_tree<TLAS, E>(sc, a, r, stk, park, st);
    });
}

hipError_t launch_shade_rays(const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* rays, uint32_t n, const ShadeOut& out, FusedVariant v,
                             hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (v.stack > 64 || v.pend > 8) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_shade_rays, sc.single_identity != 0u, v, (n + 255u) / 256u, s, sc, a, rays, n, out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
