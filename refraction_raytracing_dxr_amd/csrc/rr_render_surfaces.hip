// rr_render_surfaces.hip -- opaque hit groups (rr_shade_rays_surfaces[_device], rr_render_surfaces[_device]) for gfx950:
// k_shade_rays_nested and k_render_nested over the ray tree of rr_render_surfaces.h, in which an instance whose row of the surface
// table is opaque is lit by the context's lights through shadow rays, emits, and may continue as a mirror.
//
// The shapes are the nested kernels': a wave is 64 consecutive caller rays, or one 8x8 pixel block whose lanes loop over the samples;
// instantiations come from for_tree_variant and occupancy from ShadeWaves; the LDS stacks are the same, and the shadow rays walk on
// them.  The surface table is read like the material table, per lane through vector loads.  The lights and the ambient term are the
// same for every lane and travel by value as a kernel argument (LightsDev, 8 x 32 + 16 bytes).
//
// Each kernel has a twin for transparent shadows (rr_set_shadow_steps), k_shade_rays_shadows and k_render_shadows: the same body
// over the tree's WALK form (rr_render_shadows.h), with one more argument, shadow_k, the cap on a walk's TraceRay calls
// (1 .. SHADOW_MAX_STEPS), the same for every lane, so the walk's loop has a scalar bound.  The launchers pick the twin where the cap
// is not 0.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_shadows.h"

namespace rr {

// What the kernels hand to shade_caller_ray and render_frame: one written closure per kernel pair.  WALK: the tree's form; shadow_k
// is read by that form only.  The members are references to the kernel's arguments, as a lambda's captures are (by value the
// first-hit kernels' instructions come out in another order than they had as lambdas)
template <int PEND, bool TLAS, class E, bool WALK>
struct SurfacesRay {
    const SceneDev& sc; const DispatchDev& a; const MatDev* const& mats; const SurfArgs& sf; const LightsDev& lights;
    uint32_t shadow_k; const uint32_t& mat0;
    __device__ __forceinline__ f3 operator()(const RayState& r, E* stk, LaneStats& st) const
    {
        RegParkNested<PEND> park;
        return ray_tree_surfaces<TLAS, E, WALK>(sc, a, mats, sf, lights, mat0, with_empty_media(r), stk, park, st, shadow_k);
    }
};
template <int PEND, bool TLAS, class E, bool WALK>
struct SurfacesSample {
    const SceneDev& sc; const DispatchDev& a; const CamDev& cam; const SampleOffsets& off; const MatDev* const& mats; const SurfArgs& sf;
    const LightsDev& lights; uint32_t shadow_k; const uint32_t& mat0;
    __device__ __forceinline__ f3 operator()(uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) const
    {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        if (!may_hit) return culled_sample(sc, r.D, st);
        RegParkNested<PEND> park;
        return ray_tree_surfaces<TLAS, E, WALK>(sc, a, mats, sf, lights, mat0, with_empty_media(r), stk, park, st, shadow_k);
    }
};

// k_shade_rays_nested's arguments, the surface table and the lights
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays_surfaces(SceneDev sc, DispatchDev a, const MatDev* mats, SurfArgs sf,
                                                                                                  LightsDev lights, uint32_t mat0, const rr_ray_dev* rays,
                                                                                                  uint32_t n, float4* out_f32, uint32_t* out_rgba8,
                                                                                                  uint32_t* out_n)
{
    shade_caller_ray<STACK, E>(a, rays, n, out_f32, out_rgba8, out_n, SurfacesRay<PEND, TLAS, E, false>{ sc, a, mats, sf, lights, 0u, mat0 });
}

// k_shade_rays_surfaces' arguments and the cap
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays_shadows(SceneDev sc, DispatchDev a, const MatDev* mats, SurfArgs sf,
                                                                                                 LightsDev lights, uint32_t shadow_k, uint32_t mat0,
                                                                                                 const rr_ray_dev* rays, uint32_t n, float4* out_f32,
                                                                                                 uint32_t* out_rgba8, uint32_t* out_n)
{
    shade_caller_ray<STACK, E>(a, rays, n, out_f32, out_rgba8, out_n, SurfacesRay<PEND, TLAS, E, true>{ sc, a, mats, sf, lights, shadow_k, mat0 });
}

// k_render_nested's arguments, the surface table and the lights
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_surfaces(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                              const MatDev* mats, SurfArgs sf, LightsDev lights, uint32_t mat0,
                                                                                              uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                              float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           SurfacesSample<PEND, TLAS, E, false>{ sc, a, cam, off, mats, sf, lights, 0u, mat0 });
}

// k_render_surfaces' arguments and the cap
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_shadows(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                             const MatDev* mats, SurfArgs sf, LightsDev lights,
                                                                                             uint32_t shadow_k, uint32_t mat0, uint32_t n_samples,
                                                                                             uint32_t blocks_x, uint32_t n_blocks, float4* out_f32,
                                                                                             uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           SurfacesSample<PEND, TLAS, E, true>{ sc, a, cam, off, mats, sf, lights, shadow_k, mat0 });
}

hipError_t launch_shade_rays_surfaces(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, const SurfaceLaunch& su, uint32_t mat0,
                                      const rr_ray_dev* rays, uint32_t n, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (v.stack > 64 || v.pend > 8 || !su.ok(mats)) return hipErrorInvalidValue;
    const SurfArgs sf = { su.surfs, su.n_surfs };
    if (su.shadow_k)
        return RR_LAUNCH_TREE_KERNEL(k_shade_rays_shadows, sc.single_identity != 0u, v, (n + 255u) / 256u, s, sc, a, mats, sf, *su.lights, su.shadow_k, mat0,
                                     rays, n, out.f32, out.rgba8, out.n_rays);
    return RR_LAUNCH_TREE_KERNEL(k_shade_rays_surfaces, sc.single_identity != 0u, v, (n + 255u) / 256u, s, sc, a, mats, sf, *su.lights, mat0, rays, n, out.f32,
                                 out.rgba8, out.n_rays);
}

hipError_t launch_render_surfaces(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                  const SurfaceLaunch& su, uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !su.ok(mats)) return hipErrorInvalidValue;
    const SurfArgs sf = { su.surfs, su.n_surfs };
    if (su.shadow_k)
        return RR_LAUNCH_TREE_KERNEL(k_render_shadows, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, mats, sf, *su.lights, su.shadow_k, mat0,
                                     n_samples, fb.blocks_x, fb.n_blocks, out.f32, out.rgba8, out.n_rays);
    return RR_LAUNCH_TREE_KERNEL(k_render_surfaces, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, mats, sf, *su.lights, mat0, n_samples,
                                 fb.blocks_x, fb.n_blocks, out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
