// rr_render_surfaces.hip -- opaque hit groups (rr_shade_rays_surfaces[_device], rr_render_surfaces[_device]) for gfx950:
// k_shade_rays_nested and k_render_nested over the ray tree of rr_render_surfaces.h, in which an instance whose row of the surface
// table is opaque is lit by the context's lights through shadow rays, emits, and may continue as a mirror.
//
// The shapes are the nested kernels': a wave is 64 consecutive caller rays, or one 8x8 pixel block whose lanes loop over the samples;
// instantiations come from for_tree_variant and occupancy from ShadeWaves; the LDS stacks are the same, and the shadow rays walk on
// them.  The surface table is read like the material table, per lane through vector loads.  The lights and the ambient term are the
// same for every lane and travel by value as a kernel argument (LightsDev, 8 x 32 + 16 bytes).
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_surfaces.h"

namespace rr {

// k_shade_rays_nested's arguments, the surface table and the lights
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays_surfaces(SceneDev sc, DispatchDev a, const MatDev* mats, SurfArgs sf,
                                                                                                  LightsDev lights, uint32_t mat0, const rr_ray_dev* rays,
                                                                                                  uint32_t n, float4* out_f32, uint32_t* out_rgba8,
                                                                                                  uint32_t* out_n)
{
    shade_caller_ray<STACK, E>(a, rays, n, out_f32, out_rgba8, out_n, [&](const RayState& r, E* stk, LaneStats& st) {
        RegParkNested<PEND> park;
        return ray_tree_surfaces<TLAS, E>(sc, a, mats, sf, lights, mat0, with_empty_media(r), stk, park, st);
    });
}

// k_render_nested's arguments, the surface table and the lights
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_surfaces(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                              const MatDev* mats, SurfArgs sf, LightsDev lights, uint32_t mat0,
                                                                                              uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                              float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        if (!may_hit) return culled_sample(sc, r.D, st);
        RegParkNested<PEND> park;
        return ray_tree_surfaces<TLAS, E>(sc, a, mats, sf, lights, mat0, with_empty_media(r), stk, park, st);
    });
}

hipError_t launch_shade_rays_surfaces(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, const SurfDev* surfs, uint32_t n_surfs,
                                      const LightsDev& lights, uint32_t mat0, const rr_ray_dev* rays, uint32_t n, const ShadeOut& out, FusedVariant v,
                                      hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (v.stack > 64 || v.pend > 8 || !mats || (n_surfs && !surfs) || lights.n > MAX_LIGHTS) return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    return RR_LAUNCH_TREE_KERNEL(k_shade_rays_surfaces, sc.single_identity != 0u, v, (n + 255u) / 256u, s, sc, a, mats, sf, lights, mat0, rays, n, out.f32,
                                 out.rgba8, out.n_rays);
}

hipError_t launch_render_surfaces(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                  const SurfDev* surfs, uint32_t n_surfs, const LightsDev& lights, uint32_t mat0, uint32_t n_samples, const ShadeOut& out,
                                  FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !mats || (n_surfs && !surfs) || lights.n > MAX_LIGHTS) return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    return RR_LAUNCH_TREE_KERNEL(k_render_surfaces, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, mats, sf, lights, mat0, n_samples, fb.blocks_x,
                                 fb.n_blocks, out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
