// rr_render_materials.hip -- per-instance glass (rr_shade_rays_materials[_device], rr_render_materials[_device]) for gfx950:
// k_shade_rays and k_render_samples over the ray tree of rr_render_materials.h, in which the hit instance's hit-group index selects
// a row of the context's material table -- an index of refraction and an absorption coefficient per colour channel -- and the path
// weight is RGB.
//
// The shapes are the scalar kernels': a wave is 64 consecutive caller rays, or one 8x8 pixel block whose lanes loop over the
// samples and reconverge behind each sample's tree; instantiations come from for_tree_variant and occupancy from ShadeWaves.  The
// table lives in device memory (rows of 32 bytes): which instance a lane hits differs per lane, so a row comes through vector loads,
// { ior, inv_ior } at every ClosestHit and the three sigmas only for a ray that arrives from inside.  A scene that skips the top
// level has one instance, whose index travels as a kernel argument.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_materials.h"

namespace rr {

// k_shade_rays' arguments, then the table and the index of instance 0 (read only by the builds without a top level)
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays_mat(SceneDev sc, DispatchDev a, const MatDev* mats, uint32_t mat0,
                                                                                             const rr_ray_dev* rays, uint32_t n, float4* out_f32,
                                                                                             uint32_t* out_rgba8, uint32_t* out_n)
{
    shade_caller_ray<STACK, E>(a, rays, n, out_f32, out_rgba8, out_n, [&](const RayState& r, E* stk, LaneStats& st) {
        RegParkMat<PEND> park;
        return ray_tree_mat<TLAS, E>(sc, a, mats, mat0, with_rgb_weight(r), stk, park, st);
    });
}

// k_render_samples' arguments, then the table and the index of instance 0
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_materials(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                               const MatDev* mats, uint32_t mat0, uint32_t n_samples,
                                                                                               uint32_t blocks_x, uint32_t n_blocks, float4* out_f32,
                                                                                               uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        if (!may_hit) return culled_sample(sc, r.D, st);
        RegParkMat<PEND> park;
        return ray_tree_mat<TLAS, E>(sc, a, mats, mat0, with_rgb_weight(r), stk, park, st);
    });
}

hipError_t launch_shade_rays_mat(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, uint32_t mat0, const rr_ray_dev* rays, uint32_t n,
                                 const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (v.stack > 64 || v.pend > 8 || !mats) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_shade_rays_mat, sc.single_identity != 0u, v, (n + 255u) / 256u, s, sc, a, mats, mat0, rays, n, out.f32, out.rgba8, out.n_rays);
}

hipError_t launch_render_materials(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                   uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !mats) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_render_materials, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, mats, mat0, n_samples, fb.blocks_x, fb.n_blocks,
                                 out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
