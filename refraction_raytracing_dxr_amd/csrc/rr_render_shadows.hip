// rr_render_shadows.hip -- transparent shadows (rr_set_shadow_steps) for gfx950: k_shade_rays_surfaces, k_render_surfaces and
// k_render_lit over the ray tree of rr_render_shadows.h, in which the shadow ray of an opaque hit walks through the glass between
// the hit and the light, takes its tint and is stopped only by an opaque surface.
//
// The shapes, the arguments and the occupancy are the twins': a wave is 64 consecutive caller rays, or one 8x8 pixel block whose
// lanes loop over the samples; instantiations come from for_tree_variant and waves per SIMD from ShadeWaves; the LDS stacks are the
// same and the walks use them.  One argument is new: shadow_k, the cap on a walk's TraceRay calls (1 .. SHADOW_MAX_STEPS), the same
// for every lane, so the walk's loop has a scalar bound.  The launchers here are reached only with shadow_k >= 1: with the setting
// at 0 the host launches the twins (rr_render_surfaces.hip, rr_render_lit.hip), which this file does not touch.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_shadows.h"

namespace rr {

// k_shade_rays_surfaces' arguments and the cap
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays_shadows(SceneDev sc, DispatchDev a, const MatDev* mats, SurfArgs sf,
                                                                                                 LightsDev lights, uint32_t shadow_k, uint32_t mat0,
                                                                                                 const rr_ray_dev* rays, uint32_t n, float4* out_f32,
                                                                                                 uint32_t* out_rgba8, uint32_t* out_n)
{
    shade_caller_ray<STACK, E>(a, rays, n, out_f32, out_rgba8, out_n, [&](const RayState& r, E* stk, LaneStats& st) {
        RegParkNested<PEND> park;
        return ray_tree_surfaces_transmit<TLAS, E>(sc, a, mats, sf, lights, [&](uint32_t i) -> const LightDev& { return lights.l[i]; }, shadow_k, mat0,
                                                   with_empty_media(r), stk, park, st);
    });
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
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        if (!may_hit) return culled_sample(sc, r.D, st);
        RegParkNested<PEND> park;
        return ray_tree_surfaces_transmit<TLAS, E>(sc, a, mats, sf, lights, [&](uint32_t i) -> const LightDev& { return lights.l[i]; }, shadow_k, mat0,
                                                   with_empty_media(r), stk, park, st);
    });
}

// the cap is one more word beside k_render_lit's 2144 bytes of arguments
static_assert(sizeof(DispatchDev) + sizeof(CamDev) + 3 * sizeof(SampleOffsets) + sizeof(LensDev) + sizeof(SampleBands) + sizeof(SampleKeys) +
              sizeof(SurfArgs) + sizeof(LightsDev) + sizeof(LightShapesDev) + 8 * sizeof(uint32_t) + 7 * sizeof(void*) + 96 <= 4096,
              "k_render_lit_shadows: the kernel arguments do not fit the kernarg segment");

// k_render_lit's arguments and the cap: every walk goes towards the light as moved for its sample, so a shaped light's soft shadow
// takes the glass's colour
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_lit_shadows(const KeyDev* __restrict__ keys, DispatchDev a, CamDev cam,
                                                                                                 SampleOffsets off, SampleOffsets loff, SampleOffsets lgt,
                                                                                                 LensDev lens, SampleBands band, SampleKeys key,
                                                                                                 const MatDev* band_mats, uint32_t n_rows, const float* band_w,
                                                                                                 SurfArgs sf, LightsDev lights, LightShapesDev shapes,
                                                                                                 uint32_t shadow_k, const float4* env, int32_t env_w,
                                                                                                 int32_t env_h, uint32_t n_samples, uint32_t blocks_x,
                                                                                                 uint32_t n_blocks, float4* out_f32, uint32_t* out_rgba8,
                                                                                                 uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = lens_or_pinhole_ray(a, cam, off, loff, lens, s, fx, fy, fw, fh);
        const uint32_t b = sample_byte(band, s);                // the band's table and weights have scalar addresses
        // < RR_MAX_SCENE_KEYS (the host checks), and provably wave-uniform: the record has a scalar address
        const KeyDev* __restrict__ const kd = keys + __builtin_amdgcn_readfirstlane(sample_byte(key, s));
        const SceneDev sc = key_scene(kd, env, env_w, env_h);
        f3 c;
        if (!may_hit) {
            c = culled_sample(sc, r.D, st);
        } else {
            RegParkNested<PEND> park;
            const float lu = lgt.v[2u * s], lv = lgt.v[2u * s + 1u];
            c = ray_tree_surfaces_transmit<TLAS, E>(sc, a, band_mats + (size_t)b * n_rows, sf, lights,
                                                    [&](uint32_t i) { return moved_light(lights, shapes, i, lu, lv); }, shadow_k, kd->mat0,
                                                    with_empty_media(r), stk, park, st);
        }
        return weighted(band_w + 3u * b, c);
    });
}

hipError_t launch_shade_rays_shadows(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, const SurfDev* surfs, uint32_t n_surfs,
                                     const LightsDev& lights, uint32_t shadow_k, uint32_t mat0, const rr_ray_dev* rays, uint32_t n, const ShadeOut& out,
                                     FusedVariant v, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (v.stack > 64 || v.pend > 8 || !mats || (n_surfs && !surfs) || lights.n > MAX_LIGHTS || shadow_k == 0 || shadow_k > SHADOW_MAX_STEPS)
        return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    return RR_LAUNCH_TREE_KERNEL(k_shade_rays_shadows, sc.single_identity != 0u, v, (n + 255u) / 256u, s, sc, a, mats, sf, lights, shadow_k, mat0, rays, n,
                                 out.f32, out.rgba8, out.n_rays);
}

hipError_t launch_render_shadows(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                 const SurfDev* surfs, uint32_t n_surfs, const LightsDev& lights, uint32_t shadow_k, uint32_t mat0, uint32_t n_samples,
                                 const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !mats || (n_surfs && !surfs) || lights.n > MAX_LIGHTS || shadow_k == 0 || shadow_k > SHADOW_MAX_STEPS)
        return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    return RR_LAUNCH_TREE_KERNEL(k_render_shadows, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, mats, sf, lights, shadow_k, mat0, n_samples,
                                 fb.blocks_x, fb.n_blocks, out.f32, out.rgba8, out.n_rays);
}

hipError_t launch_render_lit_shadows(const KeyDev* keys, bool single_identity, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off,
                                     const SampleOffsets& loff, const SampleOffsets& lgt, const LensDev& lens, const SampleBands& band,
                                     const SampleKeys& key, const MatDev* band_mats, uint32_t n_rows, const float* band_w, const SurfDev* surfs,
                                     uint32_t n_surfs, const LightsDev& lights, const LightShapesDev& shapes, uint32_t shadow_k, const float4* env,
                                     int32_t env_w, int32_t env_h, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !keys || !band_mats || !band_w || n_rows == 0 || (n_surfs && !surfs) || lights.n > MAX_LIGHTS ||
        shadow_k == 0 || shadow_k > SHADOW_MAX_STEPS)
        return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    return RR_LAUNCH_TREE_KERNEL(k_render_lit_shadows, single_identity, v, fb.groups, s, keys, a, cam, off, loff, lgt, lens, band, key, band_mats, n_rows,
                                 band_w, sf, lights, shapes, shadow_k, env, env_w, env_h, n_samples, fb.blocks_x, fb.n_blocks, out.f32, out.rgba8,
                                 out.n_rays);
}

} // namespace rr
