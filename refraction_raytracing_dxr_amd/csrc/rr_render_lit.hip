// rr_render_lit.hip -- lit shutter frames (rr_render_lit[_device]) for gfx950: k_render_shutter's frame over ray_tree_surfaces' hit
// groups, with the lights as one more per-sample table entry.  Sample s of a pixel starts on the lens (or at the pinhole), is traced
// in the captured scene keys[key[s]] and shaded by the surface tree under band table band[s] with every light moved over its shape to
// the sample's light offset (rr_render_lit.h); its colour is weighted per channel with that band's weights before it enters the
// resolve's sum.  The fold that integrates the aperture and the shutter integrates the lights' areas too: soft shadows.
//
// The shape is k_render_shutter's: a wave is one 8x8 pixel block and a lane one pixel, the lanes loop over the samples, the wave
// reconverges behind each sample's tree; instantiations come from for_tree_variant, occupancy from ShadeWaves, the LDS stacks are
// the same and the shadow rays walk on them.  The frame is render_frame and the key record's fetch key_scene (rr_render_frame.h):
// scalar loads at the head of every sample, the pointers through in_global, the environment the launch's own.  The light offsets are one more 512-byte table in the
// kernel-argument segment, read like the sub-pixel positions at a wave-uniform index; the lights and their shapes travel by value.
// k_render_lit_shadows is the twin for transparent shadows (rr_set_shadow_steps): the same body over the tree's WALK form
// (rr_render_shadows.h), with the cap shadow_k as one more argument; the launcher picks it where the cap is not 0.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_lit.h"
#include "rr_render_shadows.h"

namespace rr {

// HSA allows a kernel 4 KB of arguments; the three 512-byte tables, the 64 band and 64 key indices, the lights and their shapes take
// 2144 bytes of k_render_lit's, and k_render_lit_shadows' cap is one more word
static_assert(sizeof(DispatchDev) + sizeof(CamDev) + 3 * sizeof(SampleOffsets) + sizeof(LensDev) + sizeof(SampleBands) + sizeof(SampleKeys) +
              sizeof(SurfArgs) + sizeof(LightsDev) + sizeof(LightShapesDev) + 8 * sizeof(uint32_t) + 7 * sizeof(void*) + 96 <= 4096,
              "k_render_lit_shadows: the kernel arguments do not fit the kernarg segment");

// What the two kernels hand to render_frame: one written closure.  WALK: the tree's form; shadow_k is read by that form only.  The
// members are references to the kernel's arguments, as a lambda's captures are (rr_render_surfaces.hip says why)
template <int PEND, bool TLAS, class E, bool WALK>
struct LitSample {
    const KeyDev* __restrict__ const& keys; const DispatchDev& a; const CamDev& cam; const SampleOffsets& off; const SampleOffsets& loff;
    const SampleOffsets& lgt; const LensDev& lens; const SampleBands& band; const SampleKeys& key; const MatDev* const& band_mats;
    const uint32_t& n_rows; const float* const& band_w; const SurfArgs& sf; const LightsDev& lights; const LightShapesDev& shapes;
    uint32_t shadow_k; const float4* const& env; const int32_t& env_w; const int32_t& env_h;
    __device__ __forceinline__ f3 operator()(uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) const
    {
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
            c = ray_tree_lit<TLAS, E, WALK>(sc, a, band_mats + (size_t)b * n_rows, sf, lights, shapes, lgt.v[2u * s], lgt.v[2u * s + 1u], kd->mat0,
                                            with_empty_media(r), stk, park, st, shadow_k);
        }
        return weighted(band_w + 3u * b, c);
    }
};

// Arguments as k_render_shutter, with the surface table, the lights, their shapes and the samples' light offsets (lgt.v[2s], [2s+1])
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_lit(const KeyDev* __restrict__ keys, DispatchDev a, CamDev cam,
                                                                                         SampleOffsets off, SampleOffsets loff, SampleOffsets lgt,
                                                                                         LensDev lens, SampleBands band, SampleKeys key,
                                                                                         const MatDev* band_mats, uint32_t n_rows, const float* band_w,
                                                                                         SurfArgs sf, LightsDev lights, LightShapesDev shapes,
                                                                                         const float4* env, int32_t env_w, int32_t env_h,
                                                                                         uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                         float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           LitSample<PEND, TLAS, E, false>{ keys, a, cam, off, loff, lgt, lens, band, key, band_mats, n_rows, band_w, sf, lights, shapes, 0u, env,
                                                            env_w, env_h });
}

// k_render_lit's arguments and the cap
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
                           LitSample<PEND, TLAS, E, true>{ keys, a, cam, off, loff, lgt, lens, band, key, band_mats, n_rows, band_w, sf, lights, shapes,
                                                           shadow_k, env, env_w, env_h });
}

hipError_t launch_render_lit(const KeyDev* keys, bool single_identity, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off,
                             const SampleOffsets& loff, const SampleOffsets& lgt, const LensDev& lens, const SampleBands& band, const SampleKeys& key,
                             const MatDev* band_mats, uint32_t n_rows, const float* band_w, const SurfaceLaunch& su, const LightShapesDev& shapes,
                             const float4* env, int32_t env_w, int32_t env_h, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !keys || !band_w || n_rows == 0 || !su.ok(band_mats)) return hipErrorInvalidValue;
    const SurfArgs sf = { su.surfs, su.n_surfs };
    if (su.shadow_k)
        return RR_LAUNCH_TREE_KERNEL(k_render_lit_shadows, single_identity, v, fb.groups, s, keys, a, cam, off, loff, lgt, lens, band, key, band_mats, n_rows,
                                     band_w, sf, *su.lights, shapes, su.shadow_k, env, env_w, env_h, n_samples, fb.blocks_x, fb.n_blocks, out.f32, out.rgba8,
                                     out.n_rays);
    return RR_LAUNCH_TREE_KERNEL(k_render_lit, single_identity, v, fb.groups, s, keys, a, cam, off, loff, lgt, lens, band, key, band_mats, n_rows, band_w, sf,
                                 *su.lights, shapes, env, env_w, env_h, n_samples, fb.blocks_x, fb.n_blocks, out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
