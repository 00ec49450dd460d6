// rr_render_shutter.hip -- shutter frames (rr_render_shutter[_device]) for gfx950: k_render_composed with the scene as one more
// per-sample table entry.  Sample s of a pixel starts on the lens (or at the pinhole), is traced in the captured scene keys[key[s]]
// (rr_capture_scene_key) and shaded by the nested-media tree under band table band[s], and its colour is weighted per channel with
// that band's weights before it enters the resolve's sum: motion blur as a fold over frozen instants.
//
// The shape is k_render_composed's: a wave is one 8x8 pixel block and a lane one pixel, the lanes loop over the samples, the wave
// reconverges behind each sample's tree; instantiations come from for_tree_variant, occupancy from ShadeWaves, the LDS stacks are
// the same.  In place of a SceneDev by value the kernel takes the context's array of key records.  The sample index is
// wave-uniform, so the key index is (a byte of a kernel-argument word, made provably uniform with readfirstlane), and the record
// behind it has a scalar address: its fields are fetched with scalar loads at the head of every sample, as band_w is.  The tree
// (rr_render_nested.h) takes the scene by reference; what it is given is a per-sample copy of the record whose environment fields
// are the launch's own (key_scene, rr_render_frame.h, shared with k_render_lit) -- a record never carries an environment pointer,
// so that replacing the map after a capture cannot leave a stale one behind.  The frame around the samples is render_frame (there).
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_nested.h"

namespace rr {

// HSA allows a kernel 4 KB of arguments; the two 512-byte tables and the 64 band and 64 key indices take 1152 bytes of it
static_assert(sizeof(SampleKeys) == 64, "SampleKeys: one byte per sample, four to a word");
static_assert(sizeof(DispatchDev) + sizeof(CamDev) + 2 * sizeof(SampleOffsets) + sizeof(LensDev) + sizeof(SampleBands) + sizeof(SampleKeys) +
              7 * sizeof(uint32_t) + 7 * sizeof(void*) + 64 <= 4096, "k_render_shutter: the kernel arguments do not fit the kernarg segment");

// Arguments as k_render_composed, with keys / key in place of sc / mat0 (a.hx0..hy1: the rectangle of the union of the used keys'
// bounds) and the context's environment map beside them.  key: per sample the key it is traced in, a byte each, four to a word.
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_shutter(const KeyDev* __restrict__ keys, DispatchDev a, CamDev cam,
                                                                                             SampleOffsets off, SampleOffsets loff, LensDev lens,
                                                                                             SampleBands band, SampleKeys key, const MatDev* band_mats,
                                                                                             uint32_t n_rows, const float* band_w, const float4* env,
                                                                                             int32_t env_w, int32_t env_h, uint32_t n_samples,
                                                                                             uint32_t blocks_x, uint32_t n_blocks, float4* out_f32,
                                                                                             uint32_t* out_rgba8, uint32_t* out_n)
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
            c = ray_tree_nested<TLAS, E>(sc, a, band_mats + (size_t)b * n_rows, kd->mat0, with_empty_media(r), stk, park, st);
        }
        return weighted(band_w + 3u * b, c);
    });
}

hipError_t launch_render_shutter(const KeyDev* keys, bool single_identity, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off,
                                 const SampleOffsets& loff, const LensDev& lens, const SampleBands& band, const SampleKeys& key,
                                 const MatDev* band_mats, uint32_t n_rows, const float* band_w, const float4* env, int32_t env_w, int32_t env_h,
                                 uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !keys || !band_mats || !band_w || n_rows == 0) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_render_shutter, single_identity, v, fb.groups, s, keys, a, cam, off, loff, lens, band, key, band_mats, n_rows, band_w, env, env_w,
                                 env_h, n_samples, fb.blocks_x, fb.n_blocks, out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
