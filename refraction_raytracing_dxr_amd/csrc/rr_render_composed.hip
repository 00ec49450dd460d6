// rr_render_composed.hip -- composed frames (rr_render_composed[_device]) for gfx950: k_render_nested with k_render_lens' primary
// rays in front of the tree and k_render_spectral's weighted resolve behind it.  Sample s of a pixel starts on the lens (or at the
// pinhole), is shaded by the nested-media tree under band table band[s] of the context's band set (rr_set_material_bands), and
// its colour is weighted per channel with that band's weights before it enters the resolve's sum.
//
// The shape is k_render_nested's: a wave is one 8x8 pixel block and a lane one pixel, the lanes loop over the samples, the wave
// reconverges behind each sample's tree; instantiations come from for_tree_variant, occupancy from ShadeWaves, the LDS stacks are
// the same.  The sample index is wave-uniform, so the offsets, the lens and the sample's band index come from the kernel
// arguments with scalar loads; a band of a material table is just another table, band_mats + band[s] * n_rows, a scalar base the
// tree's vector loads index as they index the table of k_render_nested.  The band's three weights sit in device memory behind a
// wave-uniform address.  The frame is render_frame (rr_render_frame.h), the tree
// rr_render_nested.h's as it stands.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"
#include "rr_render_nested.h"

namespace rr {

// HSA allows a kernel 4 KB of arguments; the two 512-byte tables and the 64 band indices take 1088 bytes of it
static_assert(sizeof(SampleBands) == 64, "SampleBands: one byte per sample, four to a word");
static_assert(sizeof(SceneDev) + sizeof(DispatchDev) + sizeof(CamDev) + 2 * sizeof(SampleOffsets) + sizeof(LensDev) + sizeof(SampleBands) +
              6 * sizeof(uint32_t) + 5 * sizeof(void*) + 64 <= 4096, "k_render_composed: the kernel arguments do not fit the kernarg segment");

// Arguments as k_render_lens (off, loff, lens; a.hx0..hy1: the lens rectangle, or the pinhole's when lens.pinhole) and
// k_render_nested (mat0).  band: per sample the band it is shaded in, a byte each, four to a word (a scalar load fetches a word);
// band_mats: the bands' tables, n_rows rows each, one behind the other; band_w: three weights per band.
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_composed(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                              SampleOffsets loff, LensDev lens, SampleBands band,
                                                                                              const MatDev* band_mats, uint32_t n_rows,
                                                                                              const float* band_w, uint32_t mat0,
                                                                                              uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                              float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = lens_or_pinhole_ray(a, cam, off, loff, lens, s, fx, fy, fw, fh);
        const uint32_t b = sample_byte(band, s);                // the band's table and weights have scalar addresses
        f3 c;
        if (!may_hit) {
            c = culled_sample(sc, r.D, st);
        } else {
            RegParkNested<PEND> park;
            c = ray_tree_nested<TLAS, E>(sc, a, band_mats + (size_t)b * n_rows, mat0, with_empty_media(r), stk, park, st);
        }
        return weighted(band_w + 3u * b, c);
    });
}

hipError_t launch_render_composed(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const SampleOffsets& loff,
                                  const LensDev& lens, const SampleBands& band, const MatDev* band_mats, uint32_t n_rows, const float* band_w,
                                  uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb) || !band_mats || !band_w || n_rows == 0) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_render_composed, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, loff, lens, band, band_mats, n_rows, band_w, mat0,
                                 n_samples, fb.blocks_x, fb.n_blocks, out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
