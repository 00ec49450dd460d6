// rr_render_lens.hip -- thin-lens frames (rr_render_lens[_device]) for gfx950: k_render_samples with a lens of finite aperture in
// front of it.  Sample s of a pixel starts at lens offset s of a second table, on the disk camera_loc + lx * A + ly * B, and heads
// for the point of the focal plane its sub-pixel position sees through the pinhole; what lies in that plane is sharp, the rest is
// averaged over the aperture.
//
// The shape is k_render_samples': a wave is one 8x8 pixel block and a lane one pixel, the lanes loop over the samples, the wave
// reconverges behind each sample's tree and the colours are accumulated in registers and stored once.  The sample index is
// wave-uniform, so both offset tables and the lens are read from the kernel arguments with scalar loads; the lens vectors off and
// T die when the ray exists, so a traversal carries what k_render_samples' carries.  What the aperture costs is coherence: the
// 64 rays of a wave still belong to one sample, but they start on one lens point and fan out from there.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"

namespace rr {

// HSA allows a kernel 4 KB of arguments; the two 512-byte tables take a quarter of it
static_assert(sizeof(SceneDev) + sizeof(DispatchDev) + sizeof(CamDev) + 2 * sizeof(SampleOffsets) + sizeof(LensDev) + 3 * sizeof(uint32_t) +
              3 * sizeof(void*) + 64 <= 4096, "k_render_lens: the kernel arguments do not fit the kernarg segment");

// Arguments as k_render_samples; loff: n_samples lens offsets in units of the radius; lens: A, B, s (lens.pinhole: the rays are
// sample_ray's, the kernel is k_render_samples).  a.hx0..hy1: the rectangle of rr_host_lens_screen_rect.
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_lens(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                          SampleOffsets loff, LensDev lens, uint32_t n_samples,
                                                                                          uint32_t blocks_x, uint32_t n_blocks, float4* out_f32,
                                                                                          uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = lens_or_pinhole_ray(a, cam, off, loff, lens, s, fx, fy, fw, fh);
        if (!may_hit) return culled_sample(sc, r.D, st);
        RegPark<PEND> park;
        return ray_tree<TLAS, E>(sc, a, r, stk, park, st);
    });
}

hipError_t launch_render_lens(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const SampleOffsets& loff,
                              const LensDev& lens, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb)) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_render_lens, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, loff, lens, n_samples, fb.blocks_x, fb.n_blocks,
                                 out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
