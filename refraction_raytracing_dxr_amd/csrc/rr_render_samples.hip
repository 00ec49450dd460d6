// rr_render_samples.hip -- supersampled frames (rr_render_samples[_device]) for gfx950: S primary rays per pixel through S
// sub-pixel positions, each with the shader's whole ray tree, resolved in the kernel into one colour per pixel.
//
// A wave is one 8x8 pixel block and a lane one pixel, as in k_render_fused; a workgroup is four blocks next to each other in a
// row of blocks.  Every lane loops over the samples: sample s of its pixel is GenerateCameraRay with (0.5, 0.5) replaced by
// offset s, then ray_tree (rr_render_common.h: the loop k_shade_rays runs on a caller's ray), and its colour goes into three
// accumulators that are divided by S and stored once at the end.  The wave reconverges behind each sample's tree, so its 64
// lanes always trace the SAME sample of neighbouring pixels -- the coherence of a render kernel's wave, which a batch of caller
// rays has only if the caller orders it so -- and nothing of a sample ever exists in memory: no ray records, no per-sample
// colours.  The offsets arrive as kernel arguments and are read with scalar loads (the sample index is wave-uniform).
//
// That frame -- block, pixel, cull rectangle, sample loop, fold, stores -- is render_frame (rr_render_frame.h), which the eight frame
// kernels modelled on this one share; a kernel's own text is what a sample is.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_frame.h"

namespace rr {

// a: what shade_ray and store_pixel read, the frame size (W, H), the primary interval (tmin_p, tmax_p) and the scene's screen
// rectangle (hx0..hy1); cam: the frame's constants; off: n_samples offsets in pixel units.  Outputs are W * H rasters, each
// written only if its pointer is given (wave-uniform branches on kernel arguments).
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_samples(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                             uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                             float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        if (!may_hit) return culled_sample(sc, r.D, st);
        RegPark<PEND> park;
        return ray_tree<TLAS, E>(sc, a, r, stk, park, st);
    });
}

hipError_t launch_render_samples(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, uint32_t n_samples,
                                 const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb)) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_render_samples, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, n_samples, fb.blocks_x, fb.n_blocks, out.f32,
                                 out.rgba8, out.n_rays);
}

} // namespace rr
