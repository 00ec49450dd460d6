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
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_common.h"

namespace rr {

// a: what shade_ray and store_pixel read, the frame size (W, H), the primary interval (tmin_p, tmax_p) and the scene's screen
// rectangle (hx0..hy1); cam: the frame's constants; off: n_samples offsets in pixel units.  Outputs are W * H rasters, each
// written only if its pointer is given (wave-uniform branches on kernel arguments).
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_samples(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                             uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                             float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;                           // lanes outside the frame trace nothing and store nothing
    // A block outside the scene's screen rectangle is background: every sample is RayGen and one Miss on its own direction,
    // without TraceRay (k_render_fused's branch).  The rectangle (rr_host_screen_rect) holds the projection of the scene's box
    // in pixel-centre coordinates plus 8 pixels of margin, of which a quarter pays for the fp32 error of the ray directions;
    // a sample position lies inside its pixel, at most half a pixel from the centre, so a block that does not touch the
    // rectangle keeps every sample more than five pixels away from anything a ray could hit.
    const bool may_hit = x0 + 8u > a.hx0 && x0 < a.hx1 && y0 + 8u > a.hy0 && y0 < a.hy1;
    const float fx = (float)x, fy = (float)y, fw = (float)a.W, fh = (float)a.H;
    LaneStats st;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < n_samples; ++s) {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);      // (rr_render_common.h)
        f3 c;
        if (!may_hit) {                                         // payload.color = 0 + 1 * texel (hlsl:57-62, 127-137)
            const f3 e = env_lookup(sc, r.D);
            c = mk3(fmaf(1.0f, e.x, 0.0f), fmaf(1.0f, e.y, 0.0f), fmaf(1.0f, e.z, 0.0f));
            ++st.rays;
        } else {
            RegPark<PEND> park;
            c = ray_tree<TLAS, E>(sc, a, r, stk, park, st);
        }
        // the resolve's sum starts AT sample 0 (0 + c would turn a -0 into +0) and takes the others in their order
        sum = s ? mk3(sum.x + c.x, sum.y + c.y, sum.z + c.z) : c;
    }
    const float fs = (float)n_samples;
    const f3 out = mk3(sum.x / fs, sum.y / fs, sum.z / fs);
    const size_t o = (size_t)y * a.W + x;
    if (out_f32) out_f32[o] = make_float4(out.x, out.y, out.z, 1.0f);
    if (out_rgba8) store_pixel(a, out_rgba8, nullptr, o, out);
    if (out_n) out_n[o] = st.rays;
}

// stack, pend, stack16: a FusedVariant of the scene, through the ray-tree kernels' ladder (for_tree_variant, rr_choice.h)
hipError_t launch_render_samples(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, uint32_t n_samples,
                                 float4* f32, uint32_t* rgba8, uint32_t* n_rays, int stack, int pend, bool stack16, hipStream_t s)
{
    if (a.W == 0 || a.H == 0 || a.W > 32768u || a.H > 32768u || n_samples == 0 || n_samples > SampleOffsets::MAX) return hipErrorInvalidValue;
    if (stack > 64 || pend > 8) return hipErrorInvalidValue;
    const uint32_t blocks_x = (a.W + 7u) / 8u, n_blocks = blocks_x * ((a.H + 7u) / 8u);         // <= 4096 * 4096
    return for_tree_variant(sc.single_identity != 0u, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_render_samples<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n_blocks + 3u) / 4u), dim3(256), T::lds_bytes, s, sc, a,
                           cam, off, n_samples, blocks_x, n_blocks, f32, rgba8, n_rays);
        return hipGetLastError();
    });
}

} // namespace rr
