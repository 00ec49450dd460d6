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
#include "rr_render_common.h"

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
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;                           // lanes outside the frame trace nothing and store nothing
    // A block outside the lens rectangle is background for every point of the lens disk (rr_host_lens_screen_rect: the union over
    // the disk's bounding square, each with k_render_samples' margin): every sample is RayGen and one Miss on its own direction.
    const bool may_hit = x0 + 8u > a.hx0 && x0 < a.hx1 && y0 + 8u > a.hy0 && y0 < a.hy1;
    const float fx = (float)x, fy = (float)y, fw = (float)a.W, fh = (float)a.H;
    LaneStats st;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < n_samples; ++s) {
        const RayState r = lens.pinhole ? sample_ray(a, cam, off, s, fx, fy, fw, fh) : lens_ray(a, cam, off, loff, lens, s, fx, fy, fw, fh);
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
hipError_t launch_render_lens(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const SampleOffsets& loff,
                              const LensDev& lens, uint32_t n_samples, float4* f32, uint32_t* rgba8, uint32_t* n_rays, int stack, int pend,
                              bool stack16, hipStream_t s)
{
    if (a.W == 0 || a.H == 0 || a.W > 32768u || a.H > 32768u || n_samples == 0 || n_samples > SampleOffsets::MAX) return hipErrorInvalidValue;
    if (stack > 64 || pend > 8) return hipErrorInvalidValue;
    const uint32_t blocks_x = (a.W + 7u) / 8u, n_blocks = blocks_x * ((a.H + 7u) / 8u);         // <= 4096 * 4096
    return for_tree_variant(sc.single_identity != 0u, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_render_lens<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n_blocks + 3u) / 4u), dim3(256), T::lds_bytes, s, sc, a,
                           cam, off, loff, lens, n_samples, blocks_x, n_blocks, f32, rgba8, n_rays);
        return hipGetLastError();
    });
}

} // namespace rr
