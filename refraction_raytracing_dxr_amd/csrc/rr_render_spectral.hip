// rr_render_spectral.hip -- spectral frames (rr_render_spectral[_device]) for gfx950: k_render_samples with a band table.  Sample k
// of a pixel is k_render_samples' sample k, shaded with the index of refraction of band k, and its colour is weighted per channel
// before it enters the resolve's sum: distribution ray tracing over the wavelength, which is what puts colour fringes on glass.
//
// The shape is k_render_samples': a wave is one 8x8 pixel block and a lane one pixel, the lanes loop over the samples, the wave
// reconverges behind each sample's tree, and three accumulators are divided by S and stored once.  The sample index is
// wave-uniform, so the band's five words that a sample needs (ior, inv_ior, three weights) come from the kernel arguments with
// scalar loads like the offsets.  shade_ray reads a.ior / a.inv_ior, so the tree of sample k gets a copy of the DispatchDev
// with those two fields replaced: the struct lives in scalar registers, and after SROA only the fields that are read remain.
// Nothing of a band ever exists in memory: no per-band frames, no pass over them.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_common.h"

namespace rr {

// HSA allows a kernel 4 KB of arguments; the offsets take 512 bytes of it and the band table 1280
static_assert(sizeof(BandTable) == 1280, "BandTable: ior[64], inv_ior[64], weight[64][3]");
static_assert(sizeof(SceneDev) + sizeof(DispatchDev) + sizeof(CamDev) + sizeof(SampleOffsets) + sizeof(BandTable) + 3 * sizeof(uint32_t) +
              3 * sizeof(void*) + 64 <= 4096, "k_render_spectral: the kernel arguments do not fit the kernarg segment");

// Arguments as k_render_samples; bands: n_samples rows, row k the index of refraction (and its reciprocal, inv_ior_of on the host)
// that sample k's tree refracts with and the weight of its colour per channel.
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_spectral(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                              BandTable bands, uint32_t n_samples, uint32_t blocks_x,
                                                                                              uint32_t n_blocks, float4* out_f32, uint32_t* out_rgba8,
                                                                                              uint32_t* out_n)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;                           // lanes outside the frame trace nothing and store nothing
    // A block outside the scene's screen rectangle is background for every band: the primary rays are k_render_samples', so its
    // rectangle and margin hold, and a Miss does not look at the index of refraction.  Its samples are weighted like any other.
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
            DispatchDev ab = a;                                 // this sample's band: what shade_ray refracts with
            ab.ior = bands.ior[s]; ab.inv_ior = bands.inv_ior[s];
            RegPark<PEND> park;
            c = ray_tree<TLAS, E>(sc, ab, r, stk, park, st);
        }
        // p_k = weight * c_k, one rounding; the sum starts AT p_0 (0 + p would turn a -0 into +0) and takes the others in their order
        const f3 p = mk3(bands.weight[s][0] * c.x, bands.weight[s][1] * c.y, bands.weight[s][2] * c.z);
        sum = s ? mk3(sum.x + p.x, sum.y + p.y, sum.z + p.z) : p;
    }
    const float fs = (float)n_samples;
    const f3 out = mk3(sum.x / fs, sum.y / fs, sum.z / fs);
    const size_t o = (size_t)y * a.W + x;
    if (out_f32) out_f32[o] = make_float4(out.x, out.y, out.z, 1.0f);
    if (out_rgba8) store_pixel(a, out_rgba8, nullptr, o, out);
    if (out_n) out_n[o] = st.rays;
}

// stack, pend, stack16: a FusedVariant of the scene, through the ray-tree kernels' ladder (for_tree_variant, rr_choice.h)
hipError_t launch_render_spectral(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const BandTable& bands,
                                  uint32_t n_samples, float4* f32, uint32_t* rgba8, uint32_t* n_rays, int stack, int pend, bool stack16,
                                  hipStream_t s)
{
    if (a.W == 0 || a.H == 0 || a.W > 32768u || a.H > 32768u || n_samples == 0 || n_samples > BandTable::MAX) return hipErrorInvalidValue;
    if (stack > 64 || pend > 8) return hipErrorInvalidValue;
    const uint32_t blocks_x = (a.W + 7u) / 8u, n_blocks = blocks_x * ((a.H + 7u) / 8u);         // <= 4096 * 4096
    return for_tree_variant(sc.single_identity != 0u, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_render_spectral<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n_blocks + 3u) / 4u), dim3(256), T::lds_bytes, s, sc,
                           a, cam, off, bands, n_samples, blocks_x, n_blocks, f32, rgba8, n_rays);
        return hipGetLastError();
    });
}

} // namespace rr
