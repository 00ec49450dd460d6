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
#include "rr_render_frame.h"

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
    render_frame<STACK, E>(a, n_samples, blocks_x, n_blocks, out_f32, out_rgba8, out_n,
                           [&](uint32_t s, float fx, float fy, float fw, float fh, bool may_hit, E* stk, LaneStats& st) {
        const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        f3 c;
        if (!may_hit) {                                         // a Miss does not look at the index of refraction
            c = culled_sample(sc, r.D, st);
        } else {
            DispatchDev ab = a;                                 // this sample's band: what shade_ray refracts with
            ab.ior = bands.ior[s]; ab.inv_ior = bands.inv_ior[s];
            RegPark<PEND> park;
            c = ray_tree<TLAS, E>(sc, ab, r, stk, park, st);
        }
        return weighted(bands.weight[s], c);
    });
}

hipError_t launch_render_spectral(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const BandTable& bands,
                                  uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_samples, v, fb)) return hipErrorInvalidValue;
    return RR_LAUNCH_TREE_KERNEL(k_render_spectral, sc.single_identity != 0u, v, fb.groups, s, sc, a, cam, off, bands, n_samples, fb.blocks_x, fb.n_blocks,
                                 out.f32, out.rgba8, out.n_rays);
}

} // namespace rr
