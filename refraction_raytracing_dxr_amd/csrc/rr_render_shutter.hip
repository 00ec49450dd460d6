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
// (rr_render_nested.h) takes the scene by reference and is untouched; what it is given is a per-sample copy of the record whose
// environment fields are the launch's own -- a record never carries an environment pointer, so that replacing the map after a
// capture cannot leave a stale one behind.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
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
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;                           // lanes outside the frame trace nothing and store nothing
    // A block outside the rectangle is background in every key used, for every point of the lens disk
    const bool may_hit = x0 + 8u > a.hx0 && x0 < a.hx1 && y0 + 8u > a.hy0 && y0 < a.hy1;
    const float fx = (float)x, fy = (float)y, fw = (float)a.W, fh = (float)a.H;
    LaneStats st;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < n_samples; ++s) {
        const RayState r = lens.pinhole ? sample_ray(a, cam, off, s, fx, fy, fw, fh) : lens_ray(a, cam, off, loff, lens, s, fx, fy, fw, fh);
        const uint32_t b = (band.w[s >> 2] >> ((s & 3u) * 8u)) & 0xffu;    // wave-uniform: the band's table and weights have scalar addresses
        // wave-uniform and < RR_MAX_SCENE_KEYS (the host checks): the record has a scalar address
        const uint32_t k = __builtin_amdgcn_readfirstlane((key.w[s >> 2] >> ((s & 3u) * 8u)) & 0xffu);
        const KeyDev* __restrict__ const kd = keys + k;
        SceneDev sc = kd->sc;
        sc.blas0.nodes = in_global(sc.blas0.nodes); sc.blas0.tris = in_global(sc.blas0.tris); sc.blas0.nrms = in_global(sc.blas0.nrms);
        sc.pool_nodes = in_global(sc.pool_nodes); sc.pool_tris = in_global(sc.pool_tris); sc.pool_nrms = in_global(sc.pool_nrms);
        sc.insts = in_global(sc.insts);
        sc.env = env; sc.env_w = env_w; sc.env_h = env_h;
        f3 c;
        if (!may_hit) {                                         // payload.color = 0 + 1 * texel (hlsl:57-62, 127-137)
            const f3 e = env_lookup(sc, r.D);
            c = mk3(fmaf(1.0f, e.x, 0.0f), fmaf(1.0f, e.y, 0.0f), fmaf(1.0f, e.z, 0.0f));
            ++st.rays;
        } else {
            RegParkNested<PEND> park;
            c = ray_tree_nested<TLAS, E>(sc, a, band_mats + (size_t)b * n_rows, kd->mat0, with_empty_media(r), stk, park, st);
        }
        // p_k = weight * c_k, one rounding; the sum starts AT p_0 (0 + p would turn a -0 into +0) and takes the others in their order
        const float* const w = band_w + 3u * b;
        const f3 p = mk3(w[0] * c.x, w[1] * c.y, w[2] * c.z);
        sum = s ? mk3(sum.x + p.x, sum.y + p.y, sum.z + p.z) : p;
    }
    const float fs = (float)n_samples;
    const f3 out = mk3(sum.x / fs, sum.y / fs, sum.z / fs);
    const size_t o = (size_t)y * a.W + x;
    if (out_f32) out_f32[o] = make_float4(out.x, out.y, out.z, 1.0f);
    if (out_rgba8) store_pixel(a, out_rgba8, nullptr, o, out);
    if (out_n) out_n[o] = st.rays;
}

// stack, pend, stack16: a FusedVariant valid for every key used, through the ray-tree kernels' ladder (for_tree_variant, rr_choice.h)
hipError_t launch_render_shutter(const KeyDev* keys, bool single_identity, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off,
                                 const SampleOffsets& loff, const LensDev& lens, const SampleBands& band, const SampleKeys& key,
                                 const MatDev* band_mats, uint32_t n_rows, const float* band_w, const float4* env, int32_t env_w, int32_t env_h,
                                 uint32_t n_samples, float4* f32, uint32_t* rgba8, uint32_t* n_rays, int stack, int pend, bool stack16,
                                 hipStream_t s)
{
    if (a.W == 0 || a.H == 0 || a.W > 32768u || a.H > 32768u || n_samples == 0 || n_samples > SampleOffsets::MAX) return hipErrorInvalidValue;
    if (stack > 64 || pend > 8 || !keys || !band_mats || !band_w || n_rows == 0) return hipErrorInvalidValue;
    const uint32_t blocks_x = (a.W + 7u) / 8u, n_blocks = blocks_x * ((a.H + 7u) / 8u);         // <= 4096 * 4096
    return for_tree_variant(single_identity, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_render_shutter<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n_blocks + 3u) / 4u), dim3(256), T::lds_bytes, s, keys,
                           a, cam, off, loff, lens, band, key, band_mats, n_rows, band_w, env, env_w, env_h, n_samples, blocks_x, n_blocks, f32, rgba8,
                           n_rays);
        return hipGetLastError();
    });
}

} // namespace rr
