// rr_render_surfaces.hip -- opaque hit groups (rr_shade_rays_surfaces[_device], rr_render_surfaces[_device]) for gfx950:
// k_shade_rays_nested and k_render_nested over the ray tree of rr_render_surfaces.h, in which an instance whose row of the surface
// table is opaque is lit by the context's lights through shadow rays, emits, and may continue as a mirror.
//
// The shapes are the nested kernels': a wave is 64 consecutive caller rays, or one 8x8 pixel block whose lanes loop over the samples;
// instantiations come from for_tree_variant and occupancy from ShadeWaves; the LDS stacks are the same, and the shadow rays walk on
// them.  The surface table is read like the material table, per lane through vector loads.  The lights and the ambient term are the
// same for every lane and travel by value as a kernel argument (LightsDev, 8 x 32 + 16 bytes).
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_surfaces.h"

namespace rr {

// k_shade_rays_nested's arguments, the surface table and the lights
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_shade_rays_surfaces(SceneDev sc, DispatchDev a, const MatDev* mats, SurfArgs sf,
                                                                                                  LightsDev lights, uint32_t mat0, const rr_ray_dev* rays,
                                                                                                  uint32_t n, float4* out_f32, uint32_t* out_rgba8,
                                                                                                  uint32_t* out_n)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(rays + i);
    const uint4 o = q[0], d = q[1];                             // (q[2]: flags, instance_mask, pad -- the tree's TraceRay calls fix them)
    RayStateNested r;
    r.O = mk3(__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z));
    r.D = mk3(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    r.tmin = __uint_as_float(o.w); r.tmax = __uint_as_float(d.w);
    r.w = mk3(1.0f, 1.0f, 1.0f); r.count = 0; r.media = 0u;     // RayGen's payload, the weight per channel; the ray starts in air
    LaneStats st;
    RegParkNested<PEND> park;
    const f3 acc = ray_tree_surfaces<TLAS, E>(sc, a, mats, sf, lights, mat0, r, stk, park, st);
    if (out_f32) out_f32[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
    if (out_rgba8) store_pixel(a, out_rgba8, nullptr, i, acc);
    if (out_n) out_n[i] = st.rays;
}

// k_render_nested's arguments, the surface table and the lights
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_render_surfaces(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                              const MatDev* mats, SurfArgs sf, LightsDev lights, uint32_t mat0,
                                                                                              uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks,
                                                                                              float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;                           // lanes outside the frame trace nothing and store nothing
    // A block outside the scene's screen rectangle is background whatever the surfaces: its primary rays are a Miss, which looks at
    // no table and no light.
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
            RegParkNested<PEND> park;
            c = ray_tree_surfaces<TLAS, E>(sc, a, mats, sf, lights, mat0, with_empty_media(r), stk, park, st);
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
hipError_t launch_shade_rays_surfaces(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, const SurfDev* surfs, uint32_t n_surfs,
                                      const LightsDev& lights, uint32_t mat0, const rr_ray_dev* rays, uint32_t n, float4* f32, uint32_t* rgba8,
                                      uint32_t* n_rays, int stack, int pend, bool stack16, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (stack > 64 || pend > 8 || !mats || (n_surfs && !surfs) || lights.n > MAX_LIGHTS) return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    return for_tree_variant(sc.single_identity != 0u, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_shade_rays_surfaces<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n + 255u) / 256u), dim3(256), T::lds_bytes, s, sc,
                           a, mats, sf, lights, mat0, rays, n, f32, rgba8, n_rays);
        return hipGetLastError();
    });
}

hipError_t launch_render_surfaces(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                  const SurfDev* surfs, uint32_t n_surfs, const LightsDev& lights, uint32_t mat0, uint32_t n_samples, float4* f32,
                                  uint32_t* rgba8, uint32_t* n_rays, int stack, int pend, bool stack16, hipStream_t s)
{
    if (a.W == 0 || a.H == 0 || a.W > 32768u || a.H > 32768u || n_samples == 0 || n_samples > SampleOffsets::MAX) return hipErrorInvalidValue;
    if (stack > 64 || pend > 8 || !mats || (n_surfs && !surfs) || lights.n > MAX_LIGHTS) return hipErrorInvalidValue;
    const SurfArgs sf = { surfs, n_surfs };
    const uint32_t blocks_x = (a.W + 7u) / 8u, n_blocks = blocks_x * ((a.H + 7u) / 8u);         // <= 4096 * 4096
    return for_tree_variant(sc.single_identity != 0u, FusedVariant{ stack, pend, stack16 }, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_render_surfaces<T::stack, T::pend, T::tlas, typename T::entry>), dim3((n_blocks + 3u) / 4u), dim3(256), T::lds_bytes, s, sc, a,
                           cam, off, mats, sf, lights, mat0, n_samples, blocks_x, n_blocks, f32, rgba8, n_rays);
        return hipGetLastError();
    });
}

} // namespace rr
