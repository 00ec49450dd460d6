// rr_render_frame.h -- what the ray-tree kernels share around their trees: the frame of the nine supersampling kernels
// (k_render_samples, _lens, _spectral, _materials, _nested, _surfaces, _composed, _shutter, _lit), the shell of the four caller-ray
// kernels (k_shade_rays, _mat, _nested, _surfaces), and the pieces of a sample that more than one kernel needs.  A kernel keeps its
// name, its arguments and its launch bounds, and says only what is its own: how a sample's primary ray is made, which tree walks it
// under which tables, and whether its colour is weighted.  Everything here is inlined into the kernel; nothing of it is a call.
#pragma once
#include "rr_render_common.h"

namespace rr {

// this lane's column of its wave's traversal stack: a workgroup's four stacks are its dynamic LDS
template <int STACK, class E> __device__ __forceinline__ E* lane_stack(uint32_t wave, uint32_t lane)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    return reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
}

// A sample of a culled block: RayGen and one Miss on its own direction, without TraceRay -- payload.color = 0 + 1 * texel
// (hlsl:57-62, 127-137)
__device__ __forceinline__ f3 culled_sample(const SceneDev& sc, f3 D, LaneStats& st)
{
    const f3 e = env_lookup(sc, D);
    const f3 c = mk3(fmaf(1.0f, e.x, 0.0f), fmaf(1.0f, e.y, 0.0f), fmaf(1.0f, e.z, 0.0f));
    ++st.rays;
    return c;
}

// The frame: a wave is one 8x8 pixel block of an a.W x a.H raster (four blocks next to each other to a workgroup) and a lane one
// pixel; the lane folds its n_samples samples and stores once.  sample(s, fx, fy, fw, fh, may_hit, stk, st) returns sample s'
// contribution to the pixel, weighted where the kernel weights; s and may_hit are wave-uniform, and the wave reconverges behind
// every call.  Outputs are W * H rasters, each written only if its pointer is given (wave-uniform branches on kernel arguments).
template <int STACK, class E, class F>
__device__ __forceinline__ void render_frame(const DispatchDev& a, uint32_t n_samples, uint32_t blocks_x, uint32_t n_blocks, float4* out_f32,
                                             uint32_t* out_rgba8, uint32_t* out_n, F&& sample)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    E* stk = lane_stack<STACK, E>(wave, lane);
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;                           // lanes outside the frame trace nothing and store nothing
    // A block outside the launch's screen rectangle is background: every sample is culled_sample (k_render_fused's branch).  The
    // rectangle (rr_host_screen_rect; rr_host_lens_screen_rect for a lens: the union over the disk's bounding square; the union of
    // the keys used where there are keys) holds the projection of the scene's box in pixel-centre coordinates plus 8 pixels of
    // margin, of which a quarter pays for the fp32 error of the ray directions; a sample position lies inside its pixel, at most
    // half a pixel from the centre, so a block that does not touch the rectangle keeps every sample more than five pixels away
    // from anything a ray could hit.  A Miss looks at no table, no medium and no light, and is weighted like any other sample.
    const bool may_hit = x0 + 8u > a.hx0 && x0 < a.hx1 && y0 + 8u > a.hy0 && y0 < a.hy1;
    const float fx = (float)x, fy = (float)y, fw = (float)a.W, fh = (float)a.H;
    LaneStats st;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < n_samples; ++s) {
        const f3 c = sample(s, fx, fy, fw, fh, may_hit, stk, st);
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

// sample s' primary ray behind a lens: lens_ray, or sample_ray where the lens is a pinhole
__device__ __forceinline__ RayState lens_or_pinhole_ray(const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const SampleOffsets& loff,
                                                        const LensDev& lens, uint32_t s, float fx, float fy, float fw, float fh)
{
    return lens.pinhole ? sample_ray(a, cam, off, s, fx, fy, fw, fh) : lens_ray(a, cam, off, loff, lens, s, fx, fy, fw, fh);
}

// entry s of a byte-per-sample table (SampleBands, SampleKeys): byte s & 3 of word s >> 2, least significant first.  Wave-uniform
// with s: what it indexes has a scalar address
template <class T> __device__ __forceinline__ uint32_t sample_byte(const T& t, uint32_t s)
{
    return (t.w[s >> 2] >> ((s & 3u) * 8u)) & 0xffu;
}

// p = weight * c per channel, one rounding each
__device__ __forceinline__ f3 weighted(const float* w, f3 c)
{
    return mk3(w[0] * c.x, w[1] * c.y, w[2] * c.z);
}

// For the kernels that take the scene from a key record in memory (k_render_shutter, k_render_lit).  A pointer read from such a
// record is a generic pointer to the compiler, which the tree would dereference with flat_load --
// through the aperture check and both memory counters, the LDS stacks' among them -- where k_render_composed, whose pointers are
// kernel arguments and known to be global, uses global_load with a scalar base.  The record's pointers are hipMalloc'ed device
// memory: in_global says so, by way of the global address space and back.  The empty statement between the two casts keeps the
// pair from being folded away before the address spaces are inferred; it holds the pointer in scalar registers, where it is anyway
// (the record has a scalar address), and a pointer the build does not use is dropped with it.
template <class T> __device__ __forceinline__ const T* in_global(const T* p)
{
    const __attribute__((address_space(1))) T* g = (const __attribute__((address_space(1))) T*)p;
    asm("" : "+s"(g));
    return (const T*)g;
}

// The scene of key record kd (a scalar address: its fields come through scalar loads at the head of a sample): a copy whose
// pointers are known to be global and whose environment is the launch's own -- a record never carries an environment pointer, so
// that replacing the map after a capture cannot leave a stale one behind
__device__ __forceinline__ SceneDev key_scene(const KeyDev* __restrict__ kd, const float4* env, int32_t env_w, int32_t env_h)
{
    SceneDev sc = kd->sc;
    sc.blas0.nodes = in_global(sc.blas0.nodes); sc.blas0.tris = in_global(sc.blas0.tris); sc.blas0.nrms = in_global(sc.blas0.nrms);
    sc.pool_nodes = in_global(sc.pool_nodes); sc.pool_tris = in_global(sc.pool_tris); sc.pool_nrms = in_global(sc.pool_nrms);
    sc.insts = in_global(sc.insts);
    sc.env = env; sc.env_w = env_w; sc.env_h = env_h;
    return sc;
}

// The caller-ray shell: one lane per ray, a wave is 64 consecutive rays.  A lane starts on the 48-byte record the caller wrote
// (origin, tmin, dir, tmax as they are; q[2] -- flags, instance_mask, pad -- is not read: the tree's TraceRay calls fix them) as
// RayGen's payload (RayTracing.hlsl:57-60); tree(r, stk, st) returns the colour of its tree.  Each output has n entries and is
// written only if its pointer is given.
template <int STACK, class E, class F>
__device__ __forceinline__ void shade_caller_ray(const DispatchDev& a, const rr_ray_dev* rays, uint32_t n, float4* out_f32, uint32_t* out_rgba8,
                                                 uint32_t* out_n, F&& tree)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    E* stk = lane_stack<STACK, E>(wave, lane);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(rays + i);
    const uint4 o = q[0], d = q[1];
    RayState r;
    r.O = mk3(__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z));
    r.D = mk3(__uint_as_float(d.x), __uint_as_float(d.y), __uint_as_float(d.z));
    r.tmin = __uint_as_float(o.w); r.tmax = __uint_as_float(d.w);
    r.w = 1.0f; r.count = 0; r.outside = true;
    LaneStats st;
    const f3 acc = tree(r, stk, st);
    if (out_f32) out_f32[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
    if (out_rgba8) store_pixel(a, out_rgba8, nullptr, i, acc);
    if (out_n) out_n[i] = st.rays;
}

} // namespace rr
