// rr_render_adaptive.hip -- adaptive supersampling (rr_render_adaptive[_device]) for gfx950: every pixel takes the first n_base
// samples of the pattern, and only the pixels whose base samples show contrast take the rest, up to n_max.
//
// Every pixel of the result is, bit for bit, that pixel of k_render_samples at n_base or at n_max samples: the sample rays, the
// ray tree and the fold ((c_0 + c_1) + ...) are those of rr_render_samples.hip, and what decides between the two is a handful of
// fp32 comparisons on display values (include/rrdxr.h has the rule; the build's -ffp-contract=off keeps them unfused).  Stages,
// all on one stream, all state in the caller's workspace (AdaptiveWorkspace, rr_launch.h):
//   k_adaptive_base      k_render_samples' wave = 8x8 block, lane = pixel in Morton order; samples 0..n_base-1; one record per
//                        pixel (sum r, g, b and the pixel's own contrast) and its ray count
//   k_adaptive_classify  the same mapping without tracing: own record and four neighbours' -> the decision; finalises the unrefined
//                        pixels, writes n_taken of all, and one 64-bit ballot per block
//   k_adaptive_scan      one workgroup: exclusive scan of the blocks' popcounts -> each block's base in the list, and the total
//   k_adaptive_list      ballot + base -> the refined pixels' indices: blocks in raster order, lanes in Morton order
//   k_adaptive_refine    a wave takes 64 consecutive list entries, a lane one refined pixel: samples n_base..n_max-1 continue
//                        the stored fold
// Nothing is appended by atomics and nothing is counted in place, so a workspace is reusable without clearing and the list's
// order -- the refine pass's coherence -- is the same in every run.
#include <hip/hip_runtime.h>
#include "rr_choice.h"
#include "rr_render_common.h"

namespace rr {

// what store_pixel shows of a channel value, in [0, 1]: NaN -> 0, +inf -> 1 (fmaxf / fminf return the operand that is a number)
__device__ __forceinline__ float display_value(float c, bool tonemap)
{
    const float m = fmaxf(c, 0.0f);
    return tonemap ? fminf(m / (1.0f + m), 1.0f) : fminf(m, 1.0f);
}

// a: as for k_render_samples.  rec[o] = (sum of the base samples r, g, b; r_own), cnt[o] = TraceRay calls so far
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_adaptive_base(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                            uint32_t n_base, uint32_t blocks_x, uint32_t n_blocks,
                                                                                            float4* rec, uint32_t* cnt)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t wb = blockIdx.x * 4u + wave;                 // the wave's 8x8 block, in raster order
    if (wb >= n_blocks) return;
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x0 = px.x0, y0 = px.y0, x = px.x, y = px.y;
    if (x >= a.W || y >= a.H) return;
    const bool may_hit = x0 + 8u > a.hx0 && x0 < a.hx1 && y0 + 8u > a.hy0 && y0 < a.hy1;      // k_render_samples' background branch
    const bool tm = a.tonemap != 0u;
    const float fx = (float)x, fy = (float)y, fw = (float)a.W, fh = (float)a.H;
    LaneStats st;
    f3 sum = mk3(0.0f, 0.0f, 0.0f), lo = mk3(1.0f, 1.0f, 1.0f), hi = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t s = 0; s < n_base; ++s) {
        RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
        f3 c;
        if (!may_hit) {
            const f3 e = env_lookup(sc, r.D);
            c = mk3(fmaf(1.0f, e.x, 0.0f), fmaf(1.0f, e.y, 0.0f), fmaf(1.0f, e.z, 0.0f));
            ++st.rays;
        } else {
            RegPark<PEND> park;
            c = ray_tree<TLAS, E>(sc, a, r, stk, park, st);
        }
        sum = s ? mk3(sum.x + c.x, sum.y + c.y, sum.z + c.z) : c;
        const f3 v = mk3(display_value(c.x, tm), display_value(c.y, tm), display_value(c.z, tm));
        lo = mk3(fminf(lo.x, v.x), fminf(lo.y, v.y), fminf(lo.z, v.z));
        hi = mk3(fmaxf(hi.x, v.x), fmaxf(hi.y, v.y), fmaxf(hi.z, v.z));
    }
    const float r_own = fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z);
    const size_t o = (size_t)y * a.W + x;
    rec[o] = make_float4(sum.x, sum.y, sum.z, r_own);
    cnt[o] = st.rays;
}

// a: W, H, tonemap.  One wave per 8x8 block in k_adaptive_base's mapping, four blocks per workgroup.
__global__ __launch_bounds__(256) void k_adaptive_classify(DispatchDev a, uint32_t n_base, uint32_t n_max, float threshold, uint32_t blocks_x,
                                                          uint32_t n_blocks, const float4* rec, const uint32_t* cnt, unsigned long long* masks,
                                                          float4* out_f32, uint32_t* out_rgba8, uint32_t* out_n, uint32_t* out_taken)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t wb = blockIdx.x * 4u + wave;
    if (wb >= n_blocks) return;                                 // (wave-uniform)
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x = px.x, y = px.y;
    const bool inside = x < a.W && y < a.H;
    const bool tm = a.tonemap != 0u;
    const float fb = (float)n_base;
    bool refine = false;
    if (inside) {
        const size_t o = (size_t)y * a.W + x;
        const float4 p = rec[o];
        const f3 res = mk3(p.x / fb, p.y / fb, p.z / fb);
        const f3 b = mk3(display_value(res.x, tm), display_value(res.y, tm), display_value(res.z, tm));
        float r_nb = 0.0f;
        // the 4-neighbours inside the frame: left, right, up, down
        const bool has[4] = { x > 0u, x + 1u < a.W, y > 0u, y + 1u < a.H };
        const size_t at[4] = { o - 1u, o + 1u, o - a.W, o + a.W };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!has[k]) continue;
            const float4 q = rec[at[k]];
            const f3 bq = mk3(display_value(q.x / fb, tm), display_value(q.y / fb, tm), display_value(q.z / fb, tm));
            r_nb = fmaxf(r_nb, fmaxf(fmaxf(fabsf(b.x - bq.x), fabsf(b.y - bq.y)), fabsf(b.z - bq.z)));
        }
        refine = p.w > threshold || r_nb > threshold;
        if (out_taken) out_taken[o] = refine ? n_max : n_base;
        if (!refine || n_base == n_max) {                       // (n_base == n_max: no refine pass follows, and the base fold is the whole one)
            if (out_f32) out_f32[o] = make_float4(res.x, res.y, res.z, 1.0f);
            if (out_rgba8) store_pixel(a, out_rgba8, nullptr, o, res);
            if (out_n) out_n[o] = cnt[o];
        }
    }
    const unsigned long long m = __ballot(refine);
    if (lane == 0u) masks[wb] = m;
}

// base[i] = refined pixels of the blocks before block i, base[n_blocks] = all of them.  One workgroup of 1024 threads, each with a
// contiguous run of blocks.
__global__ __launch_bounds__(1024) void k_adaptive_scan(const unsigned long long* masks, uint32_t n_blocks, uint32_t* base)
{
    __shared__ uint32_t part[2][1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + 1023u) / 1024u;
    const uint32_t i0 = min(t * per, n_blocks), i1 = min(i0 + per, n_blocks);
    uint32_t mine = 0;
    for (uint32_t i = i0; i < i1; ++i) mine += (uint32_t)__popcll(masks[i]);
    part[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (uint32_t d = 1; d < 1024u; d <<= 1) {                  // inclusive scan of the threads' sums
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = part[cur][t] - mine;
    for (uint32_t i = i0; i < i1; ++i) { base[i] = run; run += (uint32_t)__popcll(masks[i]); }
    if (t == 1023u) base[n_blocks] = part[cur][t];
}

// list[base[block] + rank of the lane among the block's refined lanes] = the lane's pixel
__global__ __launch_bounds__(256) void k_adaptive_list(uint32_t W, uint32_t blocks_x, uint32_t n_blocks, const unsigned long long* masks,
                                                      const uint32_t* base, uint32_t* list)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t wb = blockIdx.x * 4u + wave;
    if (wb >= n_blocks) return;
    const unsigned long long m = masks[wb];
    if (!((m >> lane) & 1ull)) return;                          // (set only for lanes inside the frame)
    const WavePixel px = wave_pixel(wb, blocks_x, lane);
    const uint32_t x = px.x, y = px.y;
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    list[base[wb] + rank] = y * W + x;                          // (W * H <= 2^30)
}

// a: as for k_adaptive_base.  total: base[n_blocks].  Waves stride over the list by the grid's waves: a grid sized for the worst
// case makes one trip, most waves none.
template <int STACK, int PEND, bool TLAS, class E>
__global__ __launch_bounds__(256, (ShadeWaves<STACK, TLAS, E>::value)) void k_adaptive_refine(SceneDev sc, DispatchDev a, CamDev cam, SampleOffsets off,
                                                                                              uint32_t n_base, uint32_t n_max, const uint32_t* list,
                                                                                              const uint32_t* total, const float4* rec,
                                                                                              const uint32_t* cnt, float4* out_f32, uint32_t* out_rgba8,
                                                                                              uint32_t* out_n)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;
    const uint32_t n = *total;
    const float fw = (float)a.W, fh = (float)a.H, fm = (float)n_max;
    for (uint32_t w0 = (blockIdx.x * 4u + wave) * 64u; w0 < n; w0 += gridDim.x * 256u) {
        const uint32_t i = w0 + lane;
        if (i >= n) continue;
        const uint32_t o = list[i];
        const uint32_t y = o / a.W, x = o - y * a.W;
        const float fx = (float)x, fy = (float)y;
        const float4 p = rec[o];
        f3 sum = mk3(p.x, p.y, p.z);
        LaneStats st;
        for (uint32_t s = n_base; s < n_max; ++s) {
            const RayState r = sample_ray(a, cam, off, s, fx, fy, fw, fh);
            RegPark<PEND> park;
            const f3 c = ray_tree<TLAS, E>(sc, a, r, stk, park, st);
            sum = mk3(sum.x + c.x, sum.y + c.y, sum.z + c.z);
        }
        const f3 out = mk3(sum.x / fm, sum.y / fm, sum.z / fm);
        if (out_f32) out_f32[o] = make_float4(out.x, out.y, out.z, 1.0f);
        if (out_rgba8) store_pixel(a, out_rgba8, nullptr, o, out);
        if (out_n) out_n[o] = cnt[o] + st.rays;
    }
}

hipError_t launch_render_adaptive(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, uint32_t n_base,
                                  uint32_t n_max, float threshold, const AdaptiveWorkspace& ws, uint32_t* n_taken, uint32_t refine_groups, const ShadeOut& out,
                                  FusedVariant v, hipStream_t s)
{
    FrameBlocks fb;
    if (!frame_blocks(a, n_max, v, fb) || n_base == 0 || n_base > n_max) return hipErrorInvalidValue;
    const uint32_t blocks_x = fb.blocks_x, n_blocks = fb.n_blocks, groups = fb.groups, worst = (uint32_t)(((size_t)a.W * a.H + 255u) / 256u);
    if (refine_groups == 0 || refine_groups > worst) refine_groups = worst;
    // both traced stages take the scene's FusedVariant through the ray-tree kernels' ladder (for_tree_variant, rr_choice.h)
    const bool si = sc.single_identity != 0u;
    if (hipError_t e = RR_LAUNCH_TREE_KERNEL(k_adaptive_base, si, v, groups, s, sc, a, cam, off, n_base, blocks_x, n_blocks, ws.rec, ws.cnt)) return e;
    hipLaunchKernelGGL(k_adaptive_classify, dim3(groups), dim3(256), 0, s, a, n_base, n_max, threshold, blocks_x, n_blocks, ws.rec, ws.cnt, ws.masks, out.f32,
                       out.rgba8, out.n_rays, n_taken);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(1024), 0, s, ws.masks, n_blocks, ws.base);
    if (hipError_t e = hipGetLastError()) return e;
    if (n_base == n_max) return hipSuccess;                     // no samples are left to take: classify has made every pixel final
    hipLaunchKernelGGL(k_adaptive_list, dim3(groups), dim3(256), 0, s, a.W, blocks_x, n_blocks, ws.masks, ws.base, ws.list);
    if (hipError_t e = hipGetLastError()) return e;
    return RR_LAUNCH_TREE_KERNEL(k_adaptive_refine, si, v, refine_groups, s, sc, a, cam, off, n_base, n_max, ws.list, ws.total, ws.rec, ws.cnt, out.f32, out.rgba8,
                                 out.n_rays);
}

} // namespace rr
