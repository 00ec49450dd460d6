// rr_render_fused.hip -- the DispatchRays stand-in (RefractionDemo.cpp:580-594) for gfx950.
//
// One launch renders a frame: each lane owns a pixel and runs RayGen (RayTracing.hlsl:42-64),
// then walks that pixel's whole ray tree depth-first -- ClosestHit (hlsl:79-125) spawns the
// refracted child (followed immediately) and the reflected child (parked in registers),
// Miss (hlsl:127-137) adds weight*texel.  The recursive "color += w * child.color" of the
// shader becomes a path-weight sum taken in the same leaf order, so results are deterministic
// and need no atomics, queues or second launch.  A wave covers an 8x8 pixel block (Morton lane
// order) for BVH / env-map coherence; a 256-thread block covers a 32x8 strip of a 32x32 tile,
// tiles are dealt round-robin to ranks (multi-GPU sharding), and the block->tile map keeps each
// XCD on a contiguous run of tiles.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "rr_render_common.h"

namespace rr {

// WPS: waves per SIMD the instantiation is built for (0: what its stack size leaves room for, see rr_render_common.h)
template <int STACK, int PEND, bool STATS, bool TLAS, bool DIAG = false, class E = uint32_t, int WPS = 0>
__global__ __launch_bounds__(256, WPS ? WPS : TLAS ? RR_TLAS_WAVES_PER_SIMD(STACK) : sizeof(E) == 2 ? 8 : RR_FUSED_WAVES_PER_SIMD(STACK)) void k_render_fused(SceneDev sc, DispatchDev a)
{
    __shared__ uint32_t diag_trips[12];    // per wave: internal trips, leaf trips, shading passes
    const unsigned long long diag_t0 = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
    const unsigned long long diag_rt0 = DIAG ? __builtin_amdgcn_s_memrealtime() : 0ull;
    if (DIAG && threadIdx.x < 12) diag_trips[threadIdx.x] = 0;
    if (DIAG) __syncthreads();
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    E* stk = reinterpret_cast<E*>(lds) + wave * (STACK * 64) + lane;

    const BlockPos bp = wave_block_pos(a, blockIdx.x * 4u + wave);
    const uint32_t lx = compact1by1(lane), ly = compact1by1(lane >> 1);
    const uint32_t x = bp.x0 + lx, y = bp.y0 + ly;
    const bool valid = bp.tile_ok && x < a.W && y < a.H;
    const CamDev& cb = a.cams[bp.frame];                              // wave-uniform: scalar loads

    LaneStats st;
    stats_clock_begin<STATS>(st);
    st.blocks = bp.tile_ok ? 1u : 0u;
    if (STATS && bp.tile_ok && !(DIAG || (bp.x0 + 8u > a.hx0 && bp.x0 < a.hx1 && bp.y0 + 8u > a.hy0 && bp.y0 < a.hy1))) st.bg_blocks = 1u;
    if (valid) {
        st.pixels = 1;
        const bool may_hit = DIAG || (bp.x0 + 8u > a.hx0 && bp.x0 < a.hx1 && bp.y0 + 8u > a.hy0 && bp.y0 < a.hy1);
        f3 acc;
        if (!may_hit) {
            // A block outside the scene's screen rectangle (nine in ten on the reference's scenes): RayGen and one Miss, with none
            // of the ray-tree machinery -- no traversal state, no parked rays, nothing spilled -- and the same arithmetic:
            // payload.color = 0 + 1 * texel (hlsl:57-62, 127-137)
            const f3 D = camera_ray_dir(cb.M, a.sx[x], a.sy[y]);
            st.rays = 1;
            if (STATS) { st.miss = 1; if (first_active_lane()) st.passes = 1; }
            const f3 e = env_lookup(sc, D);
            acc = mk3(fmaf(1.0f, e.x, 0.0f), fmaf(1.0f, e.y, 0.0f), fmaf(1.0f, e.z, 0.0f));
        } else {
            RegPark<PEND> park;
            acc = render_pixel<STATS, TLAS, DIAG, E, GlobalNodes>(sc, a, cb, x, y, true, stk, GlobalNodes{}, park, st, Diag{ &diag_trips[wave], 4 });
        }
        // What the store needs is read from the kernel's argument block AGAIN here instead of being kept across the renderer:
        // the renderer keeps ~70 scalars live, the compiler allows itself 80 at eight waves per SIMD and moves the rest through
        // vector lanes -- 43 vector instructions per wave before this, 13 now.  (Arguments lie in the block in order, each at
        // its own alignment: `a` follows `sc`.  The asm keeps the compiler from recognising the loads as the ones it already
        // did at the top; every frame-parity test would fail on a wrong offset.)
        typedef const __attribute__((address_space(4))) DispatchDev* KA;
        KA ap = (KA)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() +
                     ((sizeof(SceneDev) + alignof(DispatchDev) - 1) / alignof(DispatchDev)) * alignof(DispatchDev));
        asm volatile("" : "+s"(ap));
        const uint32_t k_compact = ap->compact_out, k_W = ap->W, k_tonemap = ap->tonemap;
        const size_t o = k_compact == 0u ? (size_t)y * k_W + x
                                         : (size_t)bp.tile_local * (TILE * TILE) + (bp.py0 + ly) * TILE + (bp.px0 + lx);
        uint32_t* const out_rgba8 = bp.bg ? ap->out_bg + (size_t)bp.frame * ap->bg_stride : ap->out_rgba8 + (size_t)bp.frame * ap->frame_stride;
        float4* const out_f32 = ap->out_f32 ? ap->out_f32 + (size_t)bp.frame * ap->frame_stride : nullptr;
        DispatchDev a2;
        a2.tonemap = k_tonemap; a2.compact_out = k_compact;
        store_pixel(a2, out_rgba8, out_f32, o, acc);
    }

    if (DIAG) {
        uint32_t mx = st.rays;
        for (int off = 32; off > 0; off >>= 1) { uint32_t v = __shfl_xor(mx, off, 64); mx = v > mx ? v : mx; }
        if (lane == 0) {
            unsigned long long* d = a.diag + (size_t)(blockIdx.x * 4u + wave) * 4;
            d[0] = ((unsigned long long)diag_trips[8 + wave] << 40) | ((unsigned long long)diag_trips[4 + wave] << 20) | diag_trips[wave];
            d[1] = __builtin_amdgcn_s_memtime() - diag_t0; d[2] = mx | ((diag_rt0 & 0xffffffffull) << 32);
            d[3] = (unsigned long long)(diag_trips[wave] + diag_trips[4 + wave]) | ((__builtin_amdgcn_s_memrealtime() & 0xffffffffull) << 32);   // start / end on the 100 MHz clock all CUs share
        }
    }
    flush_stats<STATS>(a, st, blockIdx.x * 4u + wave, lane);
}

// ------------------------------------------------------------------------------------ launchers
// name of the render kernel instantiation the calling thread launched last (rr_stats::render_kernel_name): the one slot every
// render launcher writes, those of the other sources included
static thread_local char g_kernel_name[96] = "";
const char* last_render_kernel_name() { return g_kernel_name; }
void set_render_kernel_name(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel_name, sizeof g_kernel_name, fmt, ap);
    va_end(ap);
}

template <int STACK, int PEND, bool TLAS>
static hipError_t launch_fused_spt(const SceneDev& sc, const DispatchDev& a, bool stats, hipStream_t s)
{
    const size_t lds = (size_t)4 * STACK * 64 * sizeof(uint32_t);
    set_render_kernel_name("k_render_fused<%d, %d, %s, %s, false, unsigned int, 0>", STACK, PEND, stats ? "true" : "false", TLAS ? "true" : "false");
    if (stats) hipLaunchKernelGGL((k_render_fused<STACK, PEND, true, TLAS>), dim3(a.n_blocks), dim3(256), lds, s, sc, a);
    else       hipLaunchKernelGGL((k_render_fused<STACK, PEND, false, TLAS>), dim3(a.n_blocks), dim3(256), lds, s, sc, a);
    return hipGetLastError();
}

template <int STACK, int PEND>
static hipError_t launch_fused_sp(const SceneDev& sc, const DispatchDev& a, bool stats, hipStream_t s)
{
    if (!sc.single_identity) return launch_fused_spt<STACK, PEND, true>(sc, a, stats, s);
    return launch_fused_spt<STACK, PEND, false>(sc, a, stats, s);
}

// reference-scene kernel on 16-bit stack entries (meshes below 32 768 triangles, trees of 20..39 levels): 39 entries are
// 19 968 B per workgroup, eight workgroups per CU
template <int PEND>
static hipError_t launch_fused_s16(const SceneDev& sc, const DispatchDev& a, bool stats, hipStream_t s)
{
    const size_t lds = (size_t)4 * 39 * 64 * sizeof(uint16_t);
    set_render_kernel_name("k_render_fused<39, %d, %s, false, false, unsigned short, 0>", PEND, stats ? "true" : "false");
    if (stats) hipLaunchKernelGGL((k_render_fused<39, PEND, true, false, false, uint16_t>), dim3(a.n_blocks), dim3(256), lds, s, sc, a);
    else       hipLaunchKernelGGL((k_render_fused<39, PEND, false, false, false, uint16_t>), dim3(a.n_blocks), dim3(256), lds, s, sc, a);
    return hipGetLastError();
}

// Two-level scenes whose stack entries fit 16 bits (fewer than 32 768 pool nodes and triangles + instances) and whose trees are
// at most 30 levels deep: 15 KB of stacks per workgroup instead of 31, so the LDS no longer caps the kernel at five waves per
// SIMD, and the build for seven (72 registers, 64 words through scratch) is the fastest -- the 1 024-monkey grid at 2160p,
// Depth 16: 7.51 ms per frame with 32-bit stacks (five waves), 7.23 / 6.95 / 7.24 ms built for six / seven / eight.
// (Parking the reflected rays in LDS instead of registers -- 96 registers, five waves, a third of the spills -- measured 7.76.)
// Trees of 31..39 levels (C4: ott.obj under a TLAS) get the 39-entry build for five waves: 934 us per frame at Depth 16
// against 979 on 32-bit stacks (four waves), 993 / 1 051 built for six / seven; launches of one or two slices stay on the
// 32-bit build (2.14 against 2.44 ms).
template <int STACK, int WPS>
static hipError_t launch_fused_tlas16(const SceneDev& sc, const DispatchDev& a, bool stats, hipStream_t s)
{
    const size_t lds = (size_t)4 * STACK * 64 * sizeof(uint16_t);
    set_render_kernel_name("k_render_fused<%d, 2, %s, true, false, unsigned short, %d>", STACK, stats ? "true" : "false", WPS);
    if (stats) hipLaunchKernelGGL((k_render_fused<STACK, 2, true, true, false, uint16_t, WPS>), dim3(a.n_blocks), dim3(256), lds, s, sc, a);
    else       hipLaunchKernelGGL((k_render_fused<STACK, 2, false, true, false, uint16_t, WPS>), dim3(a.n_blocks), dim3(256), lds, s, sc, a);
    return hipGetLastError();
}

hipError_t launch_render_fused(const SceneDev& sc, const DispatchDev& a, int stack, int pend, bool stats, hipStream_t s, bool stack16)
{
    if (a.n_blocks == 0) return hipSuccess;
#ifndef RR_TLAS30_WPS
#define RR_TLAS30_WPS 7
#endif
#ifndef RR_TLAS39_WPS
#define RR_TLAS39_WPS 5
#endif
    if (stack16 && !a.diag && !sc.single_identity && pend <= 2 && stack <= 30) return launch_fused_tlas16<30, RR_TLAS30_WPS>(sc, a, stats, s);
    if (stack16 && !a.diag && !sc.single_identity && pend <= 2 && stack <= 39) return launch_fused_tlas16<39, RR_TLAS39_WPS>(sc, a, stats, s);
    if (stack16 && !a.diag && sc.single_identity && stack <= 39)
        return pend <= 2 ? launch_fused_s16<2>(sc, a, stats, s) : launch_fused_s16<8>(sc, a, stats, s);
    if (a.diag) {       // diagnostic build of the reference-scene kernel (RR_DEBUG_DIAG; never used by the product path)
        if (stack <= 19) hipLaunchKernelGGL((k_render_fused<19, 2, false, false, true>), dim3(a.n_blocks), dim3(256), 4 * 19 * 64 * 4, s, sc, a);
        else hipLaunchKernelGGL((k_render_fused<31, 2, false, false, true>), dim3(a.n_blocks), dim3(256), 4 * 31 * 64 * 4, s, sc, a);
        return hipGetLastError();
    }
    if (stack <= 19 && pend <= 2) return launch_fused_sp<19, 2>(sc, a, stats, s);
    if (stack <= 22 && pend <= 2) return launch_fused_sp<22, 2>(sc, a, stats, s);
    if (stack <= 26 && pend <= 2) return launch_fused_sp<26, 2>(sc, a, stats, s);
    if (stack <= 31) return pend <= 2 ? launch_fused_sp<31, 2>(sc, a, stats, s) : launch_fused_sp<31, 8>(sc, a, stats, s);
    if (stack <= 39) return pend <= 2 ? launch_fused_sp<39, 2>(sc, a, stats, s) : launch_fused_sp<39, 8>(sc, a, stats, s);
    return pend <= 2 ? launch_fused_sp<64, 2>(sc, a, stats, s) : launch_fused_sp<64, 8>(sc, a, stats, s);
}

} // namespace rr
