// rr_render_paths.hip -- k_render_paths: the renderer for launches of one or two slices.
//
// Path-parallel form, for launches of one or two slices (the reference's own shape is DispatchRays(W,H,1),
// RefractionDemo.cpp:589-594).  Such a launch lasts as long as its most expensive wave: in k_render_fused a lane walks its
// pixel's whole ray tree, up to 19 rays one after the other on monkey.obj, and the wave that owns that pixel makes 1 400
// loop trips while the rest of the chip is idle (Depth 1: 460 us per frame against 82 at Depth 64).  The tree only
// branches while count < max_reflect; for max_reflect <= 2 it therefore has at most four root-to-leaf paths -- refract or
// reflect at the primary hit, refract or reflect at the next, refractions only from there on -- and each ends in at most
// one leaf (a Miss, weight * texel; a terminal hit or a total internal reflection ends it with nothing).  Here FOUR lanes
// share a pixel, one in each wave of the workgroup, wave p following path p (bit 1: reflect at count 0, bit 0: reflect at
// count 1) for the 64 pixels of the block; the four leaves are then
// summed in the recursion's order -- TT, TR, RT, RR, the order in which k_render_fused reaches them -- with the same
// fma sequence, a path without a leaf contributing fma(0, 0, acc) = acc.  So the frame is bit-identical, the longest chain of
// dependent rays drops from 19 to 2 + the refraction limit, and a block's work spreads over four waves.  The primary ray is
// traced by all four lanes and the two count-1 rays by two each (more work, which a launch of one slice has room for);
// counters count a shared ray once.
// A workgroup is an 8x8 pixel block inside the scene's screen rectangle; the blocks outside the rectangle follow in the
// same launch as 32x8 strips, one Miss per pixel without a trace.  Measured and rejected (monkey.obj 1080p, Depth 1, 8/2
// bounces, us per frame; this form: 244): the four paths of a pixel in adjacent lanes of one wave, the first form of this
// kernel (271: refracted and reflected rays in one wave diverge at once); waves that retire as they finish, the last one
// summing, on 16-bit stacks so that more workgroups fit a CU (265; ott.obj 708 against 634) and, the other way, fewer
// workgroups per CU (6: 292, 4: 328) -- the chains of dependent rays that decide the launch slow down when more waves
// compete, the bulk of the frame when fewer run; s_setprio by ray depth (no effect: the waves deep in a chain are the oldest
// on their SIMD anyway).
#include <hip/hip_runtime.h>
#include "rr_render_common.h"

namespace rr {

struct PathLeaf { float w; f3 e; };

// Called by all 64 lanes of all four waves of the workgroup (valid: the lane has a pixel; it contains workgroup barriers).
// ww: the wave's stack region as 32-bit words; xch: wave 1's.  Levels with few rays left are traced by groups of lanes
// (trace_blas_group): 2 lanes per ray from 32 rays down, 4 from 16.
template <bool STATS, bool TLAS, class E>
__device__ __forceinline__ PathLeaf render_path(const SceneDev& sc, const DispatchDev& a, const CamDev& cb, uint32_t x, uint32_t y, bool valid,
                                                uint32_t path, E* stk, uint32_t* ww, uint32_t* xch, uint32_t lane, LaneStats& st, uint32_t* diag_lv = nullptr)
{
    PathLeaf leaf; leaf.w = 0.0f; leaf.e = mk3(0.0f, 0.0f, 0.0f);
    f3 O = mk3(cb.cam[0], cb.cam[1], cb.cam[2]);
    f3 D = valid ? camera_ray_dir(cb.M, a.sx[x], a.sy[y]) : mk3(0.0f, 0.0f, 1.0f);
    float w = 1.0f;
    uint32_t count = 0;
    bool outside = true, alive = valid;
    float tmin = a.tmin_p, tmax = a.tmax_p;
    for (uint32_t level = 0;; ++level) {
        const unsigned long long m_alive = __ballot(alive);
        if (level >= 2u && m_alive == 0ull) break;          // (levels 0 and 1 hold workgroup barriers: every wave goes through them)
        const int n_alive = __popcll(m_alive);
        // the lane that accounts for this ray (and owns its leaf, should it be one): rays at count 0 are shared by the four
        // lanes of the pixel, rays at count 1 by the two with the same first turn
        const bool owner = level == 0u ? path == 0u : level == 1u ? (path & 1u) == 0u : true;
        if (diag_lv && alive) {      // diagnostic builds: lanes alive at this level, time at which it starts
            if (first_active_lane()) diag_lv[level < 15u ? level : 15u] = (uint32_t)n_alive | ((uint32_t)__builtin_amdgcn_s_memrealtime() << 8);
        }
        HitRec h;
        h.t = tmax; h.hit = false; h.prim = 0; h.leaf = 0; h.inst = 0; h.U = 0.0f; h.V = 0.0f; h.ad = 1.0f;
        TravCounters cnt; cnt.nodes = 0; cnt.tris = 0;
        const uint32_t cullf = outside ? CULL_BACK : CULL_FRONT;
        if (level < 2u) {
            // A shared ray is traced ONCE: by wave 0 at level 0 (the primary ray of the block's 64 pixels), by waves 0 and 2 at
            // level 1 (the refracted and the reflected child); the closest hit -- t, leaf, instance -- goes to the other waves of
            // the workgroup through LDS (`xch`: rows of wave 1's stack region, which does not trace before level 2) and each
            // shades it for its own path: the hit attributes and the shading are the same arithmetic on the same operands.
            uint32_t* const row = xch + (level == 0u ? 0u : 3u + 3u * (path >> 1)) * 64u + lane;
            if (owner) {
                if (alive) trace_scene<STATS, TLAS, E, GlobalNodes>(sc, O, D, tmin, tmax, cullf, h, stk, cnt);
                row[0] = __float_as_uint(h.t); row[64] = h.hit ? h.leaf : 0xffffffffu; row[128] = h.inst;
            }
            __syncthreads();
            if (!owner && alive) {
                const uint32_t l = row[64];
                if (l != 0xffffffffu) {
                    h.t = __uint_as_float(row[0]); h.leaf = l; h.inst = row[128]; h.hit = true;
                    if (!TLAS) hit_attributes(sc.blas0.tris, O, D, h);
                    else {
                        const InstDev& in = sc.insts[h.inst];
                        f3 Oh = O, Dh = D;
                        if (!in.identity) { Oh = xform_point(in.inv, O); Dh = xform_dir(in.inv, D); }
                        hit_attributes(sc.pool_tris, Oh, Dh, h);
                    }
                }
            }
            if (level == 1u) __syncthreads();               // wave 1's stack region is a stack again from here on
        } else if (!TLAS && a.group_trace != 0u && n_alive <= 16) {
            trace_blas_group<4, STATS, E>(sc.blas0, alive, m_alive, O, D, tmin, tmax, cullf, h, stk, ww, lane, cnt);
            if (STATS) { st.cnt.nodes += cnt.nodes; st.cnt.tris += cnt.tris; cnt.nodes = 0; cnt.tris = 0; }
        } else if (!TLAS && a.group_trace != 0u && n_alive <= 32) {
            trace_blas_group<2, STATS, E>(sc.blas0, alive, m_alive, O, D, tmin, tmax, cullf, h, stk, ww, lane, cnt);
            if (STATS) { st.cnt.nodes += cnt.nodes; st.cnt.tris += cnt.tris; cnt.nodes = 0; cnt.tris = 0; }
        } else if (alive) {
            trace_scene<STATS, TLAS, E, GlobalNodes>(sc, O, D, tmin, tmax, cullf, h, stk, cnt);
        }
        if (STATS) { st.cnt.node_trips += cnt.node_trips; st.cnt.leaf_trips += cnt.leaf_trips; }
        if (alive) {
            if (owner) { ++st.rays; if (STATS) { st.cnt.nodes += cnt.nodes; st.cnt.tris += cnt.tris; } }
            if (STATS && first_active_lane()) ++st.passes;
            if (!h.hit) {                                             // Miss
                if (owner) { if (STATS) ++st.miss; leaf.w = w; leaf.e = env_lookup(sc, D); }
                alive = false;
            } else {
                if (STATS && owner) ++st.hits;
                if ((int)count >= a.max_refract) { if (STATS && owner) ++st.term; alive = false; }      // hlsl:82, payload.color stays 0
                else {
                    const f3 N = shading_normal<TLAS>(sc, h);
                    const f3 X = mk3(fmaf(h.t, D.x, O.x), fmaf(h.t, D.y, O.y), fmaf(h.t, D.z, O.z));
                    const f3 Nf = outside ? N : neg3(N);
                    const float R0 = (0.2f / 2.2f) * (0.2f / 2.2f);
                    const float b = 1.0f - dot3(D, Nf);
                    const float b2 = b * b, b4 = b2 * b2;
                    const float R = (R0 * (1.0f - R0)) * (b4 * b);
                    const float eta = outside ? a.inv_ior : a.ior;
                    f3 d1;
                    const bool refr = refract_ray(d1, D, Nf, eta);
                    if (STATS && owner && !refr) ++st.tir;
                    const bool refl = (int)count < a.max_reflect;
                    // which child this lane follows: the reflected one where its path says so (count 0: bit 1, count 1: bit 0), else the
                    // refracted one; k_render_fused follows the refracted child and parks the reflected one, or, without a refracted
                    // child, follows the reflected one directly -- that one is then the node's only subtree, and it belongs to the
                    // "reflect" lanes here as well (the "refract" lanes have no leaf below this node)
                    const bool turn = count == 0u ? (path & 2u) != 0u : count == 1u ? (path & 1u) != 0u : false;
                    const uint32_t c1 = count + 1u;
                    tmin = a.tmin_s; tmax = a.tmax_s;
                    O = X;
                    if (!turn) {
                        if (!refr) alive = false;
                        else { D = d1; w = w * (1.0f - R); count = c1; outside = !outside; }
                    } else {
                        if (!refl) alive = false;
                        else { D = normalize3(reflect_ray(D, Nf)); w = w * R; count = c1; }
                    }
                }
            }
        }
    }
    return leaf;
}

template <int STACK, bool STATS, bool TLAS, bool DIAG = false>
__global__ __launch_bounds__(256, TLAS ? 5 : 8) void k_render_paths(SceneDev sc, DispatchDev a, uint32_t n_pp_blocks, uint32_t rect_bw)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    __shared__ uint32_t diag_lv[4][16];        // diagnostic builds: per wave and ray level, lanes alive | start time << 8
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    const unsigned long long diag_t0 = DIAG ? __builtin_amdgcn_s_memrealtime() : 0ull;
    if (DIAG) { if (lane < 16u) diag_lv[wave][lane] = 0u; }
    LaneStats st;
    stats_clock_begin<STATS>(st);
    if (blockIdx.x < n_pp_blocks) {
        // (Measured and rejected, round 3: starting last launch's slowest blocks first -- as cost classes, whose empty workgroups cost
        // 30 ns each, and as the previous launch's completion order walked backwards: 250 us per frame against 245 on monkey.obj,
        // 450 against 397 on sphere.obj.  A chain of dependent rays runs at 220 us under the full chip's load and at 150 us on an
        // idle one, so a slow block gains nothing from starting while everything else does, and raster order keeps neighbours in L2.)
        const uint32_t frame = blockIdx.x % a.n_frames, b = blockIdx.x / a.n_frames;
        uint32_t* stk = lds + wave * (STACK * 64) + lane;
        // wave p follows path p of the block's 64 pixels: the lanes of a wave then trace rays of one kind (all refracted twice,
        // all reflected then refracted, ...), which stay closer together than the four paths of one pixel do
        const uint32_t path = wave;
        const uint32_t x = a.hx0 + (b % rect_bw) * 8u + compact1by1(lane), y = a.hy0 + (b / rect_bw) * 8u + compact1by1(lane >> 1);
        const bool valid = x < a.W && y < a.H;
        st.blocks = 1u;                 // (a quarter of an 8x8 block: the per-wave cost of the issue model does not apply to this kernel)
        if (valid && path == 0u) st.pixels = 1;
        const PathLeaf lf = render_path<STATS, TLAS, uint32_t>(sc, a, a.cams[frame], x, y, valid, path, stk, lds + wave * (STACK * 64), lds + 1 * (STACK * 64), lane, st,
                                                               DIAG ? diag_lv[wave] : nullptr);
        // the pixel's colour: its leaves in the recursion's order, handed over through the (now idle) stack space
        float* const mine = reinterpret_cast<float*>(lds + wave * (STACK * 64)) + lane;
        mine[0] = lf.w; mine[64] = lf.e.x; mine[128] = lf.e.y; mine[192] = lf.e.z;
        __syncthreads();
        if (wave == 0u && valid) {
            f3 acc = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float* src = reinterpret_cast<const float*>(lds + p * (STACK * 64)) + lane;
                const float w = src[0], ex = src[64], ey = src[128], ez = src[192];
                acc.x = fmaf(w, ex, acc.x); acc.y = fmaf(w, ey, acc.y); acc.z = fmaf(w, ez, acc.z);
            }
            store_pixel(a, a.out_rgba8 + (size_t)frame * a.frame_stride, a.out_f32 ? a.out_f32 + (size_t)frame * a.frame_stride : nullptr,
                        (size_t)y * a.W + x, acc);
        }
    } else {                                                       // a 32x8 strip outside the rectangle: Miss only
        const BlockPos bp = wave_block_pos(a, (blockIdx.x - n_pp_blocks) * 4u + wave);
        const uint32_t x = bp.x0 + compact1by1(lane), y = bp.y0 + compact1by1(lane >> 1);
        const bool in_rect = bp.x0 >= a.hx0 && bp.x0 < a.hx1 && bp.y0 >= a.hy0 && bp.y0 < a.hy1;
        if (bp.tile_ok && !in_rect && x < a.W && y < a.H) {
            const CamDev& cb = a.cams[bp.frame];
            const f3 D = camera_ray_dir(cb.M, a.sx[x], a.sy[y]);
            st.pixels = 1; st.rays = 1; if (STATS) st.miss = 1;
            const f3 e = env_lookup(sc, D);
            const f3 acc = mk3(fmaf(1.0f, e.x, 0.0f), fmaf(1.0f, e.y, 0.0f), fmaf(1.0f, e.z, 0.0f));
            store_pixel(a, a.out_rgba8 + (size_t)bp.frame * a.frame_stride, a.out_f32 ? a.out_f32 + (size_t)bp.frame * a.frame_stride : nullptr,
                        (size_t)y * a.W + x, acc);
        }
    }
    if (DIAG && a.diag) {       // per wave: start, end (100 MHz), block kind, then the 16 level words
        unsigned long long* d = a.diag + (size_t)(blockIdx.x * 4u + wave) * 12;
        if (lane == 0) { d[0] = diag_t0; d[1] = __builtin_amdgcn_s_memrealtime(); d[2] = blockIdx.x < n_pp_blocks ? 1ull : 0ull; d[3] = blockIdx.x; }
        if (lane < 8u) d[4 + lane] = (unsigned long long)diag_lv[wave][2 * lane] | ((unsigned long long)diag_lv[wave][2 * lane + 1] << 32);
    }
    flush_stats<STATS>(a, st, blockIdx.x * 4u + wave, lane);
}

// ------------------------------------------------------------------------------------ launchers
template <int STACK, bool TLAS>
static hipError_t launch_paths_st(const SceneDev& sc, const DispatchDev& a, uint32_t n_pp, uint32_t rect_bw, bool stats, hipStream_t s)
{
    const size_t lds = (size_t)4 * STACK * 64 * sizeof(uint32_t);
    const dim3 grid(n_pp + a.n_blocks);
    set_render_kernel_name("k_render_paths<%d, %s, %s, false>", STACK, stats ? "true" : "false", TLAS ? "true" : "false");
    if (a.diag && !TLAS) { hipLaunchKernelGGL((k_render_paths<STACK, false, false, true>), grid, dim3(256), lds, s, sc, a, n_pp, rect_bw); return hipGetLastError(); }
    if (stats) hipLaunchKernelGGL((k_render_paths<STACK, true, TLAS>), grid, dim3(256), lds, s, sc, a, n_pp, rect_bw);
    else       hipLaunchKernelGGL((k_render_paths<STACK, false, TLAS>), grid, dim3(256), lds, s, sc, a, n_pp, rect_bw);
    return hipGetLastError();
}

// unsharded raster frames, max_reflect <= 2, stack <= 39 entries; the rectangle DispatchDev::hx0..hy1 is not empty
hipError_t launch_render_paths(const SceneDev& sc, const DispatchDev& a, int stack, bool stats, hipStream_t s)
{
    const uint32_t rect_bw = (a.hx1 - a.hx0) / 8u, rect_bh = (a.hy1 - a.hy0) / 8u;
    const uint32_t n_pp = rect_bw * rect_bh * a.n_frames;
    if (!sc.single_identity) return stack <= 19 ? launch_paths_st<19, true>(sc, a, n_pp, rect_bw, stats, s) : launch_paths_st<39, true>(sc, a, n_pp, rect_bw, stats, s);
    return stack <= 19 ? launch_paths_st<19, false>(sc, a, n_pp, rect_bw, stats, s) : launch_paths_st<39, false>(sc, a, n_pp, rect_bw, stats, s);
}

} // namespace rr
