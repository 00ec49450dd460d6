// rr_render_lds.hip -- k_render_lds: the renderer for meshes whose BLAS fits the LDS.
//
// The same renderer with the BLAS's nodes in LDS, for meshes whose whole node array fits beside the traversal stacks
// (the reference's meshes up to shell.obj: 24-49 KB of QNodes).  Persistent workgroups of NW waves: each copies the node
// array into its LDS once, then its waves draw tickets -- a few 8x8 pixel blocks each, shared inside the workgroup -- from
// counters until none are left.  Why: in the L1-fed kernel the texture addresser / L1 / data-return path is the
// busiest unit after the VALU (TA 84 %, TD 97 % busy, 276 cycles per request; waves spend 53 % of their life in s_waitcnt:
// profiles/r02_pmc_fused.txt); a divergent 32-byte node costs the CU's L1 56 cycles and its LDS 25 (tools/ubench_nodefetch.hip),
// and a lone wave's trip shrinks from an L1 round trip to an LDS one, which is what the tail of a Depth-1 launch is made of.
// Order of work (LdsDispatch): first the screen rectangle of the mesh in 32x8 strips, then everything else in 32x32 tiles.
// Tickets come from n_queues counters per phase (rr_types.h); a wave whose own queue is empty drains the others, so every
// block is rendered whatever the placement of workgroups is.
// NW waves per workgroup, WGS workgroups per CU (NW * WGS / 4 waves per SIMD); stack entries are 16 bits (node index or
// ~leaf index: an LDS-resident array has fewer than 5 120 nodes).  After the last block the last wave to leave
// zeroes the ticket words, so the next launch on the same slot needs no memset.
// k_render_lds renders unsharded dispatches only, and its blocks come from its own two phases: no tile partitions, no launch
// order of tiles -- every scalar that stays live across the renderer is one that may end up being moved through vector lanes.
#include <hip/hip_runtime.h>
#include "rr_render_common.h"

namespace rr {

// block j (0..15, row-major 8x8 blocks) of phase 2 ticket u = tile * n_frames + slice
// (divisions by launch constants are a multiply-high with a reciprocal from the host: a scalar division would be done in the
// vector unit, twenty-odd instructions each)
__device__ __forceinline__ BlockPos lds_tile_block(const DispatchDev& a, const LdsDispatch& q, uint32_t u, uint32_t j)
{
    BlockPos p;
    const uint32_t tile = a.n_frames == 1u ? u : __umulhi(u, q.div_frames);
    p.frame = u - tile * a.n_frames;
    p.tile_local = tile;
    p.tile_ok = tile < a.n_local_tiles;
    p.bg = false;
    const uint32_t ty = a.tiles_x == 1u ? tile : __umulhi(tile, q.div_tiles_x), tx = tile - ty * a.tiles_x;
    p.px0 = (j & 3u) * 8u; p.py0 = (j >> 2) * 8u;
    p.x0 = tx * TILE + p.px0; p.y0 = ty * TILE + p.py0;
    return p;
}

// block j (0..3) of phase 1 ticket u = strip * n_frames + slice: strip = a 32x8 run of the scene's screen rectangle, row-major
__device__ __forceinline__ BlockPos lds_rect_block(const DispatchDev& a, const LdsDispatch& q, uint32_t u, uint32_t j)
{
    BlockPos p;
    const uint32_t strip = a.n_frames == 1u ? u : __umulhi(u, q.div_frames), per_row = q.rect_bw >> 2;
    p.frame = u - strip * a.n_frames;
    const uint32_t row = per_row == 1u ? strip : __umulhi(strip, q.div_per_row), col = strip - row * per_row;
    p.tile_local = 0u; p.tile_ok = true; p.bg = false;
    p.px0 = 0u; p.py0 = 0u;
    p.x0 = q.rx0 + col * 32u + j * 8u; p.y0 = q.ry0 + row * 8u;
    return p;
}

template <int NW, int WGS, bool STATS, bool DIAG = false>
__global__ __launch_bounds__(NW * 64, NW * WGS / 4) void k_render_lds(SceneDev sc, DispatchDev a, LdsDispatch q)
{
    typedef uint16_t E;
    __shared__ uint32_t diag_tr[3 * 16];        // diagnostic builds: per wave internal trips, leaf trips, shading passes
    __shared__ uint32_t wg_arrived;             // waves of this workgroup that have finished
    __shared__ unsigned long long wg_share[16]; // per wave: ((ticket + 1) | tile << 31) << 32 | next block of the ticket it drew that is still to be rendered
    if (threadIdx.x == 0) wg_arrived = 0u;      // (ordered before its first use by the barrier behind the node copy)
    if (threadIdx.x < 16) wg_share[threadIdx.x] = 0ull;
    const unsigned long long diag_t0 = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
    unsigned long long diag_wait = 0ull, diag_render = 0ull, diag_n = 0ull;       // cycles in ticket draws / in blocks, tickets | blocks << 32
    unsigned long long diag_worst = 0ull, diag_worst_trips = 0ull;                // the wave's longest block: cycles, its trips (I | L << 20 | S << 40)
    if (DIAG && threadIdx.x < 48) diag_tr[threadIdx.x] = 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    {   // the BLAS's nodes -> LDS (q.node_bytes is a multiple of 32)
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(sc.blas0.nodes);
        uint4* dst = reinterpret_cast<uint4*>(lds);
        for (uint32_t i = threadIdx.x; i < q.node_bytes / 16u; i += NW * 64) dst[i] = src[i];
    }
    __syncthreads();
    const unsigned long long diag_t1 = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;      // wave: uniform, so that everything derived from it is scalar
    const LdsNodes ns{ reinterpret_cast<const char*>(lds) };
    MemPark park{ q.park + (size_t)(blockIdx.x * NW + wave) * ((size_t)q.park_slots * 8 * 64) + lane };
    E* stk = reinterpret_cast<E*>(reinterpret_cast<char*>(lds) + q.node_bytes) + wave * (q.stack_entries * 64u) + lane;
    const uint32_t lx = compact1by1(lane), ly = compact1by1(lane >> 1);

    LaneStats st;
    stats_clock_begin<STATS>(st);
    auto in_rect = [&](const BlockPos& bp) { return bp.x0 >= q.rx0 && bp.x0 < q.rx1 && bp.y0 >= q.ry0 && bp.y0 < q.ry1; };
    // The wave's work loop.  Everything that decides WHICH block comes next is wave-uniform (scalar); the renderer itself is
    // instantiated once, at the bottom of the loop (its code is ~10 KB: several inlined copies thrash the instruction cache).
    // a wave's own queue: its XCD's number (queue i holds tickets i, i + n_queues, ...: with eight queues an XCD keeps to
    // every eighth strip and slice, which its L2 rewards -- monkey.obj Depth 64, 90 us per frame against 104 with queues
    // entered by wave number)
    const uint32_t NQ = q.n_queues;
    uint32_t home = (blockIdx.x * NW + wave) % NQ;
    if (q.home_xcc) { uint32_t xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc)); home = (xcc & 7u) % NQ; }
    // Little scalar state on purpose: the renderer below keeps ~70 scalars live, and what does not fit the scalar registers is
    // moved through vector lanes -- vector instructions (the first form of this loop, which looked through 64 counters at a
    // time and kept a strip's BlockPos, cost 491 of them in 1 362).
    uint32_t phase = 0, qi = home, tried = 0;  // tried: queues of this phase the wave has found empty
    for (;;) {
        BlockPos bp;
        bool have = false;
        while (!have) {
            // A ticket is several blocks next to each other, which share triangles and texels in the CU's L1: a 32x8 strip of the
            // scene's screen rectangle in phase 1, a whole 32x32 tile of what lies outside it in phase 2 (the background costs a
            // microsecond per block: eight counters hand out ~600 tickets per microsecond, and tickets of four blocks had the
            // background phases ask for twice that).  One wave rendering a ticket's blocks one after the other would be a chain
            // that many blocks long, and a launch cannot end before its longest chain has (1 ms on monkey.obj, on top of every
            // launch, when this kernel did that).  So the wave that draws a ticket keeps its first block and leaves the others in
            // its slot of wg_share for whichever wave of the workgroup needs a block next -- its own slot first, then the others':
            // one LDS read of all slots, one LDS atomic.
            {
                uint32_t got = 0xffffffffu, got_u = 0u;
                for (;;) {                                      // (again only after losing a block to another wave)
                    const unsigned long long mine = lane < (uint32_t)NW ? wg_share[lane] : 0ull;      // every slot at once, one per lane
                    const uint32_t mh = (uint32_t)(mine >> 32);
                    const unsigned long long m = __ballot(mh != 0u && (uint32_t)mine < ((mh & 0x80000000u) ? 16u : 4u));
                    if (m == 0ull) break;
                    const unsigned long long from_own = m >> wave << wave;                       // the wave's own slot first, then the next ones
                    const uint32_t sl = (uint32_t)__ffsll((long long)(from_own ? from_own : m)) - 1u;
                    unsigned long long v = 0ull;
                    if (lane == 0) v = atomicAdd(&wg_share[sl], 1ull);
                    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
                    if (hi != 0u && lo < ((hi & 0x80000000u) ? 16u : 4u)) { got = lo; got_u = hi; break; }
                }
                if (got != 0xffffffffu) {
                    if (got_u & 0x80000000u) { bp = lds_tile_block(a, q, (got_u & 0x7fffffffu) - 1u, got); have = bp.tile_ok && !in_rect(bp); }
                    else { bp = lds_rect_block(a, q, got_u - 1u, got); have = true; }
                    continue;
                }
            }
            if (phase >= 2u) break;
            const uint32_t total = phase == 0u ? q.p1_tickets : q.p2_tickets;
            uint32_t* const cnt = q.tickets + phase * LDS_QUEUES * 16u;
            bool drew = false;
            uint32_t u = 0;
            while (total != 0u && tried < NQ) {
                const uint32_t n_tickets = total > qi ? (total - qi + NQ - 1u) / NQ : 0u;   // tickets qi, qi + NQ, ...
                // a queue other than the wave's own is looked at before it is drawn from (a counter only ever grows: a queue
                // seen empty stays empty), so the waves that find everything drained add no atomics to the last ones' wait
                uint32_t seen = 0u;
                if (tried != 0u) {
                    if (lane == 0) seen = __hip_atomic_load(&cnt[qi * 16u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    seen = __builtin_amdgcn_readfirstlane(seen);
                }
                if (seen < n_tickets) {
                    uint32_t t = 0;
                    const unsigned long long dw0 = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
                    if (lane == 0) t = atomicAdd(&cnt[qi * 16u], 1u);
                    t = __builtin_amdgcn_readfirstlane(t);
                    if (DIAG) { diag_wait += __builtin_amdgcn_s_memtime() - dw0; diag_n += 1ull; }
                    if (t < n_tickets) { u = qi + NQ * t; drew = true; break; }
                }
                ++tried;
                qi = qi + 1u == NQ ? 0u : qi + 1u;
            }
            if (!drew) { ++phase; qi = home; tried = 0u; continue; }
            // block 0 of the ticket is this wave's, the rest is for the workgroup
            if (phase == 0u) {
                if (lane == 0) wg_share[wave] = ((unsigned long long)(u + 1u) << 32) | 1ull;
                bp = lds_rect_block(a, q, u, 0u);
                have = true;
            } else {
                if (lane == 0) wg_share[wave] = ((unsigned long long)((u + 1u) | 0x80000000u) << 32) | 1ull;
                bp = lds_tile_block(a, q, u, 0u);
                have = bp.tile_ok && !in_rect(bp);
            }
        }
        if (!have) break;
        st.blocks += 1u;
        const unsigned long long dr0 = DIAG ? __builtin_amdgcn_s_memtime() : 0ull;
        const uint32_t dI0 = DIAG ? diag_tr[wave] : 0u, dL0 = DIAG ? diag_tr[16 + wave] : 0u, dS0 = DIAG ? diag_tr[32 + wave] : 0u;
        const uint32_t x = bp.x0 + lx, y = bp.y0 + ly;
        const bool may_hit = bp.x0 + 8u > a.hx0 && bp.x0 < a.hx1 && bp.y0 + 8u > a.hy0 && bp.y0 < a.hy1;
        if (STATS && !may_hit) st.bg_blocks += 1u;
        if (x < a.W && y < a.H) {
            const CamDev& cb = a.cams[bp.frame];
            st.pixels += 1;
            const f3 acc = render_pixel<STATS, false, DIAG, E, LdsNodes>(sc, a, cb, x, y, may_hit, stk, ns, park, st, Diag{ DIAG ? &diag_tr[wave] : nullptr, 16 });
            const size_t o = a.compact_out == 0u ? (size_t)y * a.W + x
                                                : (size_t)bp.tile_local * (TILE * TILE) + (bp.py0 + ly) * TILE + (bp.px0 + lx);
            store_pixel(a, a.out_rgba8 + (size_t)bp.frame * a.frame_stride,
                        a.out_f32 ? a.out_f32 + (size_t)bp.frame * a.frame_stride : nullptr, o, acc);
        }
        if (DIAG) {
            const unsigned long long dt = __builtin_amdgcn_s_memtime() - dr0;
            diag_render += dt; diag_n += 1ull << 32;
            if (dt > diag_worst) {
                diag_worst = dt;
                diag_worst_trips = (unsigned long long)(diag_tr[wave] - dI0) | ((unsigned long long)(diag_tr[16 + wave] - dL0) << 20) |
                                   ((unsigned long long)(diag_tr[32 + wave] - dS0) << 40);
            }
        }
    }
    if (DIAG && lane == 0) {
        unsigned long long* d = a.diag + (size_t)(blockIdx.x * NW + wave) * 8;
        d[0] = diag_wait; d[1] = diag_render; d[2] = diag_n; d[3] = __builtin_amdgcn_s_memtime() - diag_t0;
        d[4] = diag_worst; d[5] = diag_worst_trips; d[6] = diag_t1 - diag_t0; d[7] = diag_tr[wave] | ((unsigned long long)diag_tr[16 + wave] << 32);
    }
    flush_stats<STATS>(a, st, blockIdx.x * NW + wave, lane);
    // Every ticket a wave drew came back before it arrives here, so the last workgroup to arrive sees all queues drained and
    // zeroes the words for the next launch.  One arrival per workgroup (its waves count in LDS first): one per wave would be
    // 6 144 atomics on one word.
    if (lane == 0) {
        const uint32_t w_arrived = atomicAdd(&wg_arrived, 1u);
        if (w_arrived + 1u == (uint32_t)NW) {
            const uint32_t arrived = atomicAdd(&q.tickets[2u * LDS_QUEUES * 16u], 1u);
            if (arrived + 1u == gridDim.x) {
                for (uint32_t k = 0; k <= 2u * LDS_QUEUES; ++k) atomicExch(&q.tickets[k * 16u], 0u);
            }
        }
    }
}

// ------------------------------------------------------------------------------------ launchers
// Workgroup shapes of k_render_lds; a shape fits when the node array plus its stacks fit the CU's LDS WGS times (limit per
// workgroup: 160 KiB / WGS, less a little for the allocation granule).  12 waves x 2 workgroups (6 waves per SIMD, 80
// registers) is the one that pays: 16 x 2 (8 waves, 64 registers) spills 28 words per lane and 8 192 waves' scratch no
// longer fits the L2 (monkey.obj Depth 64: 90 us per frame against 83), 16 x 1 leaves 4 waves per SIMD (109 us).
constexpr struct { int nw, wgs; } LDS_SHAPES[] = { { 12, 2 }, { 16, 2 }, { 16, 1 } };
// dynamic LDS of a workgroup of shape i: the node array, then a stack of 16-bit entries per lane
static size_t lds_shape_bytes(int i, uint32_t node_bytes, uint32_t stack_entries) { return (size_t)node_bytes + (size_t)LDS_SHAPES[i].nw * stack_entries * 64 * sizeof(uint16_t); }

int lds_kernel_shape(uint32_t node_bytes, uint32_t stack_entries, size_t* lds_bytes, int min_shape)
{
    for (int i = min_shape < 0 ? 0 : min_shape; i < 3; ++i) {
        const size_t need = lds_shape_bytes(i, node_bytes, stack_entries);
        if (need <= (size_t)(160 * 1024) / LDS_SHAPES[i].wgs - 512) { if (lds_bytes) *lds_bytes = need; return i; }
        if (min_shape <= 0) break;       // product path: the first shape or none
    }
    return -1;
}

template <int SHAPE, bool STATS, bool DIAG = false>
static hipError_t launch_lds_nw(const SceneDev& sc, const DispatchDev& a, const LdsDispatch& q, int n_cus, hipStream_t s)
{
    constexpr int NW = LDS_SHAPES[SHAPE].nw, WGS = LDS_SHAPES[SHAPE].wgs;
    // more than 64 KB of dynamic LDS has to be asked for, once per instantiation
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_render_lds<NW, WGS, STATS, DIAG>), hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    if (attr != hipSuccess) return attr;
    if (!DIAG) set_render_kernel_name("k_render_lds<%d, %d, %s, false>", NW, WGS, STATS ? "true" : "false");
    hipLaunchKernelGGL((k_render_lds<NW, WGS, STATS, DIAG>), dim3((uint32_t)n_cus * WGS), dim3(NW * 64), lds_shape_bytes(SHAPE, q.node_bytes, q.stack_entries), s, sc, a, q);
    return hipGetLastError();
}

hipError_t launch_render_lds(const SceneDev& sc, const DispatchDev& a, LdsDispatch q, int n_cus, bool stats, hipStream_t s, int min_shape)
{
    if (a.n_blocks == 0) return hipSuccess;
    const int shape = lds_kernel_shape(q.node_bytes, q.stack_entries, nullptr, min_shape);
    if (shape < 0) return hipErrorInvalidValue;
    {   // one queue per workgroup of the shape that will run (never more than LDS_QUEUES)
        const uint32_t grid = (uint32_t)n_cus * (uint32_t)LDS_SHAPES[shape].wgs;
        if (q.n_queues > grid) q.n_queues = grid;
        if (q.n_queues > LDS_QUEUES) q.n_queues = LDS_QUEUES;
        if (q.n_queues < 1u) q.n_queues = 1u;
    }
    q.p2_tickets = a.n_local_tiles * a.n_frames;        // phase 2: one 32x32 tile of one slice per ticket (blocks inside the rectangle are skipped)
    // phase 1: the rectangle, widened to whole 32-pixel columns, in 32x8 strips of one slice each
    if (q.rx1 > q.rx0 && q.ry1 > q.ry0) {
        q.rx0 &= ~31u;
        q.rx1 = (q.rx1 + 31u) & ~31u;
    }
    const bool rect = q.rx1 > q.rx0 && q.ry1 > q.ry0;
    q.rect_bw = rect ? (q.rx1 - q.rx0) / 8u : 0u;
    q.p1_tickets = !rect ? 0u : (q.rect_bw / 4u) * ((q.ry1 - q.ry0) / 8u) * a.n_frames;
    if ((uint64_t)q.p2_tickets * a.n_frames >= 0xffffffffull || (uint64_t)q.p1_tickets * a.n_frames >= 0xffffffffull) return hipErrorInvalidValue;   // (multiply-high divisions)
    q.div_frames = (uint32_t)(0x100000000ull / a.n_frames) + 1u;
    q.div_tiles_x = (uint32_t)(0x100000000ull / a.tiles_x) + 1u;
    q.div_per_row = rect ? (uint32_t)(0x100000000ull / (q.rect_bw / 4u)) + 1u : 0u;
    static_assert(sizeof LDS_SHAPES / sizeof LDS_SHAPES[0] == 3, "lds_kernel_shape and the rungs below");
    if (a.diag) return launch_lds_nw<0, false, true>(sc, a, q, n_cus, s);       // diagnostic build (RR_DEBUG_DIAG): per-wave cycles in ticket draws and in blocks; the product shape
    if (shape == 0) return stats ? launch_lds_nw<0, true>(sc, a, q, n_cus, s) : launch_lds_nw<0, false>(sc, a, q, n_cus, s);
    if (shape == 1) return stats ? launch_lds_nw<1, true>(sc, a, q, n_cus, s) : launch_lds_nw<1, false>(sc, a, q, n_cus, s);
    return stats ? launch_lds_nw<2, true>(sc, a, q, n_cus, s) : launch_lds_nw<2, false>(sc, a, q, n_cus, s);
}

} // namespace rr
