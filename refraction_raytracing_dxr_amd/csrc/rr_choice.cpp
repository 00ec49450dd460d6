// rr_choice.cpp -- the kernel-choice policy of rr_choice.h
#include "rr_choice.h"

namespace rr {

KernelChoice* ChoiceClass::find(unsigned long long key)
{
    ++clock;
    KernelChoice* lru = &e[0];
    for (KernelChoice& x : e) {
        if (x.valid && x.key == key) { x.stamp = clock; return &x; }
        if (x.stamp < lru->stamp) lru = &x;
    }
    *lru = KernelChoice();
    lru->valid = true; lru->key = key; lru->stamp = clock;
    return lru;
}

const KernelChoice* ChoiceClass::peek(unsigned long long key) const
{
    for (const KernelChoice& x : e) if (x.valid && x.key == key) return &x;
    return nullptr;
}

unsigned long long choice_key(uint32_t width, uint32_t height, const rr_dispatch_params& p, uint32_t depth)
{
    return ((unsigned long long)width << 48) ^ ((unsigned long long)height << 32) ^ ((unsigned long long)(uint32_t)p.max_refract << 8) ^
           ((unsigned long long)(uint32_t)p.max_reflect << 4) ^ (depth <= 2 ? depth : depth < 8 ? 3u : depth < 24 ? 4u : depth < 48 ? 5u : 6u);
}

// a two-level scene whose every node / leaf reference of the pool fits a 16-bit stack entry
static bool pool16(const SceneFacts& s) { return s.pool_nodes < 32768u && s.pool_refs < 32768u; }

KernelPick pick_kernel(const SceneFacts& s, const LaunchFacts& l, const DebugFacts& d)
{
    const bool stream_ok = !s.single_identity && l.max_reflect <= 2 && l.max_refract <= (int)CHOICE_STREAM_MAX_GEN - 2 && pool16(s) &&
                           s.need <= 39 && !l.diag && d.stack == 0 && !d.tlas32;
    // Launches of one or two slices whose scene is small on screen last as long as their most expensive wave: there the path-
    // parallel kernel (four lanes per pixel, a fifth of the longest ray chain) wins -- monkey.obj 1080p Depth 1: 268 us against
    // 471; where the mesh fills the frame its repeated rays lose (sphere.obj 483 us against 263): those stay with k_render_fused.
    const bool paths_ok = !l.compact && l.tile_world == 1 && l.max_reflect <= 2 && s.need <= 39 && d.stack == 0 && l.have_rect && l.depth <= 2;
    // k_render_lds: persistent workgroups, the BLAS's nodes in LDS; unsharded dispatches only, and its ticket arithmetic
    // divides by multiply-high
    const bool lds_ok = s.lds_fits && (uint64_t)l.n_tiles * l.depth * l.depth < 0x40000000ull && !l.compact && !l.mesh;
    KernelPick pk = { K_FUSED, CLS_NONE, K_FUSED, K_FUSED };
    if (d.kernel == 10) { if (stream_ok) pk.kernel = K_STREAM; }
    else if (d.kernel == 5) { if (paths_ok) pk.kernel = K_PATHS; }
    else if (d.kernel == 4) { if (lds_ok) pk.kernel = K_LDS; }
    else if (d.kernel == 0 && !l.diag) {
        if (stream_ok) { pk.cls = CLS_TLAS; pk.cand_b = K_STREAM; }
        else if (paths_ok) { pk.cls = CLS_FEW; pk.cand_b = K_PATHS; }
        else if (lds_ok && l.depth >= 3) {
            // the persistent kernel pays off from about twenty slices a launch (monkey.obj: 1.43 against 1.38 ms at Depth 16,
            // 1.67 / 1.74 at 20, 2.53 / 2.77 at 32, 4.80 / 5.45 at 64; tools/exp_lds_depths.py): from 24 on it is the default, the
            // L1-fed one the alternative
            pk.cls = CLS_MANY;
            if (l.depth >= 24u) { pk.cand_a = K_LDS; pk.cand_b = K_FUSED; } else pk.cand_b = K_LDS;
        }
    }
    if (l.diag && paths_ok && l.rect_share < 0.25 && d.kernel == 0) pk.kernel = K_PATHS;      // (the diagnostic builds keep round 2's rule)
    return pk;
}

int chosen_kernel(const KernelPick& pk, const KernelChoice* ch, double rect_share)
{
    if (pk.cls == CLS_NONE) return pk.kernel;
    const int choice = ch ? ch->choice : 0;
    // (until the measurement: the round-2 rule for launches of one or two slices -- the path-parallel kernel where the scene is small on screen)
    if (choice == 0 && pk.cand_b == K_PATHS && rect_share < 0.25) return K_PATHS;
    return choice == 2 ? pk.cand_b : pk.cand_a;
}

bool measure_due(KernelChoice& ch, double rect_share, bool no_cull)
{
    if (ch.choice != 0 && (rect_share > 2.0 * ch.share || rect_share * 2.0 < ch.share)) { ch.choice = 0; ch.seen = 0; ch.ms[0] = ch.ms[1] = 0.0f; }
    return ch.choice == 0 && !no_cull && ch.seen++ >= 1u;
}

void record_timings(KernelChoice& ch, float ms_a, float ms_b, double rect_share)
{
    // Two measurements, on consecutive dispatches of the shape, decide together (a launch repeats within 1-2 %; k_render_lds
    // against k_render_fused, monkey.obj Depth 64: 2 to 10 % faster launch by launch round the orbit, 6 % over it).  An
    // alternative that is clearly slower the first time is not measured again.
    const bool first = !(ch.ms[0] > 0.0f);
    const float sum_a = ch.ms[0] + ms_a, sum_b = ch.ms[1] + ms_b;
    if (first && ms_b >= 1.02f * ms_a) ch.choice = 1;
    else if (!first) ch.choice = sum_b < 0.98f * sum_a ? 2 : 1;
    ch.ms[0] = sum_a; ch.ms[1] = sum_b;
    ch.share = rect_share;
}

FusedVariant fused_variant(const SceneFacts& s, uint32_t depth, int max_reflect, const DebugFacts& d)
{
    const uint32_t need = s.need;
    int stack = need <= 19 ? 19 : need <= 22 ? 22 : need <= 26 ? 26 : need <= 31 ? 31 : need <= 39 ? 39 : 64;     // rr_render_fused.hip: sizes that fill the LDS with 6 / 5 / 4 / 2 workgroups
    if (d.stack >= (int)need) stack = d.stack;   // experiments only; never below the tree depth (the kernels do not check)
    // deep trees of small meshes: 16-bit stack entries keep eight waves per SIMD (LDS would otherwise allow 6/5/4)
    bool stack16 = s.single_identity && need > 19 && need <= 39 && d.stack == 0 && s.blas_tris < 32768u;
    // two-level scenes: 16-bit entries wherever every node / leaf reference of the pool fits them (RR_DEBUG_TLAS32=1: never)
    if (!s.single_identity && pool16(s) && (need <= 30 || (need <= 39 && depth > 2)) && max_reflect <= 2 && d.stack == 0 && !d.tlas32) stack16 = true;
    // (launches of one or two slices: the ladder above is the faster one at every depth, sphere.obj Depth 1 250 us against 268)
    if (depth <= 2 && s.single_identity) stack16 = false;
    // (the two-level 16-bit-stack builds are sized by the tree itself: 30 entries still leave five workgroups per CU)
    if (!s.single_identity && stack16 && d.stack == 0) stack = (int)need;
    return { stack, max_reflect <= 2 ? 2 : 8, stack16 };
}

uint64_t owned_pixels(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, const rr_mesh_partition* part)
{
    const uint32_t TILE = CHOICE_TILE, tiles_x = (width + TILE - 1) / TILE, n_tiles = tiles_x * ((height + TILE - 1) / TILE);
    auto tile_px = [&](uint32_t t) {
        const uint32_t x0 = (t % tiles_x) * TILE, y0 = (t / tiles_x) * TILE;
        const uint32_t w = width - x0 < TILE ? width - x0 : TILE, h = height - y0 < TILE ? height - y0 : TILE;
        return (uint64_t)w * h;
    };
    uint64_t px = 0;
    if (!part) for (uint32_t t = rank; t < n_tiles; t += world) px += tile_px(t);
    else
        for (uint32_t t = 0; t < n_tiles; ++t) {
            const uint32_t tx = t % tiles_x, ty = t / tiles_x;
            const bool in_rect = part->rect_w == 0 || (tx >= part->rect_x0 && tx < part->rect_x0 + part->rect_w && ty >= part->rect_y0 && ty < part->rect_y0 + part->rect_h);
            const uint32_t i = part->rect_w == 0 ? t : (ty - part->rect_y0) * part->rect_w + (tx - part->rect_x0);
            uint32_t owner = 0, slot = 0;
            if (in_rect) (void)rr_host_mesh_tile_home(part, i, &owner, &slot);
            if (in_rect ? owner == rank : rank == 0) px += tile_px(t);
        }
    return px;
}

} // namespace rr
