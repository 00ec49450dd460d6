// rr_choice.h -- which render kernel renders a dispatch: plain C++, no HIP (tests/test_kernel_choice.py).  Neither k_render_fused
// nor a class's alternative wins everywhere (1080p orbits: k_render_lds 6 % ahead on sphere.obj, 2 % behind on monkey.obj: it
// depends on how busy the texture path is, which the host cannot see).  So it is MEASURED per scene and launch shape: a
// class's first dispatch of a shape renders on the default (clocks come up), the next one or two are rendered by both
// candidates between HIP events (bit-identical frames, three extra launches), and from then on the alternative renders the
// shape only if it took under 98 % of the default's time over both.  rr_build_tlas starts afresh; a shape (choice_key: frame
// size, bounce limits, launch depth 1 / 2 / 3-7 / 8-23 / 24-47 / 48+) keeps its choice -- a class remembers its four most
// recent shapes -- until its rectangle share doubles or halves.  Classes: two-level scenes (fused / k_stream_*), many slices of
// the reference's scene (fused / k_render_lds), one or two slices (fused / k_render_paths).  rr_capi_dispatch.cpp gathers the facts
// (pick_launch), times the candidates and launches; every rule is stated here.
#pragma once
#include <cstdint>
#include "../../include/rrdxr.h"
namespace rr {
constexpr uint32_t CHOICE_TILE = 32, CHOICE_STREAM_MAX_GEN = 64;     // rr_types.h's (HIP types there; rr_capi.cpp checks)
enum RenderKernel { K_FUSED = 0, K_LDS = 1, K_PATHS = 2, K_STREAM = 7 };         // rr_stats::render_kernel
enum ChoiceClassId { CLS_NONE = -1, CLS_TLAS = 0, CLS_MANY = 1, CLS_FEW = 2 };

// a launch shape's choice: 0 undecided, 1 candidate A (the default), 2 candidate B; the dispatches of the shape seen; the
// rectangle share of the frame and the two candidates' summed times at the measurement; LRU stamp
struct KernelChoice {
    int choice = 0; uint32_t seen = 0; unsigned long long key = 0; double share = 0.0; float ms[2] = { 0.0f, 0.0f };
    bool valid = false; unsigned long long stamp = 0;
};

struct ChoiceClass {
    KernelChoice e[4]; unsigned long long clock = 0;
    KernelChoice* find(unsigned long long key);               // the shape's entry; a new shape takes the place of the least recently used
    const KernelChoice* peek(unsigned long long key) const;   // the shape's entry or null; changes nothing
};
unsigned long long choice_key(uint32_t width, uint32_t height, const rr_dispatch_params& p, uint32_t depth);

// The scene: one identity instance?, deepest stack it can need, that instance's BLAS triangles, or a two-level pool's nodes
// and leaf references; lds_fits: one identity instance whose nodes fit LDS beside the stacks (lds_kernel_shape).
struct SceneFacts { bool single_identity; uint32_t need, blas_tris, pool_nodes, pool_refs; bool lds_fits; };
// The launch: slices, tiles of one slice, tile world; compact: tile output; mesh: the mesh-tile partition; the scene's screen
// rectangle (seen at all, its share of the frame); bounce limits; RR_DISPATCH_DEBUG_NO_CULL; diag: RR_DEBUG_DIAG records it.
struct LaunchFacts { uint32_t depth, n_tiles, tile_world; bool compact, mesh, have_rect; double rect_share; int max_refract, max_reflect; bool no_cull, diag; };
// RR_DEBUG_KERNEL (0 measured choice, 1 "fused", 4 "lds", 5 "paths", 10 "stream"), RR_DEBUG_STACK, RR_DEBUG_TLAS32
struct DebugFacts { int kernel, stack; bool tlas32; };

// the launch's kernel before any measurement, and its class with the default (a) and the alternative (b) if it has one
struct KernelPick { int kernel; int cls; int cand_a, cand_b; };
KernelPick pick_kernel(const SceneFacts& s, const LaunchFacts& l, const DebugFacts& d);
// the kernel that renders the launch given its shape's entry (null: nothing measured yet)
int chosen_kernel(const KernelPick& pk, const KernelChoice* ch, double rect_share);
// does this dispatch measure?  Renews a choice whose rectangle share doubled or halved and counts the shape's dispatches
bool measure_due(KernelChoice& ch, double rect_share, bool no_cull);
// the two candidates' times of one measurement (a: the default)
void record_timings(KernelChoice& ch, float ms_a, float ms_b, double rect_share);
// k_render_fused's instantiation: stack entries, parked-ray slots and 16-bit stack entries
struct FusedVariant { int stack, pend; bool stack16; };
FusedVariant fused_variant(const SceneFacts& s, uint32_t depth, int max_reflect, const DebugFacts& d);

// The ray-tree kernels (k_shade_rays, k_render_samples, k_adaptive_base / _refine: ray_tree on a lane behind a RayGen of their own)
// are built as <STACK, PEND, TLAS, E>: stack entries, parked-ray slots, two-level scene, stack entry type.  TreeVariant names one
// instantiation, as a tag a generic lambda takes; a workgroup's four stacks take lds_bytes of LDS.
template <int STACK, int PEND, bool TLAS, class E> struct TreeVariant {
    static constexpr int stack = STACK, pend = PEND;
    static constexpr bool tlas = TLAS;
    using entry = E;
    static constexpr uint32_t lds_bytes = 4u * STACK * 64u * sizeof(E);
};
template <int STACK, int PEND, class F> auto tree_variant32(bool single_identity, F&& f)
{
    return !single_identity ? f(TreeVariant<STACK, PEND, true, uint32_t>{}) : f(TreeVariant<STACK, PEND, false, uint32_t>{});
}
// The one ladder of those kernels: f(TreeVariant) of the instantiation that runs a scene's FusedVariant (stack <= 64, pend <= 8: the
// launchers check) -- launch_render_fused's ladder without its 22-entry rung (seven waves per SIMD against six: DESIGN 5.5).  20
// instantiations in all; tests/test_kernel_choice.py walks every rung.  The other ladders stay where they are: launch_render_fused's
// has that rung and branches on its diag and stats builds with waves per SIMD of its own per rung (rr_render_fused.hip); the trace, query
// and multi-hit kernels are <STACK, TLAS> builds of two stack sizes without parked rays, two lines each.
template <class F> auto for_tree_variant(bool single_identity, FusedVariant v, F&& f)
{
    const bool si = single_identity;
    if (v.stack16 && !si && v.pend <= 2 && v.stack <= 30) return f(TreeVariant<30, 2, true, uint16_t>{});
    if (v.stack16 && !si && v.pend <= 2 && v.stack <= 39) return f(TreeVariant<39, 2, true, uint16_t>{});
    if (v.stack16 && si && v.stack <= 39) return v.pend <= 2 ? f(TreeVariant<39, 2, false, uint16_t>{}) : f(TreeVariant<39, 8, false, uint16_t>{});
    if (v.stack <= 19 && v.pend <= 2) return tree_variant32<19, 2>(si, f);
    if (v.stack <= 26 && v.pend <= 2) return tree_variant32<26, 2>(si, f);
    if (v.stack <= 31) return v.pend <= 2 ? tree_variant32<31, 2>(si, f) : tree_variant32<31, 8>(si, f);
    if (v.stack <= 39) return v.pend <= 2 ? tree_variant32<39, 2>(si, f) : tree_variant32<39, 8>(si, f);
    return v.pend <= 2 ? tree_variant32<64, 2>(si, f) : tree_variant32<64, 8>(si, f);
}
// pixels of one slice that rank `rank` renders (edge tiles counted exactly): round robin tiles, or the mesh partition's
uint64_t owned_pixels(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, const rr_mesh_partition* part);

} // namespace rr
