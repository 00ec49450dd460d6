// rr_render_shadows.h -- the shadow ray of the transparent-shadow kernels (k_shade_rays_shadows and k_render_shadows in
// rr_render_surfaces.hip, k_render_lit_shadows in rr_render_lit.hip): the WALK form of ray_tree_surfaces_two_site
// (rr_render_surfaces.h) puts shadow_walk where step b's first-hit ray stands -- a straight WALK through the glass between the opaque
// hit and the light, attenuated by what it crosses and stopped only by an opaque surface.  Opt-in: the context's shadow_steps
// (rr_set_shadow_steps) is K, 0 <= K <= RR_SHADOW_MAX_STEPS = 16; with K == 0 the launchers run the first-hit kernels and nothing here
// is reached.
//
// Everything in rr_render_surfaces.h's contract stands but the shadow ray of step b.  With K >= 1, for a light the hit faces
// (cs > 0; Ld, far, g from light_at as before) -- one rounding per written operation, fmaf only where written:
//   start   T = (1, 1, 1), Ls = L (the media list of the radiance ray at the hit), Xs = X, fs = far.
//   each of up to K calls
//           TraceRay(Xs, Ld, [tmin_secondary, fs], cull flags 0, closest hit, InstanceInclusionMask = shadow_mask), counted in n_rays.
//           Miss: the walk ends LIT.
//           Hit on a row whose surface kind is opaque: the walk ends OCCLUDED, the light adds nothing.
//           Hit on a glass row m at t:
//             1. c = top(Ls); if c is not air, T.ch = T.ch * rr_expf_neg(-(sigma_c.ch * t))     (absorb_crossed: the medium CROSSED)
//             2. Ls = front ? push(Ls, m) : remove(Ls, m)     (media_push / media_remove: a push onto a full list is dropped, removing
//                an absent row is a no-op; front is the HitKind, as in the nested tree)
//             3. Xs.ch = fmaf(t, Ld.ch, Xs.ch), fs = fs - t
//             4. !(fs > tmin_secondary): the walk ends LIT
//             5. this was the K-th call: the walk ends OCCLUDED -- the cap is conservative.
//   lit     f = cs * g, E.ch = fmaf(radiance.ch, f * T.ch, E.ch).
// A scene without a top level walks its one instance (mask 1, row mat0) the same way if shadow_mask & 1; otherwise the first call
// misses.
//
// Reductions, byte for byte in colours, RGBA8 and ray counts:
//   any K  equals the tree's first-hit form wherever no shadow ray's first hit is glass: a first call that misses or stops on an
//          opaque row is the first-hit ray's answer, and f * 1.0f == f.
//   K = 1  equals it on every scene but for one corner, which step 4 standing before step 5 leaves: a glass hit closer than
//          tmin_secondary to the far end of its interval ends the walk lit where the first-hit ray is occluded.
//
// Not modelled: Fresnel loss and bending at the interfaces the walk crosses (no normal is fetched: the walk is straight and keeps
// all of its weight but the absorption); absorption beyond the last hit, for a light that stands inside a medium; caustics (a lit
// surface receives no light that was refracted or reflected on its way).
//
// The shape.  The walk is a second trace_scene<..., QUERY = true> site with any_lane = false, inside a loop whose bound K is a
// kernel argument and so wave-uniform; a lane leaves the loop at its own call and the wave reconverges behind it, as it does behind
// the first-hit site of the two-site tree.  The walk's hit record, HitRecWalk, keeps what the walk reads -- t, the instance (for the
// row) and the HitKind -- and skips u, v and the normal, as HitRecShadow skips everything.  Its state (T, Ls, Xs, fs) is eight
// registers that live across the walk's traversals beside X, Nf, E and the radiance ray; DESIGN 5.17 has the code object's figures.
// The traversal stack is free while a hit is shaded, so the walk uses the same LDS column.
#pragma once
#include "rr_render_surfaces.h"

namespace rr {

// The hit record of a walk's call: HitRec's walk (hits_begin, hit_bound, leaf_test and hit_found bind to HitRec's overloads), and of
// the attributes only the face: the sign of hit_attributes' det, from the same operations in the same order, without U, V and ad
struct HitRecWalk : HitRec { bool front; };
__device__ __forceinline__ float face_det(const TriRec* __restrict__ tris, uint32_t leaf, f3 D)
{
    const float4* q = reinterpret_cast<const float4*>(tris + leaf);
    const float4 b = q[1], c = q[2];
    return dot3(mk3(b.x, b.y, b.z), cross3(D, mk3(c.x, c.y, c.z)));
}
__device__ __forceinline__ void hits_end_blas(const TriRec* __restrict__ tris, f3, f3 D, HitRecWalk& best)
{
    best.front = false;
    if (best.hit) best.front = face_det(tris, best.leaf, D) > 0.0f;
}
__device__ __forceinline__ void hits_end_scene(const SceneDev& sc, f3, f3 D, HitRecWalk& best)
{
    best.front = false;
    if (best.hit) {
        const InstDev in = inst_record(sc.insts, best.inst);
        f3 Dh = D;
        if (!in.identity) Dh = xform_dir(in.inv, D);
        best.front = (face_det(sc.pool_tris, best.leaf, Dh) > 0.0f) != ((in.flags & 0x2u) != 0u);
    }
}

// The walk of one light from X towards Ld over [a.tmin_s, far], at most K calls (K >= 1, wave-uniform); L: the radiance ray's list
// at the hit; mask: the light's shadow_mask (& 1 without a top level).  True: lit, and T is what the glass let through
template <bool TLAS, class E>
__device__ __forceinline__ bool shadow_walk(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf, uint32_t mat0,
                                            uint32_t K, uint32_t mask, f3 X, f3 Ld, float far, uint32_t L, E* stk, LaneStats& st, f3& T)
{
    T = mk3(1.0f, 1.0f, 1.0f);
    f3 Xs = X;
    float fs = far;
    uint32_t Ls = L;
    for (uint32_t k = 0; k < K; ++k) {
        HitRecWalk hs;
        trace_scene<false, TLAS, E, GlobalNodes, true, HitRecWalk>(sc, Xs, Ld, a.tmin_s, fs, 0u, hs, stk, st.cnt, Diag{ nullptr }, GlobalNodes{}, mask,
                                                                   false);
        ++st.rays;
        if (!hs.hit) return true;
        const uint32_t row = hit_material<TLAS>(sc, hs, mat0);
        if (row < sf.n && sf.rows[row].kind == SURFACE_OPAQUE) return false;
        const uint32_t c = media_top(Ls);
        if (c) absorb_crossed(mats, c, hs.t, T);
        Ls = hs.front ? media_push(Ls, row + 1u) : media_remove(Ls, row + 1u);
        Xs = mk3(fmaf(hs.t, Ld.x, Xs.x), fmaf(hs.t, Ld.y, Xs.y), fmaf(hs.t, Ld.z, Xs.z));
        fs = fs - hs.t;
        if (!(fs > a.tmin_s)) return true;
    }
    return false;                                             // the cap
}

} // namespace rr
