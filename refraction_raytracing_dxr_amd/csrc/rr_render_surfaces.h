// rr_render_surfaces.h -- the ray tree of the surface kernels (rr_render_surfaces.hip): shade_ray_nested and ray_tree_nested of
// rr_render_nested.h with a second hit group.  Row m of the surface table (rr_set_surfaces) says what an instance of material row m
// is: glass, shaded by rr_render_nested.h's ClosestHit, or an opaque surface lit by the context's lights through shadow rays.  Rows
// at or beyond the table's length are glass.
//
// Everything in rr_render_nested.h's contract stands, step 1 included: absorption over t in the medium CROSSED comes first.  After
// it, a hit with count < max_refract on a row whose kind is SURFACE_OPAQUE does this instead of steps 2-5 (one rounding per written
// operation, fmaf only where written, dot = dot3):
//   a. L is unchanged.  X = fmaf(t, D, O); N the shading normal; Nf = front ? N : -N.
//   b. E = ambient; then for each light in table order
//        directional: Ld = v, far = tmax_secondary, g = 1
//        point:       d = v - X, d2 = dot(d, d), far = sqrtf(d2), Ld = d / far, g = 1.0f / d2
//        cs = dot(Nf, Ld); !(cs > 0): the light adds nothing and NO ray is traced.  Otherwise one shadow ray,
//        TraceRay(X, Ld, [tmin_secondary, far], cull flags 0, ACCEPT_FIRST_HIT_AND_END_SEARCH, InstanceInclusionMask = shadow_mask),
//        counted in n_rays whether or not an instance passes the mask; any accepted hit occludes, glass included.  Unoccluded:
//        f = cs * g, E.ch = fmaf(radiance.ch, f, E.ch).
//   c. col.ch = fmaf(albedo.ch, E.ch, emission.ch); acc.ch = fmaf(w.ch, col.ch, acc.ch).
//   d. any specular.ch != 0: one child (X, normalize(ReflectRay(D, Nf)), w.ch * specular.ch, L, count + 1) on the secondary
//      interval.  It is the continuing ray: nothing is parked, and max_reflect does not gate it -- count alone bounds it, so
//      ray_tree's bound (count grows by one per level) stands.  Otherwise the branch ends and a parked ray is popped, as after a Miss.
// A scene without a top level shades its one instance (mask 1, row mat0) the same way; its shadow ray passes if shadow_mask & 1.
//
// Reduction: with no table, or with every row glass, no lane takes the opaque branch, the lights are never read and the tree is
// ray_tree_nested's operation for operation.
//
// Two forms of the shadow ray are kept, with the same result bits; DESIGN 5.14 has the figures of both, on which the choice rests:
//   TWO SITES (the default, the faster): a second trace_scene<..., QUERY = true> call site inside the opaque shader, any_lane = true.
//     Its hit record, HitRecShadow, has no attributes: nothing reads them.
//   ONE SITE (-DRR_SURFACES_ONE_SITE): the tree has one trace_scene<..., QUERY = true> call site.  A shadow ray is a trip of the
//     tree's own loop: the lane carries X, Nf, E, its light index and f = cs * g as state, and the site takes a per-lane mask (0xff
//     for a radiance ray) and a per-lane first-hit flag.  Lanes that trace shadow rays stay converged with lanes that trace radiance
//     rays, and there is one copy of the walk.  Its hit record, HitRecTree, skips the attributes of the hit on a shadow trip.
// The two-site tree takes "light row i" as a callable (ray_tree_surfaces_two_site): the table's row for the surface kernels, the row
// moved to one sample's offset for the lit frames (rr_render_lit.h), which use this form in either build.
// The traversal stack is free while a hit is being shaded, so a shadow ray walks on the same LDS column.  The light rows sit in the
// kernel-argument segment (LightsDev, rr_types.h) and every loop over them has a wave-uniform index, so they arrive through scalar
// loads; the surface row differs per lane and comes through vector loads, as mats does.
// Not covered: environment lighting of opaque surfaces, textures, opaque rows in the composed and shutter frames, the dispatch
// kernels and the _materials calls.  (Opaque rows over scene keys, through a lens and under lights with an area: rr_render_lit.h.
// Shadow rays that pass glass and take its tint: the two-site tree's WALK form, which puts shadow_walk (rr_render_shadows.h, with
// its contract) where step b's first-hit ray stands; the walk leaves out Fresnel loss and bending at the interfaces it crosses,
// absorption beyond its last hit, and caustics.)
#pragma once
#include "rr_render_nested.h"

namespace rr {

// The hit record of a shadow ray of the two-site form: HitRec's walk (hits_begin, hit_bound, leaf_test and hit_found bind to HitRec's
// overloads) without the attributes of the hit, which nothing reads -- only .hit
struct HitRecShadow : HitRec {};
__device__ __forceinline__ void hits_end_blas(const TriRec* __restrict__, f3, f3, HitRecShadow&) {}
__device__ __forceinline__ void hits_end_scene(const SceneDev&, f3, f3, HitRecShadow&) {}

// The hit record of the one-site form: HitRecFace, whose end steps are skipped on a shadow trip (shadow is set by the caller before
// the walk; hits_begin does not touch it)
struct HitRecTree : HitRecFace { bool shadow; };
__device__ __forceinline__ void hits_end_blas(const TriRec* __restrict__ tris, f3 O, f3 D, HitRecTree& best)
{
    if (!best.shadow) hits_end_blas(tris, O, D, static_cast<HitRecFace&>(best));
}
__device__ __forceinline__ void hits_end_scene(const SceneDev& sc, f3 O, f3 D, HitRecTree& best)
{
    if (!best.shadow) hits_end_scene(sc, O, D, static_cast<HitRecFace&>(best));
}

// what the surface kernels read beside the material table
struct SurfArgs {
    const SurfDev* rows;      // device memory, n rows; n == 0: every row is glass and rows is not read
    uint32_t n;
};

// step 1 of the nested contract: Beer-Lambert over t in the medium crossed (c: top(L), not air)
__device__ __forceinline__ void absorb_crossed(const MatDev* __restrict__ mats, uint32_t c, float t, f3& w)
{
    const MatDev* __restrict__ mc = mats + (c - 1u);
    const float sr = mc->sigma[0], sg = mc->sigma[1], sb = mc->sigma[2];
    w.x = w.x * rr_expf_neg(-(sr * t));
    w.y = w.y * rr_expf_neg(-(sg * t));
    w.z = w.z * rr_expf_neg(-(sb * t));
}

// The walk of the tree's WALK form, defined in rr_render_shadows.h: a translation unit that instantiates that form includes it; the
// first-hit form never names it, so this header compiles alone
template <bool TLAS, class E>
__device__ __forceinline__ bool shadow_walk(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf, uint32_t mat0,
                                            uint32_t K, uint32_t mask, f3 X, f3 Ld, float far, uint32_t L, E* stk, LaneStats& st, f3& T);

// steps 2-5 of the nested contract on a glass row: shade_ray_nested's text after the absorption.  True: r is the continuing ray
template <bool TLAS, class PK>
__device__ __forceinline__ bool glass_hit(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const HitRecFace& h, uint32_t m,
                                          f3 X, RayStateNested& r, int& np, PK& park)
{
    const uint32_t L = r.media, c = media_top(L);
    const uint32_t Lp = h.front ? media_push(L, m) : media_remove(L, m);
    const uint32_t cp = media_top(Lp);
    const uint32_t c1 = r.count + 1u;
    r.tmin = a.tmin_s; r.tmax = a.tmax_s;
    r.O = X;
    if (cp == c) {                                            // not an interface: straight on, at the price of one count
        r.media = Lp; r.count = c1;
        return true;
    }
    f3 N = shading_normal<TLAS>(sc, h);
    f3 Nf = h.front ? N : neg3(N);
    const float R0 = (0.2f / 2.2f) * (0.2f / 2.2f);           // hlsl:92
    float b = 1.0f - dot3(r.D, Nf);                           // hlsl:93, pow(b,5) = b*b*b*b*b
    float b2 = b * b, b4 = b2 * b2;
    float R = (R0 * (1.0f - R0)) * (b4 * b);
    const float n_from = c ? mats[c - 1u].ior : 1.0f, inv_n_to = cp ? mats[cp - 1u].inv_ior : 1.0f;
    float eta = n_from * inv_n_to;                            // hlsl:95 between the two media
    f3 d1;
    bool refr = refract_ray(d1, r.D, Nf, eta);
    bool refl = (int)r.count < a.max_reflect;                 // hlsl:110
    f3 d2 = mk3(0.0f, 0.0f, 0.0f);
    if (refl) d2 = normalize3(reflect_ray(r.D, Nf));          // hlsl:113
    if (refr) {
        if (refl) {                                           // park the reflected child: it stays in L
            PendRayNested p;
            p.ox = X.x; p.oy = X.y; p.oz = X.z; p.dx = d2.x; p.dy = d2.y; p.dz = d2.z;
            p.wr = r.w.x * R; p.wg = r.w.y * R; p.wb = r.w.z * R; p.count = c1; p.media = L;
            park.put(np, p);
            ++np;
        }
        const float T = 1.0f - R;
        r.D = d1; r.w = mk3(r.w.x * T, r.w.y * T, r.w.z * T); r.count = c1; r.media = Lp;            // hlsl:103-107
        return true;
    }
    if (refl) {
        r.D = d2; r.w = mk3(r.w.x * R, r.w.y * R, r.w.z * R); r.count = c1;                            // hlsl:118-122 (L stays)
        return true;
    }
    return false;
}

// step b's geometry of one light at X: the direction towards it, the far end of its shadow ray and the falloff
__device__ __forceinline__ void light_at(const LightDev& lt, const DispatchDev& a, f3 X, f3& Ld, float& far, float& g)
{
    Ld = mk3(lt.v[0], lt.v[1], lt.v[2]);
    far = a.tmax_s; g = 1.0f;
    if (lt.kind == LIGHT_POINT) {
        const f3 d = mk3(lt.v[0] - X.x, lt.v[1] - X.y, lt.v[2] - X.z);
        const float d2 = dot3(d, d);
        far = sqrtf(d2);
        Ld = mk3(d.x / far, d.y / far, d.z / far);
        g = 1.0f / d2;
    }
}

// steps c and d: the colour of the opaque hit, and its mirror child.  True: r is the continuing ray (L stays)
__device__ __forceinline__ bool opaque_end(const DispatchDev& a, const SurfDev* __restrict__ s, f3 Ev, f3 Nf, f3 X, RayStateNested& r, f3& acc)
{
    const f3 col = mk3(fmaf(s->albedo[0], Ev.x, s->emission[0]), fmaf(s->albedo[1], Ev.y, s->emission[1]), fmaf(s->albedo[2], Ev.z, s->emission[2]));
    acc.x = fmaf(r.w.x, col.x, acc.x); acc.y = fmaf(r.w.y, col.y, acc.y); acc.z = fmaf(r.w.z, col.z, acc.z);
    const float kr = s->specular[0], kg = s->specular[1], kb = s->specular[2];
    if (kr != 0.0f || kg != 0.0f || kb != 0.0f) {
        r.D = normalize3(reflect_ray(r.D, Nf));
        r.w = mk3(r.w.x * kr, r.w.y * kg, r.w.z * kb);
        r.O = X; r.count = r.count + 1u;
        r.tmin = a.tmin_s; r.tmax = a.tmax_s;
        return true;
    }
    return false;
}

// the branch has ended: take up the ray parked last.  False: the tree is done
template <class PK>
__device__ __forceinline__ bool pop_parked(const DispatchDev& a, RayStateNested& r, int& np, PK& park)
{
    if (np == 0) return false;
    --np;
    const PendRayNested p = park.get(np);
    r.O = mk3(p.ox, p.oy, p.oz); r.D = mk3(p.dx, p.dy, p.dz); r.w = mk3(p.wr, p.wg, p.wb);
    r.count = p.count; r.media = p.media;
    r.tmin = a.tmin_s; r.tmax = a.tmax_s;
    return true;
}

// ray_tree_nested with the opaque hit group, two-site form: the shadow rays are traced where the hit is shaded.  light_row(i) is row
// i of the lights as this tree sees it -- the table's row (a reference), or a copy of it moved for one sample (rr_render_lit.h); i is
// wave-uniform.  lights itself gives the ambient term and the number of rows.  Built in either form's build: the lit frames use it.
// WALK: step b's shadow ray is shadow_walk under the cap K (1 .. SHADOW_MAX_STEPS, wave-uniform) and the light is weighted with what
// the glass let through (rr_render_shadows.h); the first-hit form never reads K
template <bool TLAS, class E, bool WALK = false, class PK, class LR>
__device__ __forceinline__ f3 ray_tree_surfaces_two_site(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf,
                                                         const LightsDev& lights, LR&& light_row, uint32_t mat0, RayStateNested r, E* stk, PK& park,
                                                         LaneStats& st, uint32_t K = 0u)
{
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    int np = 0;
    for (;;) {
        HitRecFace h;
        trace_scene<false, TLAS, E, GlobalNodes>(sc, r.O, r.D, r.tmin, r.tmax, 0u, h, stk, st.cnt, Diag{ nullptr }, GlobalNodes{});
        ++st.rays;
        bool have_next = false;
        if (!h.hit) {                                         // Miss
            f3 e = env_lookup(sc, r.D);
            acc.x = fmaf(r.w.x, e.x, acc.x); acc.y = fmaf(r.w.y, e.y, acc.y); acc.z = fmaf(r.w.z, e.z, acc.z);
        } else if ((int)r.count < a.max_refract) {            // ClosestHit
            const uint32_t row = hit_material<TLAS>(sc, h, mat0);
            const uint32_t c = media_top(r.media);
            if (c) absorb_crossed(mats, c, h.t, r.w);
            const f3 X = mk3(fmaf(h.t, r.D.x, r.O.x), fmaf(h.t, r.D.y, r.O.y), fmaf(h.t, r.D.z, r.O.z));   // hlsl:88
            if (row < sf.n && sf.rows[row].kind == SURFACE_OPAQUE) {
                const f3 N = shading_normal<TLAS>(sc, h);
                const f3 Nf = h.front ? N : neg3(N);
                f3 Ev = mk3(lights.ambient[0], lights.ambient[1], lights.ambient[2]);
                for (uint32_t i = 0; i < lights.n; ++i) {
                    const LightDev& lt = light_row(i);                    // (a copy lives as long as lt)
                    f3 Ld;
                    float far, g;
                    light_at(lt, a, X, Ld, far, g);
                    const float cs = dot3(Nf, Ld);
                    if (cs > 0.0f) {
                        if constexpr (WALK) {
                            f3 T;
                            if (shadow_walk<TLAS, E>(sc, a, mats, sf, mat0, K, TLAS ? lt.shadow_mask : (lt.shadow_mask & 1u), X, Ld, far, r.media, stk, st, T)) {
                                const float f = cs * g;
                                Ev.x = fmaf(lt.radiance[0], f * T.x, Ev.x); Ev.y = fmaf(lt.radiance[1], f * T.y, Ev.y);
                                Ev.z = fmaf(lt.radiance[2], f * T.z, Ev.z);
                            }
                        } else {
                            HitRecShadow hs;
                            trace_scene<false, TLAS, E, GlobalNodes, true, HitRecShadow>(sc, X, Ld, a.tmin_s, far, 0u, hs, stk, st.cnt, Diag{ nullptr },
                                                                                         GlobalNodes{}, TLAS ? lt.shadow_mask : (lt.shadow_mask & 1u), true);
                            ++st.rays;
                            if (!hs.hit) {
                                const float f = cs * g;
                                Ev.x = fmaf(lt.radiance[0], f, Ev.x); Ev.y = fmaf(lt.radiance[1], f, Ev.y); Ev.z = fmaf(lt.radiance[2], f, Ev.z);
                            }
                        }
                    }
                }
                have_next = opaque_end(a, sf.rows + row, Ev, Nf, X, r, acc);
            } else {
                have_next = glass_hit<TLAS>(sc, a, mats, h, row + 1u, X, r, np, park);
            }
        }
        if (!have_next && !pop_parked(a, r, np, park)) break;
    }
    return acc;
}

#ifndef RR_SURFACES_ONE_SITE
// the surface kernels' tree: the lights are the table's rows
template <bool TLAS, class E, bool WALK = false, class PK>
__device__ __forceinline__ f3 ray_tree_surfaces(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf,
                                                const LightsDev& lights, uint32_t mat0, RayStateNested r, E* stk, PK& park, LaneStats& st,
                                                uint32_t K = 0u)
{
    return ray_tree_surfaces_two_site<TLAS, E, WALK>(sc, a, mats, sf, lights, [&](uint32_t i) -> const LightDev& { return lights.l[i]; }, mat0, r, stk,
                                                     park, st, K);
}
#else
// ray_tree_nested with the opaque hit group, one trace site: a lane's trip is a radiance ray or, while it shades an opaque hit, the
// shadow ray of light `li`.  Every loop over the lights runs over the whole table with a per-lane condition, so its index stays
// wave-uniform; between two of a hit's shadow rays the lane keeps X, Nf, E, li, f and the row, and recomputes the rest.
// The walk has the two-site tree only: WALK forwards to it, as the other build does
template <bool TLAS, class E, bool WALK = false, class PK>
__device__ __forceinline__ f3 ray_tree_surfaces(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf,
                                                const LightsDev& lights, uint32_t mat0, RayStateNested r, E* stk, PK& park, LaneStats& st,
                                                uint32_t K = 0u)
{
    if constexpr (WALK)
        return ray_tree_surfaces_two_site<TLAS, E, true>(sc, a, mats, sf, lights, [&](uint32_t i) -> const LightDev& { return lights.l[i]; }, mat0, r, stk,
                                                         park, st, K);
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    int np = 0;
    bool shadow = false;                                      // this trip is a shadow ray
    f3 X = mk3(0.0f, 0.0f, 0.0f), Nf = X, Ev = X, sD = X;
    float f = 0.0f, sfar = 0.0f;
    uint32_t li = 0u, smask = 0u, row = 0u;
    for (;;) {
        HitRecTree h;
        h.shadow = shadow;
        trace_scene<false, TLAS, E, GlobalNodes, true, HitRecTree>(sc, shadow ? X : r.O, shadow ? sD : r.D, shadow ? a.tmin_s : r.tmin,
                                                                  shadow ? sfar : r.tmax, 0u, h, stk, st.cnt, Diag{ nullptr }, GlobalNodes{},
                                                                  shadow ? smask : 0xffu, shadow);
        ++st.rays;
        bool have_next = false, lighting = false;
        if (shadow) {                                         // the answer for light li
            if (!h.hit)
                for (uint32_t i = 0; i < lights.n; ++i)
                    if (i == li) {
                        const LightDev& lt = lights.l[i];
                        Ev.x = fmaf(lt.radiance[0], f, Ev.x); Ev.y = fmaf(lt.radiance[1], f, Ev.y); Ev.z = fmaf(lt.radiance[2], f, Ev.z);
                    }
            ++li;
            lighting = true;
        } else if (!h.hit) {                                  // Miss
            f3 e = env_lookup(sc, r.D);
            acc.x = fmaf(r.w.x, e.x, acc.x); acc.y = fmaf(r.w.y, e.y, acc.y); acc.z = fmaf(r.w.z, e.z, acc.z);
        } else if ((int)r.count < a.max_refract) {            // ClosestHit
            row = hit_material<TLAS>(sc, h, mat0);
            const uint32_t c = media_top(r.media);
            if (c) absorb_crossed(mats, c, h.t, r.w);
            X = mk3(fmaf(h.t, r.D.x, r.O.x), fmaf(h.t, r.D.y, r.O.y), fmaf(h.t, r.D.z, r.O.z));          // hlsl:88
            if (row < sf.n && sf.rows[row].kind == SURFACE_OPAQUE) {
                const f3 N = shading_normal<TLAS>(sc, h);
                Nf = h.front ? N : neg3(N);
                Ev = mk3(lights.ambient[0], lights.ambient[1], lights.ambient[2]);
                li = 0u;
                lighting = true;
            } else {
                have_next = glass_hit<TLAS>(sc, a, mats, h, row + 1u, X, r, np, park);
            }
        }
        if (lighting) {                                       // the next light this hit faces, from li on
            shadow = false;
            for (uint32_t i = 0; i < lights.n; ++i)
                if (!shadow && i >= li) {
                    const LightDev& lt = lights.l[i];
                    f3 Ld;
                    float far, g;
                    light_at(lt, a, X, Ld, far, g);
                    const float cs = dot3(Nf, Ld);
                    if (cs > 0.0f) {
                        shadow = true;
                        li = i; f = cs * g; sD = Ld; sfar = far;
                        smask = TLAS ? lt.shadow_mask : (lt.shadow_mask & 1u);
                    }
                }
            if (shadow) continue;
            have_next = opaque_end(a, sf.rows + row, Ev, Nf, X, r, acc);
        }
        if (!have_next && !pop_parked(a, r, np, park)) break;
    }
    return acc;
}
#endif

} // namespace rr
