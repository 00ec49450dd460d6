// rr_render_lit.h -- the ray tree of the lit frames (rr_render_lit.hip): ray_tree_surfaces of rr_render_surfaces.h, two-site form,
// with the lights of ONE SAMPLE.  A lit frame gives every sample a light offset (lu, lv) in [-1, 1]^2, and light i, whose row of the
// shape table is (ex, ey), stands for that sample at
//   v' = fmaf(lv, ey, fmaf(lu, ex, v))      per component, fp32, each fmaf rounded once (rr_host_moved_lights on the host)
// Everything else in rr_render_surfaces.h's contract stands word for word with v' in place of v: step b's geometry is light_at's, on a
// copy of the row whose v is v'.  Without a shape table (shapes.on == 0) the row is used as it is, a -0 in v included.
//
// Where the move happens is the point of this header.  The sample index is wave-uniform, so lu, lv and every row of both tables are
// wave-uniform values with scalar addresses in the kernel-argument segment.  A per-sample moved COPY of LightsDev, indexed by the
// light loop's counter, would be a 272-byte private array with a dynamic index: scratch, or a ladder of selects.  Instead the row
// is moved where it is read: lights.l[i] and shapes.s[i] arrive through scalar loads as before (9 + 6 words), and three pairs of
// v_fma_f32 with scalar operands make v' in vector registers, once per light per opaque hit -- beside a shadow ray's walk, nothing.
// No lane move, no scratch; DESIGN 5.15 has the code object's figures.
//
// The shadow ray has the two-site form only: a second trace_scene<..., QUERY = true> call site inside the opaque shader.
// Reduction: with every light offset applied to a zero shape, or with no shape table, v' == v in value and the tree is
// ray_tree_surfaces' operation for operation; with no surface table or every row glass it is ray_tree_nested's.
#pragma once
#include "rr_render_surfaces.h"

namespace rr {

// light row i of one sample: the row as set, its v moved by the sample's offset over the light's shape
__device__ __forceinline__ LightDev moved_light(const LightsDev& lights, const LightShapesDev& shapes, uint32_t i, float lu, float lv)
{
    LightDev m = lights.l[i];
    if (shapes.on) {
        const LightShapeDev& sh = shapes.s[i];
        m.v[0] = fmaf(lv, sh.ey[0], fmaf(lu, sh.ex[0], m.v[0]));
        m.v[1] = fmaf(lv, sh.ey[1], fmaf(lu, sh.ex[1], m.v[1]));
        m.v[2] = fmaf(lv, sh.ey[2], fmaf(lu, sh.ex[2], m.v[2]));
    }
    return m;
}

// ray_tree_surfaces with the lights moved to (lu, lv): the shadow rays are traced where the hit is shaded
template <bool TLAS, class E, class PK>
__device__ __forceinline__ f3 ray_tree_lit(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf,
                                           const LightsDev& lights, const LightShapesDev& shapes, float lu, float lv, uint32_t mat0,
                                           RayStateNested r, E* stk, PK& park, LaneStats& st)
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
                    const LightDev lt = moved_light(lights, shapes, i, lu, lv);
                    f3 Ld;
                    float far, g;
                    light_at(lt, a, X, Ld, far, g);
                    const float cs = dot3(Nf, Ld);
                    if (cs > 0.0f) {
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
                have_next = opaque_end(a, sf.rows + row, Ev, Nf, X, r, acc);
            } else {
                have_next = glass_hit<TLAS>(sc, a, mats, h, row + 1u, X, r, np, park);
            }
        }
        if (!have_next && !pop_parked(a, r, np, park)) break;
    }
    return acc;
}

} // namespace rr
