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
// The tree is not a copy: ray_tree_surfaces_two_site (rr_render_surfaces.h) asks a callable for light row i, and this header hands it
// moved_light where the surface kernels hand it the table's row.  So the shadow ray has the two-site form only, whichever form
// rr_render_surfaces.hip is built with.
// Reduction: with every light offset applied to a zero shape, or with no shape table, v' == v in value and the tree computes what
// ray_tree_surfaces computes; with no surface table or every row glass, what ray_tree_nested computes.
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

// ray_tree_surfaces, two-site form, with the lights moved to (lu, lv).  WALK, K: the tree's; every walk goes towards the light as
// moved for its sample, so a shaped light's soft shadow takes the glass's colour
template <bool TLAS, class E, bool WALK = false, class PK>
__device__ __forceinline__ f3 ray_tree_lit(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, const SurfArgs& sf,
                                           const LightsDev& lights, const LightShapesDev& shapes, float lu, float lv, uint32_t mat0,
                                           RayStateNested r, E* stk, PK& park, LaneStats& st, uint32_t K = 0u)
{
    return ray_tree_surfaces_two_site<TLAS, E, WALK>(sc, a, mats, sf, lights, [&](uint32_t i) { return moved_light(lights, shapes, i, lu, lv); }, mat0, r,
                                                     stk, park, st, K);
}

} // namespace rr
