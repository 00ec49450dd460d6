// rr_render_materials.h -- the ray tree of the material kernels (rr_render_materials.hip): shade_ray and ray_tree of
// rr_render_common.h with a material per instance.  Three things differ from shade_ray, and nothing else:
//   1. the path weight is one float per channel: RayGen sets (1, 1, 1), every w * (1 - R) and w * R is taken per channel, a Miss adds
//      acc.c = fmaf(w.c, e.c, acc.c), and a parked ray carries three weights (10 words instead of 8);
//   2. ClosestHit refracts with the material m of the hit instance: eta = outside ? mats[m].inv_ior : mats[m].ior;
//   3. a ray that arrives with outside == false has travelled h.t through the glass of instance m (secondary directions are
//      normalised by the shader, so h.t is a length) and is absorbed first: w.c = w.c * rr_expf_neg(-(mats[m].sigma[c] * h.t)),
//      each operation rounded once.  The medium is that of the surface being left: for overlapping or nested instances a stated
//      approximation.  A Miss from inside (an open mesh) absorbs nothing.
// With sigma == 0 the factor is rr_expf_neg(-0) = 1 exactly, so a table whose rows are all { ior, 0, 0, 0 } gives the bits of shade_ray
// under DispatchDev::ior = ior.
#pragma once
#include "rr_render_common.h"

namespace rr {

struct PendRayMat {
    float ox, oy, oz, dx, dy, dz, wr, wg, wb;
    uint32_t meta;          // count | outside << 16
};

// RegPark with the ten-word slot
template <int PEND>
struct RegParkMat {
    PendRayMat pend[PEND];
    __device__ __forceinline__ void put(int k, const PendRayMat& p)
    {
#pragma unroll
        for (int i = 0; i < PEND; ++i) if (i == k) pend[i] = p;
    }
    __device__ __forceinline__ PendRayMat get(int k) const
    {
        PendRayMat p = pend[0];
#pragma unroll
        for (int i = 1; i < PEND; ++i) if (i == k) p = pend[i];
        return p;
    }
};

// a lane's current ray: RayState with the weight per channel
struct RayStateMat {
    f3 O, D, w;
    float tmin, tmax;
    uint32_t count;
    bool outside;
};

__device__ __forceinline__ RayStateMat with_rgb_weight(const RayState& s)
{
    RayStateMat r;
    r.O = s.O; r.D = s.D; r.w = mk3(s.w, s.w, s.w);
    r.tmin = s.tmin; r.tmax = s.tmax; r.count = s.count; r.outside = s.outside;
    return r;
}

// The material of the hit: the instance's index through a vector load (the hit instance differs per lane), or mat0 where the scene
// skips the top level.  The host has checked every index of the scene against the table's length.
template <bool TLAS>
__device__ __forceinline__ uint32_t hit_material(const SceneDev& sc, const HitRec& h, uint32_t mat0)
{
    return TLAS ? sc.insts[h.inst].material : mat0;
}

// shade_ray (rr_render_common.h) with the three changes above.  a.ior and a.inv_ior are not read.
template <bool TLAS, class PK>
__device__ __forceinline__ bool shade_ray_mat(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, uint32_t mat0,
                                              const HitRec& h, RayStateMat& r, f3& acc, int& np, PK& park)
{
    bool have_next = false;
    if (!h.hit) {                                             // Miss
        f3 e = env_lookup(sc, r.D);
        acc.x = fmaf(r.w.x, e.x, acc.x); acc.y = fmaf(r.w.y, e.y, acc.y); acc.z = fmaf(r.w.z, e.z, acc.z);
    } else if ((int)r.count < a.max_refract) {                // ClosestHit (a hit at the refraction limit adds nothing: its weight is not needed)
        const MatDev* __restrict__ m = mats + hit_material<TLAS>(sc, h, mat0);
        const float2 n = *reinterpret_cast<const float2*>(&m->ior);         // { ior, inv_ior }
        if (!r.outside) {                                     // through the glass of the surface being left: Beer-Lambert over h.t
            const float sr = m->sigma[0], sg = m->sigma[1], sb = m->sigma[2];
            r.w.x = r.w.x * rr_expf_neg(-(sr * h.t));
            r.w.y = r.w.y * rr_expf_neg(-(sg * h.t));
            r.w.z = r.w.z * rr_expf_neg(-(sb * h.t));
        }
        f3 N = shading_normal<TLAS>(sc, h);
        f3 X = mk3(fmaf(h.t, r.D.x, r.O.x), fmaf(h.t, r.D.y, r.O.y), fmaf(h.t, r.D.z, r.O.z));   // hlsl:88
        f3 Nf = r.outside ? N : neg3(N);
        const float R0 = (0.2f / 2.2f) * (0.2f / 2.2f);       // hlsl:92
        float b = 1.0f - dot3(r.D, Nf);                       // hlsl:93, pow(b,5) = b*b*b*b*b
        float b2 = b * b, b4 = b2 * b2;
        float R = (R0 * (1.0f - R0)) * (b4 * b);
        float eta = r.outside ? n.y : n.x;                    // hlsl:95 with the instance's material
        f3 d1;
        bool refr = refract_ray(d1, r.D, Nf, eta);
        bool refl = (int)r.count < a.max_reflect;             // hlsl:110
        f3 d2 = mk3(0.0f, 0.0f, 0.0f);
        if (refl) d2 = normalize3(reflect_ray(r.D, Nf));      // hlsl:113
        const uint32_t c1 = r.count + 1u;
        r.tmin = a.tmin_s; r.tmax = a.tmax_s;
        r.O = X;
        if (refr) {
            if (refl) {                                       // park the reflected child
                PendRayMat p;
                p.ox = X.x; p.oy = X.y; p.oz = X.z; p.dx = d2.x; p.dy = d2.y; p.dz = d2.z;
                p.wr = r.w.x * R; p.wg = r.w.y * R; p.wb = r.w.z * R; p.meta = c1 | (r.outside ? 0x10000u : 0u);
                park.put(np, p);
                ++np;
            }
            const float T = 1.0f - R;
            r.D = d1; r.w = mk3(r.w.x * T, r.w.y * T, r.w.z * T); r.count = c1; r.outside = !r.outside;   // hlsl:103-107
            have_next = true;
        } else if (refl) {
            r.D = d2; r.w = mk3(r.w.x * R, r.w.y * R, r.w.z * R); r.count = c1;                        // hlsl:118-122
            have_next = true;
        }
    }
    if (!have_next) {
        if (np == 0) return false;
        --np;
        const PendRayMat p = park.get(np);
        r.O = mk3(p.ox, p.oy, p.oz); r.D = mk3(p.dx, p.dy, p.dz); r.w = mk3(p.wr, p.wg, p.wb);
        r.count = p.meta & 0xffffu; r.outside = (p.meta & 0x10000u) != 0u;
        r.tmin = a.tmin_s; r.tmax = a.tmax_s;
    }
    return true;
}

// ray_tree (rr_render_common.h) over shade_ray_mat: the tree of primary ray r, depth-first; bounded by the same argument
template <bool TLAS, class E, class PK>
__device__ __forceinline__ f3 ray_tree_mat(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, uint32_t mat0, RayStateMat r,
                                           E* stk, PK& park, LaneStats& st)
{
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    int np = 0;
    for (;;) {
        HitRec h;
        trace_scene<false, TLAS, E, GlobalNodes>(sc, r.O, r.D, r.tmin, r.tmax, r.outside ? CULL_BACK : CULL_FRONT, h, stk, st.cnt,
                                                 Diag{ nullptr }, GlobalNodes{});
        ++st.rays;
        if (!shade_ray_mat<TLAS>(sc, a, mats, mat0, h, r, acc, np, park)) break;
    }
    return acc;
}

} // namespace rr
