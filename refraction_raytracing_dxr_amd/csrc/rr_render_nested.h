// rr_render_nested.h -- the ray tree of the nested-media kernels (rr_render_nested.hip): shade_ray_mat and ray_tree_mat of
// rr_render_materials.h with a list of the media a ray is in, so that instances may sit inside, or overlap, other instances.
//
// A ray carries (O, D, w[3], count, L).  L lists the material rows of the media the ray is in, in the order it entered them, four
// at most; empty is air (ior 1, no absorption).  A caller's primary ray starts with L empty.  L is ONE 32-bit word: byte k holds
// row + 1 of the k-th medium entered and 0 above the list's end, so push, top and remove-last-occurrence are a few shifts, masks and
// selects on one register -- no array, no loop, nothing a lane could index dynamically into scratch.  Rows are therefore limited to
// 0 .. 254 (NESTED_MAX_MATERIAL; the host refuses a scene with a higher one).
//
// TraceRay is called with cull flags 0 (both faces) and mask 0xff; the face of the hit is HitRecFace::front (rr_device.h).
//   Miss:        acc.c = fmaf(w.c, e.c, acc.c); nothing is absorbed, whatever L holds (an open mesh).
//   ClosestHit on an instance of row m at distance t, count < max_refract (a hit at the limit adds nothing):
//     1. c = top(L); if c is not air, w.ch = w.ch * rr_expf_neg(-(sigma[c].ch * t)): the medium CROSSED, not the one hit.
//     2. front face: L' = push(L, m), a push onto a full list is dropped; back face: L' = L without its last occurrence of m,
//        removing an absent row is a no-op.  c' = top(L').
//     3. X = fmaf(t, D, O); children have count + 1 and [tmin_secondary, tmax_secondary].
//     4. c' == c (as bytes): NOT AN INTERFACE -- the ray leaves something whose surface lies inside a medium entered later, enters
//        a second body of the same row, has its push dropped, or meets a back face from outside.  One child (X, D, w, L'): D and
//        w keep their bits, no reflection, no Fresnel factor.  The pass still costs one count, so the tree stays bounded by
//        ray_tree's argument (count grows by one per level and ends the branch at max_refract; one parked ray per level while
//        count < max_reflect).
//     5. otherwise AN INTERFACE: N, X, R as shade_ray_mat; Nf = front ? N : -N; eta = ior[c] * inv_ior[c'], air being 1.0f on
//        either side; the refracted child carries L' and w * (1 - R), the reflected one (count < max_reflect) stays where it was: L
//        and w * R; total internal reflection leaves the reflected child alone.  Depth-first, reflected rays parked, as before.
//
// Reduction: where culled and unculled TraceRay find the same hit for every ray of every tree -- closed, consistently wound,
// pairwise disjoint instances -- this tree is shade_ray_mat's bit for bit: 1.0f * inv_ior and ior * 1.0f are exact, top(L) is the
// instance being left, front is outside.
// Overlap is handled without priorities: of two surfaces that cross, the interface is taken at the first one met and the second
// is "not an interface".
// Not covered: more than four simultaneous media (the dropped push), rays that start inside a medium, R0 from the two indices (it
// stays the shader's constant), lens / spectral / adaptive frames, the dispatch kernels.
#pragma once
#include "rr_render_materials.h"

namespace rr {

constexpr uint32_t NESTED_MAX_MEDIA = 4, NESTED_MAX_MATERIAL = 254;

// ---- the medium list in one register: bytes of row + 1 from the low end, 0 = empty -------------------------------------------------
__device__ __forceinline__ uint32_t media_count(uint32_t L) { return (39u - (uint32_t)__clz((int)L)) >> 3; }      // __clz(0) = 32
// the last medium entered (0: air).  The bytes above the list's end are 0, so the shifted word IS the byte; an empty list shifts 0
__device__ __forceinline__ uint32_t media_top(uint32_t L) { return L >> ((media_count(L) * 8u - 8u) & 31u); }
__device__ __forceinline__ uint32_t media_push(uint32_t L, uint32_t b)
{
    const uint32_t n = media_count(L);
    return n < NESTED_MAX_MEDIA ? L | (b << ((n * 8u) & 31u)) : L;
}
// L without the highest byte equal to b (b != 0, so an empty byte never matches); the bytes above it move down
__device__ __forceinline__ uint32_t media_remove(uint32_t L, uint32_t b)
{
    const bool m3 = (L >> 24) == b, m2 = ((L >> 16) & 0xffu) == b, m1 = ((L >> 8) & 0xffu) == b, m0 = (L & 0xffu) == b;
    const uint32_t up = L >> 8;
    return m3 ? L & 0x00ffffffu
         : m2 ? (L & 0x0000ffffu) | (up & 0x00ff0000u)
         : m1 ? (L & 0x000000ffu) | (up & 0x00ffff00u)
         : m0 ? up : L;
}

// PendRayMat and the list: eleven words
struct PendRayNested {
    float ox, oy, oz, dx, dy, dz, wr, wg, wb;
    uint32_t count, media;
};

template <int PEND>
struct RegParkNested {
    PendRayNested pend[PEND];
    __device__ __forceinline__ void put(int k, const PendRayNested& p)
    {
#pragma unroll
        for (int i = 0; i < PEND; ++i) if (i == k) pend[i] = p;
    }
    __device__ __forceinline__ PendRayNested get(int k) const
    {
        PendRayNested p = pend[0];
#pragma unroll
        for (int i = 1; i < PEND; ++i) if (i == k) p = pend[i];
        return p;
    }
};

// a lane's current ray: RayStateMat with the list in place of outside
struct RayStateNested {
    f3 O, D, w;
    float tmin, tmax;
    uint32_t count, media;
};

__device__ __forceinline__ RayStateNested with_empty_media(const RayState& s)
{
    RayStateNested r;
    r.O = s.O; r.D = s.D; r.w = mk3(s.w, s.w, s.w);
    r.tmin = s.tmin; r.tmax = s.tmax; r.count = s.count; r.media = 0u;
    return r;
}

// shade_ray_mat over the list (see the head of this file).  mats: the context's table, row b - 1 for byte b; a lane loads
// { ior, inv_ior } of c and c' at an interface and the sigmas of c only when c is not air.  a.ior and a.inv_ior are not read.
template <bool TLAS, class PK>
__device__ __forceinline__ bool shade_ray_nested(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, uint32_t mat0,
                                                 const HitRecFace& h, RayStateNested& r, f3& acc, int& np, PK& park)
{
    bool have_next = false;
    if (!h.hit) {                                             // Miss
        f3 e = env_lookup(sc, r.D);
        acc.x = fmaf(r.w.x, e.x, acc.x); acc.y = fmaf(r.w.y, e.y, acc.y); acc.z = fmaf(r.w.z, e.z, acc.z);
    } else if ((int)r.count < a.max_refract) {                // ClosestHit
        const uint32_t m = hit_material<TLAS>(sc, h, mat0) + 1u;
        const uint32_t L = r.media, c = media_top(L);
        if (c) {                                              // Beer-Lambert over h.t in the medium crossed
            const MatDev* __restrict__ mc = mats + (c - 1u);
            const float sr = mc->sigma[0], sg = mc->sigma[1], sb = mc->sigma[2];
            r.w.x = r.w.x * rr_expf_neg(-(sr * h.t));
            r.w.y = r.w.y * rr_expf_neg(-(sg * h.t));
            r.w.z = r.w.z * rr_expf_neg(-(sb * h.t));
        }
        const uint32_t Lp = h.front ? media_push(L, m) : media_remove(L, m);
        const uint32_t cp = media_top(Lp);
        f3 X = mk3(fmaf(h.t, r.D.x, r.O.x), fmaf(h.t, r.D.y, r.O.y), fmaf(h.t, r.D.z, r.O.z));   // hlsl:88
        const uint32_t c1 = r.count + 1u;
        r.tmin = a.tmin_s; r.tmax = a.tmax_s;
        r.O = X;
        if (cp == c) {                                        // not an interface: straight on, at the price of one count
            r.media = Lp; r.count = c1;
            have_next = true;
        } else {
            f3 N = shading_normal<TLAS>(sc, h);
            f3 Nf = h.front ? N : neg3(N);
            const float R0 = (0.2f / 2.2f) * (0.2f / 2.2f);   // hlsl:92
            float b = 1.0f - dot3(r.D, Nf);                   // hlsl:93, pow(b,5) = b*b*b*b*b
            float b2 = b * b, b4 = b2 * b2;
            float R = (R0 * (1.0f - R0)) * (b4 * b);
            const float n_from = c ? mats[c - 1u].ior : 1.0f, inv_n_to = cp ? mats[cp - 1u].inv_ior : 1.0f;
            float eta = n_from * inv_n_to;                    // hlsl:95 between the two media
            f3 d1;
            bool refr = refract_ray(d1, r.D, Nf, eta);
            bool refl = (int)r.count < a.max_reflect;         // hlsl:110
            f3 d2 = mk3(0.0f, 0.0f, 0.0f);
            if (refl) d2 = normalize3(reflect_ray(r.D, Nf));  // hlsl:113
            if (refr) {
                if (refl) {                                   // park the reflected child: it stays in L
                    PendRayNested p;
                    p.ox = X.x; p.oy = X.y; p.oz = X.z; p.dx = d2.x; p.dy = d2.y; p.dz = d2.z;
                    p.wr = r.w.x * R; p.wg = r.w.y * R; p.wb = r.w.z * R; p.count = c1; p.media = L;
                    park.put(np, p);
                    ++np;
                }
                const float T = 1.0f - R;
                r.D = d1; r.w = mk3(r.w.x * T, r.w.y * T, r.w.z * T); r.count = c1; r.media = Lp;        // hlsl:103-107
                have_next = true;
            } else if (refl) {
                r.D = d2; r.w = mk3(r.w.x * R, r.w.y * R, r.w.z * R); r.count = c1;                        // hlsl:118-122 (L stays)
                have_next = true;
            }
        }
    }
    if (!have_next) {
        if (np == 0) return false;
        --np;
        const PendRayNested p = park.get(np);
        r.O = mk3(p.ox, p.oy, p.oz); r.D = mk3(p.dx, p.dy, p.dz); r.w = mk3(p.wr, p.wg, p.wb);
        r.count = p.count; r.media = p.media;
        r.tmin = a.tmin_s; r.tmax = a.tmax_s;
    }
    return true;
}

// ray_tree_mat over shade_ray_nested: the tree of primary ray r, depth-first, every TraceRay with cull flags 0
template <bool TLAS, class E, class PK>
__device__ __forceinline__ f3 ray_tree_nested(const SceneDev& sc, const DispatchDev& a, const MatDev* __restrict__ mats, uint32_t mat0,
                                              RayStateNested r, E* stk, PK& park, LaneStats& st)
{
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    int np = 0;
    for (;;) {
        HitRecFace h;
        trace_scene<false, TLAS, E, GlobalNodes>(sc, r.O, r.D, r.tmin, r.tmax, 0u, h, stk, st.cnt, Diag{ nullptr }, GlobalNodes{});
        ++st.rays;
        if (!shade_ray_nested<TLAS>(sc, a, mats, mat0, h, r, acc, np, park)) break;
    }
    return acc;
}

} // namespace rr
