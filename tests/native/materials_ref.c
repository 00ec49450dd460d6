/* materials_ref.c -- the reference of the material ray tree (tests/materials_helpers.py compiles and loads it; test infrastructure).
 *
 * ClosestHit of oracle/rr_oracle.c (trace_and_shade, accum_mode 1: the path-weight sum in the recursion's order) restated with
 * the three changes of per-instance glass:
 *   1. the path weight is one float per channel;
 *   2. eta comes from the material of the hit instance, mats[hitgroup_flags & 0xffffff];
 *   3. a ray that arrives from inside is absorbed first, w.c = w.c * exp_neg(-(sigma_a[c] * t)).
 * TraceRay and the Miss lookup are the oracle library's own (rro_trace, rro_env_lookup); the shading normal, the instance inverse,
 * the vector helpers and exp_neg are written out again here, exp_neg from its definition and not from the product's source.
 * Built with -ffp-contract=off: an operation is fused only where fmaf is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/rr_oracle.h"

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 neg(v3 a) { return mk(-a.x, -a.y, -a.z); }
static inline float dot(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static inline v3 normalize(v3 a)
{
    float inv = 1.0f / sqrtf(dot(a, a));
    return mk(a.x * inv, a.y * inv, a.z * inv);
}

/* exp(x) for x <= 0: Cephes' expf, the contract of DESIGN 3 */
float mref_expf_neg(float x)
{
    if (!(x > -87.0f)) return 0.0f;
    float k = floorf(fmaf(x, 1.44269504f, 0.5f));
    float r = fmaf(k, -0.693359375f, x);
    r = fmaf(k, 2.12194440e-4f, r);
    static const float c[6] = { 1.9875691500e-4f, 1.3981999507e-3f, 8.3334519073e-3f, 4.1665795894e-2f, 1.6666665459e-1f, 5.0000001201e-1f };
    float p = c[0];
    for (int i = 1; i < 6; ++i) p = fmaf(p, r, c[i]);
    float y = fmaf(p, r * r, r) + 1.0f;
    int32_t e = (int32_t)k + 127;                 /* k >= -126: a normal number */
    uint32_t bits = (uint32_t)e << 23;
    float s;
    memcpy(&s, &bits, 4);
    return y * s;
}

typedef struct { float ior; float sigma_a[3]; } mref_material;
typedef struct { const rro_vertex* verts; const uint32_t* idx; } mref_mesh;

typedef struct {
    float inv[12];
    int identity;
    uint32_t mesh, material;
} inst_rec;

/* world -> object of a 3x4 object -> world transform (the arithmetic of rr_build_tlas and of the oracle's instances) */
static void affine_inverse(const float t[12], float inv[12])
{
    float a = t[0], b = t[1], c = t[2], d = t[4], e = t[5], f = t[6], g = t[8], h = t[9], i = t[10];
    float c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    float det = (a * c00 + b * c01) + c * c02;
    float r = 1.0f / det;
    inv[0] = c00 * r; inv[1] = (c * h - b * i) * r; inv[2] = (b * f - c * e) * r;
    inv[4] = c01 * r; inv[5] = (a * i - c * g) * r; inv[6] = (c * d - a * f) * r;
    inv[8] = c02 * r; inv[9] = (b * g - a * h) * r; inv[10] = (a * e - b * d) * r;
    float tx = t[3], ty = t[7], tz = t[11];
    inv[3] = -((inv[0] * tx + inv[1] * ty) + inv[2] * tz);
    inv[7] = -((inv[4] * tx + inv[5] * ty) + inv[6] * tz);
    inv[11] = -((inv[8] * tx + inv[9] * ty) + inv[10] * tz);
}

typedef struct {
    const rro_scene* s;
    const mref_mesh* meshes;
    const inst_rec* insts;
    const mref_material* mats;
    const rro_params* p;
    uint64_t* absorbed;           /* per material: inside hits it absorbed at */
    uint32_t rays;
    v3 acc;
} ctx;

static void shade(ctx* c, v3 O, v3 D, float tmin, float tmax, int outside, uint32_t count, v3 w)
{
    c->rays++;
    rro_hit h;
    const float o[3] = { O.x, O.y, O.z }, d[3] = { D.x, D.y, D.z };
    rro_trace(c->s, o, d, tmin, tmax, outside ? 0x10u : 0x20u, c->p->use_bvh, &h);
    if (!h.hit) {                                                          /* Miss: a Miss from inside absorbs nothing */
        float e[3];
        rro_env_lookup(c->s, d, c->p->use_libm, e);
        c->acc.x = fmaf(w.x, e[0], c->acc.x);
        c->acc.y = fmaf(w.y, e[1], c->acc.y);
        c->acc.z = fmaf(w.z, e[2], c->acc.z);
        return;
    }
    const inst_rec* ci = &c->insts[h.inst];
    const mref_material* m = &c->mats[ci->material];
    if (!outside) {                                                        /* change 3, before anything else */
        w.x = w.x * mref_expf_neg(-(m->sigma_a[0] * h.t));
        w.y = w.y * mref_expf_neg(-(m->sigma_a[1] * h.t));
        w.z = w.z * mref_expf_neg(-(m->sigma_a[2] * h.t));
        c->absorbed[ci->material]++;
    }
    if (!(count < (uint32_t)c->p->max_refract)) return;                    /* hlsl:82 */
    const mref_mesh* me = &c->meshes[ci->mesh];
    const float* nA = me->verts[me->idx[3 * h.prim + 0]].norm;             /* hlsl:83-85 */
    const float* nB = me->verts[me->idx[3 * h.prim + 1]].norm;
    const float* nC = me->verts[me->idx[3 * h.prim + 2]].norm;
    v3 A = mk(nA[0], nA[1], nA[2]), BA = sub(mk(nB[0], nB[1], nB[2]), A), CA = sub(mk(nC[0], nC[1], nC[2]), A);
    v3 Nr = mk(fmaf(h.v, CA.x, fmaf(h.u, BA.x, A.x)), fmaf(h.v, CA.y, fmaf(h.u, BA.y, A.y)), fmaf(h.v, CA.z, fmaf(h.u, BA.z, A.z)));
    if (!ci->identity) {                                                   /* inverse transpose of object -> world */
        const float* q = ci->inv;
        Nr = mk((q[0] * Nr.x + q[4] * Nr.y) + q[8] * Nr.z, (q[1] * Nr.x + q[5] * Nr.y) + q[9] * Nr.z, (q[2] * Nr.x + q[6] * Nr.y) + q[10] * Nr.z);
    }
    v3 N = normalize(Nr);
    v3 X = mk(fmaf(h.t, D.x, O.x), fmaf(h.t, D.y, O.y), fmaf(h.t, D.z, O.z));  /* hlsl:88 */
    v3 Nf = outside ? N : neg(N);
    const float R0 = (0.2f / 2.2f) * (0.2f / 2.2f);
    float b = 1.0f - dot(D, Nf);
    float b2 = b * b, b4 = b2 * b2;
    float R = (R0 * (1.0f - R0)) * (b4 * b);
    float eta = outside ? (1.0f / m->ior) : m->ior;                        /* change 2 */
    float cs = dot(Nf, D);
    float k = 1.0f - (eta * eta) * (1.0f - cs * cs);
    if (!(k < 0.0f)) {                                                     /* RefractRay, hlsl:70-76 */
        float a = eta * cs + sqrtf(k);
        v3 d1 = normalize(mk(eta * D.x - a * Nf.x, eta * D.y - a * Nf.y, eta * D.z - a * Nf.z));
        float T = 1.0f - R;
        shade(c, X, d1, c->p->tmin_secondary, c->p->tmax_secondary, !outside, count + 1, mk(w.x * T, w.y * T, w.z * T));
    }
    if (count < (uint32_t)c->p->max_reflect) {                             /* ReflectRay, hlsl:66-68, 110-122 */
        float k2 = 2.0f * dot(Nf, D);
        v3 d2 = normalize(mk(D.x - k2 * Nf.x, D.y - k2 * Nf.y, D.z - k2 * Nf.z));
        shade(c, X, d2, c->p->tmin_secondary, c->p->tmax_secondary, outside, count + 1, mk(w.x * R, w.y * R, w.z * R));
    }
}

/* The ray trees of n rays.  rays: n x 8 floats (origin, tmin, dir, tmax); insts: the records the oracle scene `s` was given (n_insts
 * >= 1), blas indexing meshes; p: bounce limits, secondary interval, use_bvh, use_libm (ior is not read).  out_rgb: n x 3 floats,
 * out_rgba8: n x 4 rro_unorm8 bytes (alpha 255), out_rays: TraceRay calls per tree, absorbed: n_mats counters, added to; any output
 * but out_rgb may be null.  Returns 0, or -1 for an instance whose material index is not below n_mats. */
int mref_shade(const rro_scene* s, const mref_mesh* meshes, const rro_instance* insts, uint32_t n_insts, const mref_material* mats,
               uint32_t n_mats, const rro_params* p, const float* rays, uint32_t n, float* out_rgb, uint8_t* out_rgba8, uint32_t* out_rays,
               uint64_t* absorbed)
{
    static const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    inst_rec recs[64];
    uint64_t scratch[64];
    if (n_insts == 0 || n_insts > 64 || n_mats == 0 || n_mats > 64) return -1;
    for (uint32_t i = 0; i < n_insts; ++i) {
        inst_rec* r = &recs[i];
        r->identity = memcmp(insts[i].transform, ident, sizeof ident) == 0;
        if (r->identity) memcpy(r->inv, ident, sizeof ident);
        else affine_inverse(insts[i].transform, r->inv);
        r->mesh = (uint32_t)insts[i].blas;
        r->material = insts[i].hitgroup_flags & 0xffffffu;
        if (r->material >= n_mats) return -1;
    }
    memset(scratch, 0, sizeof scratch);
    for (uint32_t i = 0; i < n; ++i) {
        const float* q = rays + 8 * (size_t)i;
        ctx c = { s, meshes, recs, mats, p, absorbed ? absorbed : scratch, 0, { 0, 0, 0 } };
        shade(&c, mk(q[0], q[1], q[2]), mk(q[4], q[5], q[6]), q[3], q[7], 1, 0, mk(1.0f, 1.0f, 1.0f));    /* RayGen: weight (1, 1, 1), outside */
        out_rgb[3 * (size_t)i + 0] = c.acc.x; out_rgb[3 * (size_t)i + 1] = c.acc.y; out_rgb[3 * (size_t)i + 2] = c.acc.z;
        if (out_rgba8) {
            out_rgba8[4 * (size_t)i + 0] = rro_unorm8(c.acc.x); out_rgba8[4 * (size_t)i + 1] = rro_unorm8(c.acc.y);
            out_rgba8[4 * (size_t)i + 2] = rro_unorm8(c.acc.z); out_rgba8[4 * (size_t)i + 3] = 255;
        }
        if (out_rays) out_rays[i] = c.rays;
    }
    return 0;
}
