/* nested_ref.c -- the reference of the nested-media ray tree (tests/nested_helpers.py compiles and loads it; test infrastructure).
 *
 * The tree of include/rrdxr.h "nested media", restated from that text with a recursion and a small array for the list of media:
 *   a ray carries (O, D, w[3], count, L); L lists the rows of the media it is in, in the order it entered them, four at most;
 *   TraceRay sees both faces (flags 0); a Miss adds fmaf(w, e, acc) and absorbs nothing;
 *   ClosestHit on row m at t with count < max_refract: absorb in c = top(L) over t; front face pushes m (dropped when full), back
 *   face removes the last m (nothing when absent); c' = top(L'); c' == c: one child straight on with L'; otherwise refract with
 *   eta = ior[c] * (1 / ior[c']), air being 1, the refracted child in L', the reflected one in L.
 * TraceRay and the Miss lookup are the oracle library's own (rro_trace with flags 0, rro_env_lookup).  The face of the hit is
 * computed here from the returned primitive: det = dot(e1, cross(D, e2)) with the ray taken into the instance's object space, front =
 * (det > 0) != the instance's FRONT_COUNTERCLOCKWISE flag.  The shading normal, the instance inverse, the vector helpers and exp_neg
 * are written out again here.  Built with -ffp-contract=off: an operation is fused only where fmaf is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/rr_oracle.h"

#define MAX_MEDIA 4

typedef struct { float x, y, z; } v3;
static inline v3 mk(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 neg(v3 a) { return mk(-a.x, -a.y, -a.z); }
static inline float dot(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static inline v3 cross(v3 a, v3 b) { return mk(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))); }
static inline v3 normalize(v3 a)
{
    float inv = 1.0f / sqrtf(dot(a, a));
    return mk(a.x * inv, a.y * inv, a.z * inv);
}

/* exp(x) for x <= 0: Cephes' expf, the contract of DESIGN 3 */
static float exp_neg(float x)
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

typedef struct { float ior; float sigma_a[3]; } nref_material;
typedef struct { const rro_vertex* verts; const uint32_t* idx; } nref_mesh;

/* what the trees of one call did: conditions on a fixture, never masks on a comparison */
typedef struct {
    uint64_t interfaces;        /* ClosestHits shaded as an interface */
    uint64_t passes;            /* ClosestHits that were not an interface */
    uint64_t dropped_pushes;    /* front faces met with a full list */
    uint64_t absent_removals;   /* back faces of a row the list does not hold */
    uint64_t deepest;           /* the longest list any ray carried */
    uint64_t absorbed[256];     /* per row: segments absorbed in it */
} nref_tallies;

typedef struct {
    float inv[12];
    int identity, ccw;
    uint32_t mesh, material;
} inst_rec;

/* a list of media: rows in the order they were entered */
typedef struct { int n; uint32_t row[MAX_MEDIA]; } media;
static int top_of(const media* L) { return L->n ? (int)L->row[L->n - 1] : -1; }          /* -1: air */

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
    const nref_mesh* meshes;
    const inst_rec* insts;
    const nref_material* mats;
    const rro_params* p;
    nref_tallies* tl;
    uint32_t rays;
    v3 acc;
} ctx;

static void shade(ctx* c, v3 O, v3 D, float tmin, float tmax, media L, uint32_t count, v3 w)
{
    c->rays++;
    if ((uint64_t)L.n > c->tl->deepest) c->tl->deepest = (uint64_t)L.n;
    rro_hit h;
    const float o[3] = { O.x, O.y, O.z }, d[3] = { D.x, D.y, D.z };
    rro_trace(c->s, o, d, tmin, tmax, 0u, c->p->use_bvh, &h);
    if (!h.hit) {                                                          /* Miss: absorbs nothing, whatever L holds */
        float e[3];
        rro_env_lookup(c->s, d, c->p->use_libm, e);
        c->acc.x = fmaf(w.x, e[0], c->acc.x);
        c->acc.y = fmaf(w.y, e[1], c->acc.y);
        c->acc.z = fmaf(w.z, e[2], c->acc.z);
        return;
    }
    if (!(count < (uint32_t)c->p->max_refract)) return;                    /* a hit at the limit adds nothing */
    const inst_rec* ci = &c->insts[h.inst];
    const nref_mesh* me = &c->meshes[ci->mesh];
    const rro_vertex* vA = &me->verts[me->idx[3 * h.prim + 0]];
    const rro_vertex* vB = &me->verts[me->idx[3 * h.prim + 1]];
    const rro_vertex* vC = &me->verts[me->idx[3 * h.prim + 2]];

    /* 1. the medium crossed */
    const int cur = top_of(&L);
    if (cur >= 0) {
        const nref_material* mc = &c->mats[cur];
        w.x = w.x * exp_neg(-(mc->sigma_a[0] * h.t));
        w.y = w.y * exp_neg(-(mc->sigma_a[1] * h.t));
        w.z = w.z * exp_neg(-(mc->sigma_a[2] * h.t));
        c->tl->absorbed[cur]++;
    }

    /* the face: det of the primitive in object space */
    v3 Oo = O, Do = D;
    if (!ci->identity) {
        const float* q = ci->inv;
        Oo = mk(((q[0] * O.x + q[1] * O.y) + q[2] * O.z) + q[3], ((q[4] * O.x + q[5] * O.y) + q[6] * O.z) + q[7],
                ((q[8] * O.x + q[9] * O.y) + q[10] * O.z) + q[11]);
        Do = mk((q[0] * D.x + q[1] * D.y) + q[2] * D.z, (q[4] * D.x + q[5] * D.y) + q[6] * D.z, (q[8] * D.x + q[9] * D.y) + q[10] * D.z);
    }
    (void)Oo;
    const v3 P0 = mk(vA->position[0], vA->position[1], vA->position[2]);
    const v3 e1 = sub(mk(vB->position[0], vB->position[1], vB->position[2]), P0), e2 = sub(mk(vC->position[0], vC->position[1], vC->position[2]), P0);
    const float det = dot(e1, cross(Do, e2));
    const int front = (det > 0.0f) != (ci->ccw != 0);

    /* 2. the list behind the surface */
    media Lp = L;
    const uint32_t m = ci->material;
    if (front) {
        if (Lp.n < MAX_MEDIA) Lp.row[Lp.n++] = m;
        else c->tl->dropped_pushes++;
    } else {
        int at = -1;
        for (int i = 0; i < Lp.n; ++i) if (Lp.row[i] == m) at = i;
        if (at < 0) c->tl->absent_removals++;
        else {
            for (int i = at; i + 1 < Lp.n; ++i) Lp.row[i] = Lp.row[i + 1];
            Lp.n--;
        }
    }
    const int nxt = top_of(&Lp);

    v3 X = mk(fmaf(h.t, D.x, O.x), fmaf(h.t, D.y, O.y), fmaf(h.t, D.z, O.z));  /* 3. */
    const float ts0 = c->p->tmin_secondary, ts1 = c->p->tmax_secondary;
    if (nxt == cur) {                                                      /* 4. not an interface */
        c->tl->passes++;
        shade(c, X, D, ts0, ts1, Lp, count + 1, w);
        return;
    }
    c->tl->interfaces++;                                                   /* 5. an interface */
    const float* nA = vA->norm;                                            /* hlsl:83-85 */
    const float* nB = vB->norm;
    const float* nC = vC->norm;
    v3 A = mk(nA[0], nA[1], nA[2]), BA = sub(mk(nB[0], nB[1], nB[2]), A), CA = sub(mk(nC[0], nC[1], nC[2]), A);
    v3 Nr = mk(fmaf(h.v, CA.x, fmaf(h.u, BA.x, A.x)), fmaf(h.v, CA.y, fmaf(h.u, BA.y, A.y)), fmaf(h.v, CA.z, fmaf(h.u, BA.z, A.z)));
    if (!ci->identity) {                                                   /* inverse transpose of object -> world */
        const float* q = ci->inv;
        Nr = mk((q[0] * Nr.x + q[4] * Nr.y) + q[8] * Nr.z, (q[1] * Nr.x + q[5] * Nr.y) + q[9] * Nr.z, (q[2] * Nr.x + q[6] * Nr.y) + q[10] * Nr.z);
    }
    v3 N = normalize(Nr);
    v3 Nf = front ? N : neg(N);
    const float R0 = (0.2f / 2.2f) * (0.2f / 2.2f);
    float b = 1.0f - dot(D, Nf);
    float b2 = b * b, b4 = b2 * b2;
    float R = (R0 * (1.0f - R0)) * (b4 * b);
    const float n_from = cur >= 0 ? c->mats[cur].ior : 1.0f;
    const float inv_n_to = nxt >= 0 ? 1.0f / c->mats[nxt].ior : 1.0f;
    float eta = n_from * inv_n_to;
    float cs = dot(Nf, D);
    float k = 1.0f - (eta * eta) * (1.0f - cs * cs);
    if (!(k < 0.0f)) {                                                     /* RefractRay, hlsl:70-76 */
        float a = eta * cs + sqrtf(k);
        v3 d1 = normalize(mk(eta * D.x - a * Nf.x, eta * D.y - a * Nf.y, eta * D.z - a * Nf.z));
        float T = 1.0f - R;
        shade(c, X, d1, ts0, ts1, Lp, count + 1, mk(w.x * T, w.y * T, w.z * T));
    }
    if (count < (uint32_t)c->p->max_reflect) {                             /* ReflectRay, hlsl:66-68, 110-122: stays in L */
        float k2 = 2.0f * dot(Nf, D);
        v3 d2 = normalize(mk(D.x - k2 * Nf.x, D.y - k2 * Nf.y, D.z - k2 * Nf.z));
        shade(c, X, d2, ts0, ts1, L, count + 1, mk(w.x * R, w.y * R, w.z * R));
    }
}

/* The ray trees of n rays.  rays: n x 8 floats (origin, tmin, dir, tmax); insts: the records the oracle scene `s` was given (n_insts
 * >= 1), blas indexing meshes; p: bounce limits, secondary interval, use_bvh, use_libm (ior is not read).  out_rgb: n x 3 floats,
 * out_rgba8: n x 4 rro_unorm8 bytes (alpha 255), out_rays: TraceRay calls per tree,
 * tallies: added to; any output but out_rgb and tallies may be null.  Returns 0, or -1 for an instance whose row is not below n_mats
 * or above 254. */
int nref_shade(const rro_scene* s, const nref_mesh* meshes, const rro_instance* insts, uint32_t n_insts, const nref_material* mats,
               uint32_t n_mats, const rro_params* p, const float* rays, uint32_t n, float* out_rgb, uint8_t* out_rgba8, uint32_t* out_rays,
               nref_tallies* tallies)
{
    static const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    inst_rec recs[64];
    if (n_insts == 0 || n_insts > 64 || n_mats == 0 || !tallies) return -1;
    for (uint32_t i = 0; i < n_insts; ++i) {
        inst_rec* r = &recs[i];
        r->identity = memcmp(insts[i].transform, ident, sizeof ident) == 0;
        if (r->identity) memcpy(r->inv, ident, sizeof ident);
        else affine_inverse(insts[i].transform, r->inv);
        r->mesh = (uint32_t)insts[i].blas;
        r->material = insts[i].hitgroup_flags & 0xffffffu;
        r->ccw = ((insts[i].hitgroup_flags >> 24) & 0x2u) != 0;
        if (r->material >= n_mats || r->material > 254u) return -1;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const float* q = rays + 8 * (size_t)i;
        ctx c = { s, meshes, recs, mats, p, tallies, 0, { 0, 0, 0 } };
        media air;
        memset(&air, 0, sizeof air);
        shade(&c, mk(q[0], q[1], q[2]), mk(q[4], q[5], q[6]), q[3], q[7], air, 0, mk(1.0f, 1.0f, 1.0f));    /* RayGen: weight (1, 1, 1), in air */
        out_rgb[3 * (size_t)i + 0] = c.acc.x; out_rgb[3 * (size_t)i + 1] = c.acc.y; out_rgb[3 * (size_t)i + 2] = c.acc.z;
        if (out_rgba8) {
            out_rgba8[4 * (size_t)i + 0] = rro_unorm8(c.acc.x); out_rgba8[4 * (size_t)i + 1] = rro_unorm8(c.acc.y);
            out_rgba8[4 * (size_t)i + 2] = rro_unorm8(c.acc.z); out_rgba8[4 * (size_t)i + 3] = 255;
        }
        if (out_rays) out_rays[i] = c.rays;
    }
    return 0;
}
