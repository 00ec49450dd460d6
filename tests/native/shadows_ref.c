/* shadows_ref.c -- the reference of the ray tree with transparent shadows (tests/shadows_helpers.py compiles and loads it; test
 * infrastructure).
 *
 * The tree of include/rrdxr.h "opaque hit groups" as surfaces_ref.c restates it, with the shadow ray of step b as "transparent
 * shadows" words it.  shadow_k == 0: one first-hit shadow ray over [tmin_secondary, far], occluded iff anything is hit.
 * shadow_k = K >= 1, for a light the hit faces:
 *   T = (1, 1, 1), Ls = L of the radiance ray at the hit, Xs = X, fs = far; then up to K calls of TraceRay(Xs, Ld, [tmin_secondary,
 *   fs], flags 0, closest hit, the light's shadow_mask), each counted:
 *     miss: lit.  Hit on an opaque row: occluded.  Hit on a glass row m at t: c = top(Ls), not air: T = T * exp_neg(-(sigma_c * t));
 *     Ls = front ? push(Ls, m) : remove(Ls, m) (a push onto a full list dropped, an absent row a no-op); Xs = fmaf(t, Ld, Xs),
 *     fs = fs - t; !(fs > tmin_secondary): lit; the K-th call: occluded.
 *   lit: E = fmaf(radiance, (cs * g) * T, E).
 *
 * TraceRay and the Miss lookup are the oracle library's own (rro_trace with flags 0, rro_env_lookup).  rro_trace has no instance
 * mask, so the caller hands one extra oracle scene per light: the instances whose InstanceMask meets the light's shadow_mask, or NULL
 * where none does (every call then misses without a trace).  That scene numbers its instances anew: per light the caller also hands
 * the map from its instance indices to the whole scene's (NULL: the same numbering), through which the row, the winding flag and
 * the object space of a walk's hit are found.  Built with -ffp-contract=off: an operation is fused only where fmaf is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/rr_oracle.h"

#define MAX_MEDIA 4
#define MAX_LIGHTS 8
#define MAX_STEPS 16

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

typedef struct { float ior; float sigma_a[3]; } sref_material;
typedef struct { uint32_t kind; float albedo[3]; float emission[3]; float specular[3]; uint32_t pad[2]; } sref_surface;   /* rr_surface */
typedef struct { float v[3]; uint32_t kind; float radiance[3]; uint32_t shadow_mask; } sref_light;                         /* rr_light */
typedef struct { const rro_vertex* verts; const uint32_t* idx; } sref_mesh;

/* what the trees of one call did: conditions on a fixture, never masks on a comparison */
typedef struct {
    uint64_t interfaces;        /* glass ClosestHits shaded as an interface */
    uint64_t passes;            /* glass ClosestHits that were not an interface */
    uint64_t deepest;           /* the longest list any ray carried */
    uint64_t opaque_hits;       /* ClosestHits shaded by the opaque hit group */
    uint64_t shadow_traced;     /* shadow rays counted */
    uint64_t shadow_occluded;
    uint64_t shadow_lit;
    uint64_t lights_skipped;    /* !(cs > 0) */
    uint64_t specular_children;
    uint64_t specular_then_refracted;   /* interfaces met by a ray that descends from a specular child */
    uint64_t opaque_in_media[MAX_MEDIA + 1];   /* opaque hits by the length of L */
    uint64_t opaque_back;       /* opaque hits on a back face */
    uint64_t light_used[MAX_LIGHTS];    /* per light: shadow rays traced for it */
    uint64_t light_occluded[MAX_LIGHTS];
    /* the walks (shadow_k >= 1) */
    uint64_t walks;                     /* walks begun: shadow_traced counts their calls */
    uint64_t walk_calls[MAX_STEPS + 1]; /* walks by the number of calls they made */
    uint64_t walk_start_media[MAX_MEDIA + 1];   /* walks by the length of the list they start with */
    uint64_t walk_capped;               /* ended occluded by the cap, on a glass hit */
    uint64_t walk_ended_by_fs;          /* ended lit because the interval ran out */
    uint64_t walk_lit_glass[3];         /* lit through 0, 1, >= 2 glass hits */
    uint64_t walk_occluded_after_glass; /* stopped by an opaque row after >= 1 glass hit */
    uint64_t walk_absorbed;             /* glass hits at which a medium was crossed (T changed) */
} sref_tallies;

typedef struct {
    float inv[12];
    int identity, ccw;
    uint32_t mesh, material;
} inst_rec;

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
    const sref_mesh* meshes;
    const inst_rec* insts;
    const sref_material* mats;
    const sref_surface* surfs;
    uint32_t n_surfs;
    const sref_light* lights;
    uint32_t n_lights;
    const float* ambient;
    const rro_scene* const* shadow;     /* per light; NULL: no instance meets its mask */
    const uint32_t* const* shadow_map;  /* per light: instance of that scene -> instance of s; NULL: the same */
    uint32_t shadow_k;
    const rro_params* p;
    sref_tallies* tl;
    uint32_t rays;
    v3 acc;
} ctx;

/* the walk of light i from X towards Ld over [tmin_secondary, far], starting in the list L.  1: lit, *T what the glass lets through */
static int walk(ctx* c, uint32_t i, v3 X, v3 Ld, float far, media L, v3* T)
{
    const float ts0 = c->p->tmin_secondary;
    sref_tallies* tl = c->tl;
    *T = mk(1.0f, 1.0f, 1.0f);
    media Ls = L;
    v3 Xs = X;
    float fs = far;
    uint32_t glass = 0, calls = 0;
    int lit = 0;
    tl->walks++;
    tl->walk_start_media[L.n]++;
    for (uint32_t k = 0; k < c->shadow_k; ++k) {
        c->rays++;
        tl->shadow_traced++;
        calls++;
        rro_hit hs;
        hs.hit = 0;
        if (c->shadow[i]) {
            const float xo[3] = { Xs.x, Xs.y, Xs.z }, xd[3] = { Ld.x, Ld.y, Ld.z };
            rro_trace(c->shadow[i], xo, xd, ts0, fs, 0u, c->p->use_bvh, &hs);
        }
        if (!hs.hit) { lit = 1; break; }
        const inst_rec* ci = &c->insts[c->shadow_map[i] ? c->shadow_map[i][hs.inst] : hs.inst];
        const uint32_t m = ci->material;
        if (m < c->n_surfs && c->surfs[m].kind == 1u) {                    /* an opaque row stops the walk */
            if (glass) tl->walk_occluded_after_glass++;
            break;
        }
        glass++;
        const int cur = top_of(&Ls);                                       /* 1. the medium crossed */
        if (cur >= 0) {
            const sref_material* mc = &c->mats[cur];
            T->x = T->x * exp_neg(-(mc->sigma_a[0] * hs.t));
            T->y = T->y * exp_neg(-(mc->sigma_a[1] * hs.t));
            T->z = T->z * exp_neg(-(mc->sigma_a[2] * hs.t));
            tl->walk_absorbed++;
        }
        const sref_mesh* me = &c->meshes[ci->mesh];                        /* 2. the face: det of the primitive in object space */
        const rro_vertex* vA = &me->verts[me->idx[3 * hs.prim + 0]];
        const rro_vertex* vB = &me->verts[me->idx[3 * hs.prim + 1]];
        const rro_vertex* vC = &me->verts[me->idx[3 * hs.prim + 2]];
        v3 Do = Ld;
        if (!ci->identity) {
            const float* q = ci->inv;
            Do = mk((q[0] * Ld.x + q[1] * Ld.y) + q[2] * Ld.z, (q[4] * Ld.x + q[5] * Ld.y) + q[6] * Ld.z, (q[8] * Ld.x + q[9] * Ld.y) + q[10] * Ld.z);
        }
        const v3 P0 = mk(vA->position[0], vA->position[1], vA->position[2]);
        const v3 e1 = sub(mk(vB->position[0], vB->position[1], vB->position[2]), P0), e2 = sub(mk(vC->position[0], vC->position[1], vC->position[2]), P0);
        const int front = (dot(e1, cross(Do, e2)) > 0.0f) != (ci->ccw != 0);
        if (front) {
            if (Ls.n < MAX_MEDIA) Ls.row[Ls.n++] = m;
        } else {
            int at = -1;
            for (int j = 0; j < Ls.n; ++j) if (Ls.row[j] == m) at = j;
            if (at >= 0) {
                for (int j = at; j + 1 < Ls.n; ++j) Ls.row[j] = Ls.row[j + 1];
                Ls.n--;
            }
        }
        Xs = mk(fmaf(hs.t, Ld.x, Xs.x), fmaf(hs.t, Ld.y, Xs.y), fmaf(hs.t, Ld.z, Xs.z));      /* 3. */
        fs = fs - hs.t;
        if (!(fs > ts0)) { lit = 1; tl->walk_ended_by_fs++; break; }       /* 4. */
        if (k + 1 == c->shadow_k) tl->walk_capped++;                       /* 5. the loop ends occluded */
    }
    tl->walk_calls[calls]++;
    if (lit) tl->walk_lit_glass[glass < 2 ? glass : 2]++;
    return lit;
}

static void shade(ctx* c, v3 O, v3 D, float tmin, float tmax, media L, uint32_t count, v3 w, int from_specular)
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
    const sref_mesh* me = &c->meshes[ci->mesh];
    const rro_vertex* vA = &me->verts[me->idx[3 * h.prim + 0]];
    const rro_vertex* vB = &me->verts[me->idx[3 * h.prim + 1]];
    const rro_vertex* vC = &me->verts[me->idx[3 * h.prim + 2]];

    /* 1. the medium crossed */
    const int cur = top_of(&L);
    if (cur >= 0) {
        const sref_material* mc = &c->mats[cur];
        w.x = w.x * exp_neg(-(mc->sigma_a[0] * h.t));
        w.y = w.y * exp_neg(-(mc->sigma_a[1] * h.t));
        w.z = w.z * exp_neg(-(mc->sigma_a[2] * h.t));
    }

    /* the face: det of the primitive in object space */
    v3 Do = D;
    if (!ci->identity) {
        const float* q = ci->inv;
        Do = mk((q[0] * D.x + q[1] * D.y) + q[2] * D.z, (q[4] * D.x + q[5] * D.y) + q[6] * D.z, (q[8] * D.x + q[9] * D.y) + q[10] * D.z);
    }
    const v3 P0 = mk(vA->position[0], vA->position[1], vA->position[2]);
    const v3 e1 = sub(mk(vB->position[0], vB->position[1], vB->position[2]), P0), e2 = sub(mk(vC->position[0], vC->position[1], vC->position[2]), P0);
    const float det = dot(e1, cross(Do, e2));
    const int front = (det > 0.0f) != (ci->ccw != 0);

    /* the shading normal (hlsl:83-85), which both hit groups use; computing it early rounds nothing differently */
    const float* nA = vA->norm;
    const float* nB = vB->norm;
    const float* nC = vC->norm;
    v3 A = mk(nA[0], nA[1], nA[2]), BA = sub(mk(nB[0], nB[1], nB[2]), A), CA = sub(mk(nC[0], nC[1], nC[2]), A);
    v3 Nr = mk(fmaf(h.v, CA.x, fmaf(h.u, BA.x, A.x)), fmaf(h.v, CA.y, fmaf(h.u, BA.y, A.y)), fmaf(h.v, CA.z, fmaf(h.u, BA.z, A.z)));
    if (!ci->identity) {                                                   /* inverse transpose of object -> world */
        const float* q = ci->inv;
        Nr = mk((q[0] * Nr.x + q[4] * Nr.y) + q[8] * Nr.z, (q[1] * Nr.x + q[5] * Nr.y) + q[9] * Nr.z, (q[2] * Nr.x + q[6] * Nr.y) + q[10] * Nr.z);
    }
    const v3 N = normalize(Nr);
    const v3 Nf = front ? N : neg(N);
    const v3 X = mk(fmaf(h.t, D.x, O.x), fmaf(h.t, D.y, O.y), fmaf(h.t, D.z, O.z));
    const float ts0 = c->p->tmin_secondary, ts1 = c->p->tmax_secondary;
    const uint32_t m = ci->material;

    if (m < c->n_surfs && c->surfs[m].kind == 1u) {                        /* the opaque hit group */
        const sref_surface* sf = &c->surfs[m];
        c->tl->opaque_hits++;
        c->tl->opaque_in_media[L.n]++;
        if (!front) c->tl->opaque_back++;
        float E[3] = { c->ambient[0], c->ambient[1], c->ambient[2] };
        for (uint32_t i = 0; i < c->n_lights; ++i) {
            const sref_light* lt = &c->lights[i];
            v3 Ld = mk(lt->v[0], lt->v[1], lt->v[2]);
            float far = ts1, g = 1.0f;
            if (lt->kind == 1u) {
                const v3 dd = mk(lt->v[0] - X.x, lt->v[1] - X.y, lt->v[2] - X.z);
                const float d2 = dot(dd, dd);
                far = sqrtf(d2);
                Ld = mk(dd.x / far, dd.y / far, dd.z / far);
                g = 1.0f / d2;
            }
            const float cs = dot(Nf, Ld);
            if (!(cs > 0.0f)) { c->tl->lights_skipped++; continue; }
            c->tl->light_used[i]++;
            if (c->shadow_k == 0) {                                         /* one first-hit ray: anything occludes */
                c->rays++;
                c->tl->shadow_traced++;
                int occluded = 0;
                if (c->shadow[i]) {
                    rro_hit hs;
                    const float xo[3] = { X.x, X.y, X.z }, xd[3] = { Ld.x, Ld.y, Ld.z };
                    rro_trace(c->shadow[i], xo, xd, ts0, far, 0u, c->p->use_bvh, &hs);
                    occluded = hs.hit != 0;
                }
                if (occluded) { c->tl->shadow_occluded++; c->tl->light_occluded[i]++; continue; }
                c->tl->shadow_lit++;
                const float f = cs * g;
                E[0] = fmaf(lt->radiance[0], f, E[0]); E[1] = fmaf(lt->radiance[1], f, E[1]); E[2] = fmaf(lt->radiance[2], f, E[2]);
                continue;
            }
            v3 T;
            if (!walk(c, i, X, Ld, far, L, &T)) { c->tl->shadow_occluded++; c->tl->light_occluded[i]++; continue; }
            c->tl->shadow_lit++;
            const float f = cs * g;
            E[0] = fmaf(lt->radiance[0], f * T.x, E[0]); E[1] = fmaf(lt->radiance[1], f * T.y, E[1]); E[2] = fmaf(lt->radiance[2], f * T.z, E[2]);
        }
        const v3 col = mk(fmaf(sf->albedo[0], E[0], sf->emission[0]), fmaf(sf->albedo[1], E[1], sf->emission[1]), fmaf(sf->albedo[2], E[2], sf->emission[2]));
        c->acc.x = fmaf(w.x, col.x, c->acc.x);
        c->acc.y = fmaf(w.y, col.y, c->acc.y);
        c->acc.z = fmaf(w.z, col.z, c->acc.z);
        if (sf->specular[0] != 0.0f || sf->specular[1] != 0.0f || sf->specular[2] != 0.0f) {
            c->tl->specular_children++;
            float k2 = 2.0f * dot(Nf, D);
            v3 d2 = normalize(mk(D.x - k2 * Nf.x, D.y - k2 * Nf.y, D.z - k2 * Nf.z));
            shade(c, X, d2, ts0, ts1, L, count + 1, mk(w.x * sf->specular[0], w.y * sf->specular[1], w.z * sf->specular[2]), 1);
        }
        return;
    }

    /* 2. the list behind the surface */
    media Lp = L;
    if (front) {
        if (Lp.n < MAX_MEDIA) Lp.row[Lp.n++] = m;
    } else {
        int at = -1;
        for (int i = 0; i < Lp.n; ++i) if (Lp.row[i] == m) at = i;
        if (at >= 0) {
            for (int i = at; i + 1 < Lp.n; ++i) Lp.row[i] = Lp.row[i + 1];
            Lp.n--;
        }
    }
    const int nxt = top_of(&Lp);
    if (nxt == cur) {                                                      /* 4. not an interface */
        c->tl->passes++;
        shade(c, X, D, ts0, ts1, Lp, count + 1, w, from_specular);
        return;
    }
    c->tl->interfaces++;                                                   /* 5. an interface */
    if (from_specular) c->tl->specular_then_refracted++;
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
        shade(c, X, d1, ts0, ts1, Lp, count + 1, mk(w.x * T, w.y * T, w.z * T), from_specular);
    }
    if (count < (uint32_t)c->p->max_reflect) {                             /* ReflectRay, hlsl:66-68, 110-122: stays in L */
        float k2 = 2.0f * dot(Nf, D);
        v3 d2 = normalize(mk(D.x - k2 * Nf.x, D.y - k2 * Nf.y, D.z - k2 * Nf.z));
        shade(c, X, d2, ts0, ts1, L, count + 1, mk(w.x * R, w.y * R, w.z * R), from_specular);
    }
}

/* The ray trees of n rays.  rays: n x 8 floats (origin, tmin, dir, tmax); insts: the records the oracle scene `s` was given (n_insts
 * >= 1), blas indexing meshes; surfs: n_surfs rows (0: all glass); lights: n_lights rows, shadow: one oracle scene or NULL per light,
 * shadow_map: per light the instance of s behind each instance of that scene, or NULL for the same numbering; shadow_k: 0 ..
 * MAX_STEPS; ambient: three floats; p: bounce limits, secondary interval, use_bvh, use_libm.  out_rgb: n x 3 floats, out_rgba8: n x 4 rro_unorm8
 * bytes (alpha 255), out_rays: TraceRay calls per tree, shadow rays included; tallies: added to.  Returns 0, or -1 for what the
 * library would refuse. */
int shref_shade(const rro_scene* s, const sref_mesh* meshes, const rro_instance* insts, uint32_t n_insts, const sref_material* mats,
               uint32_t n_mats, const sref_surface* surfs, uint32_t n_surfs, const sref_light* lights, uint32_t n_lights, const float* ambient,
               const rro_scene* const* shadow, const uint32_t* const* shadow_map, uint32_t shadow_k, const rro_params* p, const float* rays, uint32_t n, float* out_rgb, uint8_t* out_rgba8,
               uint32_t* out_rays, sref_tallies* tallies)
{
    static const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    inst_rec recs[64];
    if (n_insts == 0 || n_insts > 64 || n_mats == 0 || n_lights > MAX_LIGHTS || !tallies || !ambient || shadow_k > MAX_STEPS || !shadow || !shadow_map) return -1;
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
        ctx c = { s, meshes, recs, mats, surfs, n_surfs, lights, n_lights, ambient, shadow, shadow_map, shadow_k, p, tallies, 0, { 0, 0, 0 } };
        media air;
        memset(&air, 0, sizeof air);
        shade(&c, mk(q[0], q[1], q[2]), mk(q[4], q[5], q[6]), q[3], q[7], air, 0, mk(1.0f, 1.0f, 1.0f), 0);    /* RayGen: weight (1, 1, 1), in air */
        out_rgb[3 * (size_t)i + 0] = c.acc.x; out_rgb[3 * (size_t)i + 1] = c.acc.y; out_rgb[3 * (size_t)i + 2] = c.acc.z;
        if (out_rgba8) {
            out_rgba8[4 * (size_t)i + 0] = rro_unorm8(c.acc.x); out_rgba8[4 * (size_t)i + 1] = rro_unorm8(c.acc.y);
            out_rgba8[4 * (size_t)i + 2] = rro_unorm8(c.acc.z); out_rgba8[4 * (size_t)i + 3] = 255;
        }
        if (out_rays) out_rays[i] = c.rays;
    }
    return 0;
}
