// rr_host_camera.cpp -- the per-frame camera constants of RefractionDemo::drawFrame
// (RefractionDemo.cpp:559-566), host side, no device; and the primary rays of the supersampled and thin-lens frames.
//
// The reference computes them with DirectXMath (Windows SDK header, not in its tree):
//   proj  = XMMatrixPerspectiveFovLH(52/180*3.1415, 1.333, 1, 125)          :559
//   loc   = (5 cos a, 0, 5 sin a, 1)                                       :560
//   world = XMMatrixTranslationFromVector(loc)                             :561
//   view  = XMMatrixLookAtLH((cos -a, 0, sin -a), origin, +Y)              :562
//   proj_inv = XMMatrixInverse(proj * world * view)                        :563-565
// DirectXMath's published algorithms are restated here in fp32 with its row-vector convention.
#include "../../../include/rrdxr.h"
#include "rr_host_lens.h"

#include <cmath>
#include <cstring>

namespace {

struct Vec3 { float x, y, z; };
struct Mat4 {
    float r[4][4];
    static Mat4 zero() { Mat4 m; std::memset(&m, 0, sizeof m); return m; }
    static Mat4 identity() { Mat4 m = zero(); m.r[0][0] = m.r[1][1] = m.r[2][2] = m.r[3][3] = 1.0f; return m; }
};

Vec3 operator-(Vec3 a, Vec3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
float dot(Vec3 a, Vec3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
Vec3 cross(Vec3 a, Vec3 b)
{
    return { fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)) };
}
Vec3 normalized(Vec3 a)
{
    float s = 1.0f / std::sqrt(dot(a, a));
    return { a.x * s, a.y * s, a.z * s };
}

// XMScalarSinCos: range reduction to [-pi/2, pi/2] + 11th/10th-degree minimax polynomials
void scalar_sin_cos(float v, float& s, float& c)
{
    float q = 0.159154943f * v;
    q = v >= 0.0f ? (float)(int)(q + 0.5f) : (float)(int)(q - 0.5f);
    float y = v - 6.283185307f * q;
    float sign = 1.0f;
    if (y > 1.570796327f) { y = 3.141592654f - y; sign = -1.0f; }
    else if (y < -1.570796327f) { y = -3.141592654f - y; sign = -1.0f; }
    const float y2 = y * y;
    s = (((((-2.3889859e-08f * y2 + 2.7525562e-06f) * y2 - 0.00019840874f) * y2 + 0.0083333310f) * y2 - 0.16666667f) * y2 + 1.0f) * y;
    c = sign * (((((-2.6051615e-07f * y2 + 2.4760495e-05f) * y2 - 0.0013888378f) * y2 + 0.041666638f) * y2 - 0.5f) * y2 + 1.0f);
}

// XMMatrixMultiply, SSE summation order: (x*m0 + z*m2) + (y*m1 + w*m3)
Mat4 mul(const Mat4& a, const Mat4& b)
{
    Mat4 o;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            o.r[i][j] = (a.r[i][0] * b.r[0][j] + a.r[i][2] * b.r[2][j]) + (a.r[i][1] * b.r[1][j] + a.r[i][3] * b.r[3][j]);
    return o;
}

// general 4x4 inverse by 2x2 sub-determinants (Laplace expansion over row pairs)
bool inverse(const Mat4& m, Mat4& out)
{
    const float (*a)[4] = m.r;
    const float s0 = a[0][0] * a[1][1] - a[1][0] * a[0][1];
    const float s1 = a[0][0] * a[1][2] - a[1][0] * a[0][2];
    const float s2 = a[0][0] * a[1][3] - a[1][0] * a[0][3];
    const float s3 = a[0][1] * a[1][2] - a[1][1] * a[0][2];
    const float s4 = a[0][1] * a[1][3] - a[1][1] * a[0][3];
    const float s5 = a[0][2] * a[1][3] - a[1][2] * a[0][3];
    const float c5 = a[2][2] * a[3][3] - a[3][2] * a[2][3];
    const float c4 = a[2][1] * a[3][3] - a[3][1] * a[2][3];
    const float c3 = a[2][1] * a[3][2] - a[3][1] * a[2][2];
    const float c2 = a[2][0] * a[3][3] - a[3][0] * a[2][3];
    const float c1 = a[2][0] * a[3][2] - a[3][0] * a[2][2];
    const float c0 = a[2][0] * a[3][1] - a[3][0] * a[2][1];
    const float det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    if (det == 0.0f || !std::isfinite(det)) return false;
    const float id = 1.0f / det;
    float (*b)[4] = out.r;
    b[0][0] = ( a[1][1] * c5 - a[1][2] * c4 + a[1][3] * c3) * id;
    b[0][1] = (-a[0][1] * c5 + a[0][2] * c4 - a[0][3] * c3) * id;
    b[0][2] = ( a[3][1] * s5 - a[3][2] * s4 + a[3][3] * s3) * id;
    b[0][3] = (-a[2][1] * s5 + a[2][2] * s4 - a[2][3] * s3) * id;
    b[1][0] = (-a[1][0] * c5 + a[1][2] * c2 - a[1][3] * c1) * id;
    b[1][1] = ( a[0][0] * c5 - a[0][2] * c2 + a[0][3] * c1) * id;
    b[1][2] = (-a[3][0] * s5 + a[3][2] * s2 - a[3][3] * s1) * id;
    b[1][3] = ( a[2][0] * s5 - a[2][2] * s2 + a[2][3] * s1) * id;
    b[2][0] = ( a[1][0] * c4 - a[1][1] * c2 + a[1][3] * c0) * id;
    b[2][1] = (-a[0][0] * c4 + a[0][1] * c2 - a[0][3] * c0) * id;
    b[2][2] = ( a[3][0] * s4 - a[3][1] * s2 + a[3][3] * s0) * id;
    b[2][3] = (-a[2][0] * s4 + a[2][1] * s2 - a[2][3] * s0) * id;
    b[3][0] = (-a[1][0] * c3 + a[1][1] * c1 - a[1][2] * c0) * id;
    b[3][1] = ( a[0][0] * c3 - a[0][1] * c1 + a[0][2] * c0) * id;
    b[3][2] = (-a[3][0] * s3 + a[3][1] * s1 - a[3][2] * s0) * id;
    b[3][3] = ( a[2][0] * s3 - a[2][1] * s1 + a[2][2] * s0) * id;
    return true;
}

} // namespace

extern "C" int rr_host_camera_orbit(float angle, float fov_y, float aspect, float zn, float zf, rr_scene_constants* out)
{
    if (!out || !(fov_y > 0.0f) || !(aspect > 0.0f) || zn == zf) return RR_ERR_INVALID_ARGUMENT;

    // XMMatrixPerspectiveFovLH
    float sf, cf;
    scalar_sin_cos(0.5f * fov_y, sf, cf);
    const float h = cf / sf, w = h / aspect, range = zf / (zf - zn);
    Mat4 proj = Mat4::zero();
    proj.r[0][0] = w; proj.r[1][1] = h; proj.r[2][2] = range; proj.r[2][3] = 1.0f; proj.r[3][2] = -range * zn;

    // camera_loc and the translation "world" matrix
    const float loc[4] = { 5 * cosf(angle), 0.0f, 5 * sinf(angle), 1.0f };
    Mat4 world = Mat4::identity();
    world.r[3][0] = loc[0]; world.r[3][1] = loc[1]; world.r[3][2] = loc[2];

    // XMMatrixLookAtLH -> XMMatrixLookToLH(eye, focus - eye, up)
    const Vec3 eye = { cosf(-angle), 0.0f, sinf(-angle) };
    const Vec3 up = { 0.0f, 1.0f, 0.0f };
    const Vec3 zaxis = normalized(Vec3{ 0.0f, 0.0f, 0.0f } - eye);
    const Vec3 xaxis = normalized(cross(up, zaxis));
    const Vec3 yaxis = cross(zaxis, xaxis);
    const Vec3 neg_eye = { -eye.x, -eye.y, -eye.z };
    Mat4 view = Mat4::identity();
    view.r[0][0] = xaxis.x; view.r[1][0] = xaxis.y; view.r[2][0] = xaxis.z; view.r[3][0] = dot(xaxis, neg_eye);
    view.r[0][1] = yaxis.x; view.r[1][1] = yaxis.y; view.r[2][1] = yaxis.z; view.r[3][1] = dot(yaxis, neg_eye);
    view.r[0][2] = zaxis.x; view.r[1][2] = zaxis.y; view.r[2][2] = zaxis.z; view.r[3][2] = dot(zaxis, neg_eye);

    Mat4 inv;
    if (!inverse(mul(mul(proj, world), view), inv)) return RR_ERR_INVALID_ARGUMENT;
    std::memcpy(out->proj_inv, inv.r, 64);
    std::memcpy(out->camera_loc, loc, 16);
    return RR_OK;
}

// D3D's standard multisample patterns: sample i at 0.5 + k / 16 per axis
extern "C" int rr_host_sample_pattern(uint32_t n_samples, float* offsets)
{
    static const int8_t p1[] = { 0, 0 };
    static const int8_t p2[] = { 4, 4, -4, -4 };
    static const int8_t p4[] = { -2, -6, 6, -2, -6, 2, 2, 6 };
    static const int8_t p8[] = { 1, -3, -1, 3, 5, 1, -3, -5, -5, 5, -7, -1, 3, 7, 7, -7 };
    static const int8_t p16[] = { 1, 1, -1, -3, -3, 2, 4, -1, -5, -2, 2, 5, 5, 3, 3, -5, -2, 6, 0, -7, -4, -6, -6, 4, -8, 0, 7, -4, 6, 7, -7, -8 };
    const int8_t* k = n_samples == 1 ? p1 : n_samples == 2 ? p2 : n_samples == 4 ? p4 : n_samples == 8 ? p8 : n_samples == 16 ? p16 : nullptr;
    if (!k || !offsets) return RR_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < 2 * n_samples; ++i) offsets[i] = 0.5f + (float)k[i] / 16.0f;
    return RR_OK;
}

// The built-in band table of rr_render_spectral: n bands at the midpoints of n equal slices of 400..700 nm, Cauchy's law through
// ior_d at the d line (587.6 nm) with the Abbe number over the F (486.1) and C (656.3) lines, and three tent functions of
// half-width 100 nm round 650, 550 and 450 nm as channel weights, each normalised to sum to n.  All in double, rounded once.
extern "C" int rr_host_spectral_bands(uint32_t n, float ior_d, float abbe, rr_band* bands)
{
    if (n == 0 || n > RR_MAX_SAMPLES || !bands) return RR_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(ior_d) || !(ior_d > 0.0f) || !(abbe > 0.0f)) return RR_ERR_INVALID_ARGUMENT;      // (NaN fails the comparisons; abbe may be +inf)
    if (n == 1) { bands[0] = rr_band{ ior_d, { 1.0f, 1.0f, 1.0f } }; return RR_OK; }
    const double B = ((double)ior_d - 1.0) / ((double)abbe * (1.0 / (486.1 * 486.1) - 1.0 / (656.3 * 656.3)));
    const double A = (double)ior_d - B / (587.6 * 587.6);
    static const double centre[3] = { 650.0, 550.0, 450.0 };
    double tent[RR_MAX_SAMPLES][3], total[3] = { 0.0, 0.0, 0.0 };
    for (uint32_t i = 0; i < n; ++i) {
        const double l = 400.0 + ((double)i + 0.5) / (double)n * 300.0;
        bands[i].ior = (float)(A + B / (l * l));
        if (!std::isfinite(bands[i].ior) || !(bands[i].ior > 0.0f)) return RR_ERR_INVALID_ARGUMENT;     // (an Abbe number too small for ior_d)
        for (int c = 0; c < 3; ++c) {
            tent[i][c] = std::fmax(0.0, 1.0 - std::fabs(l - centre[c]) / 100.0);
            total[c] += tent[i][c];
        }
    }
    for (uint32_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) bands[i].weight[c] = (float)(tent[i][c] * (double)n / total[c]);
    return RR_OK;
}

// GenerateCameraRay (RayTracing.hlsl:27-40) for every pixel of a frame, with the literal 0.5 replaced by (ox, oy): the
// arithmetic of k_render_samples' sample ray (screen_coord of rr_frame.hip and camera_ray_dir of rr_device.h), operation by operation
extern "C" int rr_host_camera_rays(const rr_scene_constants* c, uint32_t width, uint32_t height, float ox, float oy, float tmin, float tmax,
                                   rr_ray* rays)
{
    if (!c || !rays || width == 0 || height == 0 || width > 32768u || height > 32768u) return RR_ERR_INVALID_ARGUMENT;
    if (!(ox >= 0.0f && ox <= 1.0f && oy >= 0.0f && oy <= 1.0f)) return RR_ERR_INVALID_ARGUMENT;        // (NaN fails every comparison)
    const float* M = c->proj_inv;
    for (uint32_t y = 0; y < height; ++y) {
        const float py = (float)y + oy;
        const float sy = -(py / (float)height * 2.0f - 1.0f);
        for (uint32_t x = 0; x < width; ++x) {
            const float px = (float)x + ox;
            const float sx = px / (float)width * 2.0f - 1.0f;
            const Vec3 d = normalized(Vec3{ (sx * M[0] + sy * M[1]) + M[3], (sx * M[4] + sy * M[5]) + M[7], (sx * M[8] + sy * M[9]) + M[11] });
            rr_ray& r = rays[(size_t)y * width + x];
            std::memset(&r, 0, sizeof r);
            r.origin[0] = c->camera_loc[0]; r.origin[1] = c->camera_loc[1]; r.origin[2] = c->camera_loc[2];
            r.tmin = tmin;
            r.dir[0] = d.x; r.dir[1] = d.y; r.dir[2] = d.z;
            r.tmax = tmax;
            r.instance_mask = 0xffu;
        }
    }
    return RR_OK;
}

// ---- the thin lens of rr_render_lens ----
namespace {
float length(Vec3 a) { return std::sqrt(dot(a, a)); }
bool usable(float len) { return std::isfinite(len) && len > 0.0f; }
bool in_unit(float v) { return v >= -1.0f && v <= 1.0f; }       // (NaN fails both comparisons)
} // namespace

int rr::lens_setup(const rr_scene_constants* c, const rr_lens* lens, rr::LensDev* out)
{
    if (!c || !lens || !out) return RR_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(lens->radius) || !(lens->radius >= 0.0f)) return RR_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(lens->focus_distance) || !(lens->focus_distance > 0.0f)) return RR_ERR_INVALID_ARGUMENT;
    const float* M = c->proj_inv;
    const Vec3 u = { M[0], M[4], M[8] }, v = { M[1], M[5], M[9] }, w = { M[3], M[7], M[11] };
    const float lw = length(w);
    if (!usable(lw)) return RR_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof *out);
    out->s = lens->focus_distance / lw;
    if (!usable(out->s)) return RR_ERR_INVALID_ARGUMENT;
    out->pinhole = lens->radius == 0.0f ? 1u : 0u;
    if (out->pinhole) return RR_OK;
    if (!usable(length(u)) || !usable(length(v))) return RR_ERR_INVALID_ARGUMENT;
    const Vec3 a = normalized(u), b = normalized(v);
    out->A[0] = lens->radius * a.x; out->A[1] = lens->radius * a.y; out->A[2] = lens->radius * a.z;
    out->B[0] = lens->radius * b.x; out->B[1] = lens->radius * b.y; out->B[2] = lens->radius * b.z;
    for (int i = 0; i < 3; ++i) if (!std::isfinite(out->A[i]) || !std::isfinite(out->B[i])) return RR_ERR_INVALID_ARGUMENT;
    return RR_OK;
}

// point i of a golden-angle spiral inside the unit disk
extern "C" int rr_host_lens_pattern(uint32_t n_samples, float* lens_offsets)
{
    if (n_samples == 0 || n_samples > RR_MAX_SAMPLES || !lens_offsets) return RR_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n_samples; ++i) {
        const float r = sqrtf(((float)i + 0.5f) / (float)n_samples), theta = (float)i * 2.3999632f;
        lens_offsets[2 * i] = r * cosf(theta);
        lens_offsets[2 * i + 1] = r * sinf(theta);
    }
    return RR_OK;
}

// lens_ray of rr_render_common.h for every pixel of a frame, operation by operation: the ray from the lens point
// camera_loc + lx * A + ly * B through the point s * R of the focal plane, R being GenerateCameraRay's un-normalised vector
extern "C" int rr_host_lens_rays(const rr_scene_constants* c, uint32_t width, uint32_t height, float ox, float oy, float lx, float ly,
                                 const rr_lens* lens, float tmin, float tmax, rr_ray* rays)
{
    if (!c || !rays || width == 0 || height == 0 || width > 32768u || height > 32768u) return RR_ERR_INVALID_ARGUMENT;
    if (!(ox >= 0.0f && ox <= 1.0f && oy >= 0.0f && oy <= 1.0f) || !in_unit(lx) || !in_unit(ly)) return RR_ERR_INVALID_ARGUMENT;
    rr::LensDev L;
    if (int r = rr::lens_setup(c, lens, &L)) return r;
    if (L.pinhole) return rr_host_camera_rays(c, width, height, ox, oy, tmin, tmax, rays);
    const float* M = c->proj_inv;
    const Vec3 off = { lx * L.A[0] + ly * L.B[0], lx * L.A[1] + ly * L.B[1], lx * L.A[2] + ly * L.B[2] };
    const Vec3 org = { c->camera_loc[0] + off.x, c->camera_loc[1] + off.y, c->camera_loc[2] + off.z };
    for (uint32_t y = 0; y < height; ++y) {
        const float py = (float)y + oy;
        const float sy = -(py / (float)height * 2.0f - 1.0f);
        for (uint32_t x = 0; x < width; ++x) {
            const float px = (float)x + ox;
            const float sx = px / (float)width * 2.0f - 1.0f;
            const Vec3 R = { (sx * M[0] + sy * M[1]) + M[3], (sx * M[4] + sy * M[5]) + M[7], (sx * M[8] + sy * M[9]) + M[11] };
            const Vec3 d = normalized(Vec3{ L.s * R.x - off.x, L.s * R.y - off.y, L.s * R.z - off.z });
            rr_ray& r = rays[(size_t)y * width + x];
            std::memset(&r, 0, sizeof r);
            r.origin[0] = org.x; r.origin[1] = org.y; r.origin[2] = org.z;
            r.tmin = tmin;
            r.dir[0] = d.x; r.dir[1] = d.y; r.dir[2] = d.z;
            r.tmax = tmax;
            r.instance_mask = 0xffu;
        }
    }
    return RR_OK;
}
