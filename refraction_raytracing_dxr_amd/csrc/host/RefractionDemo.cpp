// RefractionDemo.cpp -- the reference's frame driver (RefractionDemo.cpp:513-612) over the rrdxr
// C ABI.  Same call order as the reference's initialize(): device, env map, mesh load + upload,
// acceleration structures, then per frame: camera constants, DispatchRays, copy out, wait.
#include "RefractionDemo.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace RefractionDemo {
namespace {
rr_context* g_ctx = nullptr;
Mesh cubeMesh;                               // the reference's name for its one mesh (RefractionDemo.cpp:17)
Options g_opt;
float g_angle = 0.01f;                       // static float angle (RefractionDemo.cpp:555)
std::vector<uint8_t> g_back;
bool g_back_pinned = false;
std::string g_err;
void* g_comm = nullptr;                      // RCCL communicator of the sharded form
int g_rank = 0, g_world = 1;
std::vector<rr_material> g_mats;             // the table of setMaterials: drawFrameComposed derives its band set from it
std::vector<rr_material> g_table;            // the table in force where it is not g_mats: setFloorAndLights appends the floor's row
std::vector<rr_instance_desc> g_floor_inst;  // the two instances of setFloorAndLights: drawFrameLit turns them per key
std::vector<rr_light> g_lights;              // the lights of setFloorAndLights: setLightSoftness shapes the point lights among them
bool g_shutter_tlas = false;                 // drawFrameShutter built the top level it updates per key

int fail(int code, const char* what)
{
    g_err = what;
    if (g_ctx && code != RR_ERR_IO) { g_err += ": "; g_err += rr_last_error(g_ctx); }
    return code;
}
} // namespace

int initialize(const Options& opt)
{
    shutdown();
    g_opt = opt;
    g_angle = opt.angle0;
    g_shutter_tlas = false;
    int rc = rr_create(opt.device, &g_ctx);                               // createDevice :142-172
    if (rc != RR_OK) return fail(rc, "rr_create");

    int x = 0, y = 0, n = 0;                                              // load_texture :108-140
    float* env = rr_host_image_loadf(opt.env_path.c_str(), &x, &y, &n, 3);
    if (!env) return fail(RR_ERR_IO, "env map could not be loaded");      // the reference does not check (:111)
    rc = rr_upload_envmap(g_ctx, env, x, y);
    rr_host_free(env);
    if (rc != RR_OK) return fail(rc, "rr_upload_envmap");

    cubeMesh = Mesh();
    if (!cubeMesh.load(opt.mesh_path.c_str())) return fail(RR_ERR_IO, "mesh could not be loaded");   // :537
    if ((rc = cubeMesh.upload(g_ctx)) != RR_OK) return fail(rc, "Mesh::upload");                      // :538

    // setupRaytracingAccelerationStructures :272-361: one BLAS, one identity instance, mask 1, flags 0
    const RaytracingGeometry geo = cubeMesh.raytracingGeometry();
    if ((rc = rr_build_blas(g_ctx, geo.mesh_id)) != RR_OK) return fail(rc, "rr_build_blas");
    rr_instance_desc inst;
    std::memset(&inst, 0, sizeof inst);
    inst.transform[0] = inst.transform[5] = inst.transform[10] = 1.0f;    // :325-327
    inst.instance_id_mask = 1u << 24;                                     // InstanceMask = 1, InstanceID = 0
    inst.hitgroup_flags = 0;
    inst.blas = geo.mesh_id;
    if ((rc = rr_build_tlas(g_ctx, &inst, 1)) != RR_OK) return fail(rc, "rr_build_tlas");

    if (g_back_pinned) { rr_host_unregister(g_ctx, g_back.data()); g_back_pinned = false; }
    g_back.assign((size_t)opt.width * opt.height * 4, 0);
    g_back_pinned = rr_host_register(g_ctx, g_back.data(), g_back.size()) == RR_OK;     // best effort: pageable works too
    return RR_OK;
}

int drawFrame()
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);      // :559-565
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    if ((rc = rr_set_camera(g_ctx, &sc)) != RR_OK) return fail(rc, "rr_set_camera");                  // :566
    g_angle += g_opt.angle_step;                                                                      // :567
    if ((rc = rr_dispatch_rays(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &g_opt.dispatch)) != RR_OK)
        return fail(rc, "rr_dispatch_rays");                                                          // :580-594
    if ((rc = rr_read_frame(g_ctx, g_back.data(), nullptr)) != RR_OK) return fail(rc, "rr_read_frame");   // :596-611
    return RR_OK;
}

int drawFrameSamples(int spp)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (spp <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameSamples: spp must be 1, 2, 4, 8 or 16");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    g_angle += g_opt.angle_step;
    if ((rc = rr_render_samples(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, nullptr, (uint32_t)spp, nullptr,
                                g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_samples");
    return RR_OK;
}

int drawFrameLens(int spp, float radius, float focus_distance)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (spp <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameLens: spp must be 1, 2, 4, 8 or 16");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    g_angle += g_opt.angle_step;
    const rr_lens lens = { radius, focus_distance };
    if ((rc = rr_render_lens(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, nullptr, nullptr, (uint32_t)spp, &lens,
                             nullptr, g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_lens");
    return RR_OK;
}

int drawFrameSpectral(int spp, int n_bands, float abbe)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (spp <= 0 || n_bands <= 0 || spp * (long long)n_bands > RR_MAX_SAMPLES)
        return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameSpectral: spp must be 1, 2, 4, 8 or 16 and spp * bands at most 64");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    float pos[2 * RR_MAX_SAMPLES], off[2 * RR_MAX_SAMPLES];
    rr_band one[RR_MAX_SAMPLES], bands[RR_MAX_SAMPLES];
    if ((rc = rr_host_sample_pattern((uint32_t)spp, pos)) != RR_OK) return fail(rc, "rr_host_sample_pattern");
    if ((rc = rr_host_spectral_bands((uint32_t)n_bands, g_opt.dispatch.ior, abbe, one)) != RR_OK) return fail(rc, "rr_host_spectral_bands");
    g_angle += g_opt.angle_step;
    for (int a = 0; a < spp; ++a)
        for (int b = 0; b < n_bands; ++b) {
            const int k = a * n_bands + b;
            off[2 * k] = pos[2 * a]; off[2 * k + 1] = pos[2 * a + 1];
            bands[k] = one[b];
        }
    if ((rc = rr_render_spectral(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, off, bands, (uint32_t)(spp * n_bands),
                                 nullptr, g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_spectral");
    return RR_OK;
}

int setMaterials(const rr_material* mats, int n)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (n <= 0 || !mats) return fail(RR_ERR_INVALID_ARGUMENT, "setMaterials: need at least one material");
    const int rc = rr_set_materials(g_ctx, mats, (uint32_t)n);
    if (rc != RR_OK) return fail(rc, "rr_set_materials");
    g_mats.assign(mats, mats + n);
    g_table.clear();
    return RR_OK;
}

int drawFrameMaterials(int spp)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (spp <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameMaterials: spp must be 1, 2, 4, 8 or 16");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    g_angle += g_opt.angle_step;
    if ((rc = rr_render_materials(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, nullptr, (uint32_t)spp, nullptr,
                                  g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_materials");
    return RR_OK;
}

int drawFrameNested(int spp)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (spp <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameNested: spp must be 1, 2, 4, 8 or 16");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    g_angle += g_opt.angle_step;
    if ((rc = rr_render_nested(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, nullptr, (uint32_t)spp, nullptr,
                               g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_nested");
    return RR_OK;
}

int setFloorAndLights(const float albedo[3], float specular, const rr_light* lights, int n_lights)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (g_mats.empty()) return fail(RR_ERR_STATE, "setFloorAndLights: setMaterials first");
    if (!albedo || n_lights < 0 || n_lights > RR_MAX_LIGHTS || (n_lights && !lights))
        return fail(RR_ERR_INVALID_ARGUMENT, "setFloorAndLights: need an albedo and at most 8 lights");
    // The floor needs no file: these are the 36 vertices Mesh::load gives for the shipped assets/cube.obj, in its order -- triangle
    // k / 3 of two passes over the faces -x, -z, +x, +z, -y, +y, flat normals whose zero components are negative zeros as the OBJ
    // writes them ("-0.0000").  The order and the zeros' signs only matter to a comparison bit for bit with a frame of cube.obj
    // under the same transform (tests/test_gpu_surfaces.py's rrdemo test): if the asset is ever re-exported, regenerate this table
    // from the loader's output or that test's floor differs in ties on shared edges and in the signs of zero direction components
    static const float P[36][3] = {
        { -1, 1, 1 }, { -1, -1, -1 }, { -1, -1, 1 }, { -1, 1, -1 }, { 1, -1, -1 }, { -1, -1, -1 }, { 1, 1, -1 }, { 1, -1, 1 }, { 1, -1, -1 },
        { 1, 1, 1 }, { -1, -1, 1 }, { 1, -1, 1 }, { 1, -1, -1 }, { -1, -1, 1 }, { -1, -1, -1 }, { -1, 1, -1 }, { 1, 1, 1 }, { 1, 1, -1 },
        { -1, 1, 1 }, { -1, 1, -1 }, { -1, -1, -1 }, { -1, 1, -1 }, { 1, 1, -1 }, { 1, -1, -1 }, { 1, 1, -1 }, { 1, 1, 1 }, { 1, -1, 1 },
        { 1, 1, 1 }, { -1, 1, 1 }, { -1, -1, 1 }, { 1, -1, -1 }, { 1, -1, 1 }, { -1, -1, 1 }, { -1, 1, -1 }, { -1, 1, 1 }, { 1, 1, 1 } };
    static const int axis[6] = { 0, 2, 0, 2, 1, 1 };
    static const float sign[6] = { -1, -1, 1, 1, -1, 1 };
    Mesh floor;
    for (int k = 0; k < 36; ++k) {
        Vertex v;
        std::memset(&v, 0, sizeof v);
        const int f = (k / 3) % 6;
        for (int c = 0; c < 3; ++c) { v.position[c] = P[k][c]; v.norm[c] = c == axis[f] ? sign[f] : -0.0f; }
        floor.verts.push_back(v);
        floor.indices.push_back((uint32_t)k);
    }
    int rc = floor.upload(g_ctx);
    if (rc != RR_OK) return fail(rc, "Mesh::upload (floor)");
    if ((rc = rr_build_blas(g_ctx, floor.mesh_id)) != RR_OK) return fail(rc, "rr_build_blas (floor)");
    float ymin = 3.0e38f;
    for (uint32_t i : cubeMesh.indices) ymin = cubeMesh.verts[i].position[1] < ymin ? cubeMesh.verts[i].position[1] : ymin;
    rr_instance_desc inst[2];
    std::memset(inst, 0, sizeof inst);
    inst[0].transform[0] = inst[0].transform[5] = inst[0].transform[10] = 1.0f;
    inst[0].instance_id_mask = 1u << 24;
    inst[0].blas = cubeMesh.raytracingGeometry().mesh_id;
    inst[1].transform[0] = 4.0f; inst[1].transform[5] = 0.1f; inst[1].transform[10] = 4.0f;
    inst[1].transform[7] = ymin - 0.15f;
    inst[1].instance_id_mask = 1u | (1u << 24);
    inst[1].hitgroup_flags = (uint32_t)g_mats.size();           // the row appended below
    inst[1].blas = floor.mesh_id;
    if ((rc = rr_build_tlas(g_ctx, inst, 2)) != RR_OK) return fail(rc, "rr_build_tlas");
    std::vector<rr_material> mats = g_mats;
    mats.push_back(rr_material{ 1.0f, { 0.0f, 0.0f, 0.0f } });  // never read: the row is opaque
    if ((rc = rr_set_materials(g_ctx, mats.data(), (uint32_t)mats.size())) != RR_OK) return fail(rc, "rr_set_materials");
    std::vector<rr_surface> surf(mats.size());
    std::memset(surf.data(), 0, surf.size() * sizeof(rr_surface));
    rr_surface& s = surf.back();
    s.kind = RR_SURFACE_OPAQUE;
    for (int c = 0; c < 3; ++c) { s.albedo[c] = albedo[c]; s.specular[c] = specular; }
    if ((rc = rr_set_surfaces(g_ctx, surf.data(), (uint32_t)surf.size())) != RR_OK) return fail(rc, "rr_set_surfaces");
    static const float ambient[3] = { 0.05f, 0.05f, 0.05f };
    if ((rc = rr_set_lights(g_ctx, lights, (uint32_t)n_lights, ambient)) != RR_OK) return fail(rc, "rr_set_lights");
    g_table = mats;
    g_floor_inst.assign(inst, inst + 2);
    g_lights.assign(lights, lights + n_lights);
    return RR_OK;
}

int setLightSoftness(float half_edge)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (!(half_edge >= 0.0f)) return fail(RR_ERR_INVALID_ARGUMENT, "setLightSoftness: need a half-edge >= 0");
    std::vector<rr_light_shape> shapes(g_lights.size());
    std::memset(shapes.data(), 0, shapes.size() * sizeof(rr_light_shape));
    for (size_t i = 0; i < g_lights.size(); ++i)
        if (g_lights[i].kind == RR_LIGHT_POINT) { shapes[i].ex[0] = half_edge; shapes[i].ey[2] = half_edge; }
    const int rc = rr_set_light_shapes(g_ctx, shapes.data(), (uint32_t)shapes.size());
    return rc != RR_OK ? fail(rc, "rr_set_light_shapes") : RR_OK;
}

int drawFrameSurfaces(int spp)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (spp <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameSurfaces: spp must be 1, 2, 4, 8 or 16");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    g_angle += g_opt.angle_step;
    if ((rc = rr_render_surfaces(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, nullptr, (uint32_t)spp, nullptr,
                                 g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_surfaces");
    return RR_OK;
}

// the band set of the composed and shutter frames: every row's index spread by Cauchy's law through its own value; the weights are
// the same for every row
static int setBandSet(int n_bands, float abbe)
{
    const std::vector<rr_material>& table = g_table.empty() ? g_mats : g_table;
    const int rows = (int)table.size();
    int rc;
    rr_band one[RR_MAX_SAMPLES];
    std::vector<float> iors((size_t)n_bands * rows), weights((size_t)n_bands * 3);
    for (int r = 0; r < rows; ++r) {
        if ((rc = rr_host_spectral_bands((uint32_t)n_bands, table[r].ior, abbe, one)) != RR_OK) return fail(rc, "rr_host_spectral_bands");
        for (int b = 0; b < n_bands; ++b) {
            iors[(size_t)b * rows + r] = one[b].ior;
            for (int ch = 0; ch < 3; ++ch) weights[(size_t)b * 3 + ch] = one[b].weight[ch];
        }
    }
    if ((rc = rr_set_material_bands(g_ctx, iors.data(), weights.data(), (uint32_t)n_bands)) != RR_OK) return fail(rc, "rr_set_material_bands");
    return RR_OK;
}

int drawFrameComposed(int spp, const rr_lens* lens, int n_bands, float abbe)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (g_mats.empty()) return fail(RR_ERR_STATE, "drawFrameComposed: setMaterials first");
    if (n_bands < 1) n_bands = 1;
    if (spp <= 0 || spp * (long long)n_bands > RR_MAX_SAMPLES)
        return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameComposed: spp must be 1, 2, 4, 8 or 16 and spp * bands at most 64");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    const int n = spp * n_bands, rows = (int)g_mats.size();
    float pos[2 * RR_MAX_SAMPLES], lpos[2 * RR_MAX_SAMPLES];
    if ((rc = rr_host_sample_pattern((uint32_t)spp, pos)) != RR_OK) return fail(rc, "rr_host_sample_pattern");
    if ((rc = rr_host_lens_pattern((uint32_t)n, lpos)) != RR_OK) return fail(rc, "rr_host_lens_pattern");
    if ((rc = setBandSet(n_bands, abbe)) != RR_OK) return rc;
    g_angle += g_opt.angle_step;
    rr_composed_sample samples[RR_MAX_SAMPLES];
    memset(samples, 0, sizeof samples);
    for (int a = 0; a < spp; ++a)
        for (int b = 0; b < n_bands; ++b) {                     // sample a * n_bands + b: position a in band b, lens point a * n_bands + b
            rr_composed_sample& k = samples[a * n_bands + b];
            k.offset[0] = pos[2 * a]; k.offset[1] = pos[2 * a + 1];
            k.lens_offset[0] = lpos[2 * (a * n_bands + b)]; k.lens_offset[1] = lpos[2 * (a * n_bands + b) + 1];
            k.band = (uint32_t)b;
        }
    if ((rc = rr_render_composed(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, samples, (uint32_t)n, lens, nullptr,
                                 g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_composed");
    printf("composed frame: %d positions x %d bands (Abbe number %g) of %d materials, %s, nested media\n", spp, n_bands, abbe, rows,
           lens && lens->radius > 0.0f ? "thin lens" : "pinhole");
    return RR_OK;
}

int drawFrameShutter(int spp, const rr_lens* lens, int n_bands, float abbe, int n_keys, float dt)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (g_mats.empty()) return fail(RR_ERR_STATE, "drawFrameShutter: setMaterials first");
    if (n_bands < 1) n_bands = 1;
    if (spp <= 0 || n_keys < 1 || n_keys > RR_MAX_SCENE_KEYS || spp * (long long)n_keys * n_bands > RR_MAX_SAMPLES)
        return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameShutter: spp must be 1, 2, 4, 8 or 16, keys 1 to 16 and spp * keys * bands at most 64");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    const int n = spp * n_keys * n_bands, rows = (int)g_mats.size();
    float pos[2 * RR_MAX_SAMPLES], lpos[2 * RR_MAX_SAMPLES];
    if ((rc = rr_host_sample_pattern((uint32_t)spp, pos)) != RR_OK) return fail(rc, "rr_host_sample_pattern");
    if ((rc = rr_host_lens_pattern((uint32_t)n, lpos)) != RR_OK) return fail(rc, "rr_host_lens_pattern");
    if ((rc = setBandSet(n_bands, abbe)) != RR_OK) return rc;
    // The camera is what moves in this demo, and a shutter frame has one camera: seen from the camera at angle a, the scene at
    // orbit angle a + d is the scene turned by -d about the y axis, so key j is the mesh under that turn (the environment map stays
    // where it is).  The top level is built once with ALLOW_UPDATE and updated per key.  Every key needs a top level -- a frame
    // cannot mix keys with and without one -- and the turn by 0 is the identity, which alone would be traced without: the instance
    // carries TRIANGLE_CULL_DISABLE, which keeps the top level and changes nothing else, the nested tree seeing both faces anyway
    const RaytracingGeometry geo = cubeMesh.raytracingGeometry();
    for (int j = 0; j < n_keys; ++j) {
        const float d = n_keys > 1 ? dt * (float)j / (float)(n_keys - 1) : 0.0f, c = std::cos(d), s = std::sin(d);
        rr_instance_desc inst;
        std::memset(&inst, 0, sizeof inst);
        inst.transform[0] = c; inst.transform[2] = s; inst.transform[5] = 1.0f; inst.transform[8] = -s; inst.transform[10] = c;
        inst.instance_id_mask = 1u << 24;
        inst.hitgroup_flags = RR_INSTANCE_FLAG_TRIANGLE_CULL_DISABLE << 24;
        inst.blas = geo.mesh_id;
        if ((rc = rr_build_tlas_ex(g_ctx, &inst, 1, g_shutter_tlas ? RR_BUILD_PERFORM_UPDATE : RR_BUILD_ALLOW_UPDATE)) != RR_OK) return fail(rc, "rr_build_tlas_ex");
        g_shutter_tlas = true;
        if ((rc = rr_capture_scene_key(g_ctx, (uint32_t)j)) != RR_OK) return fail(rc, "rr_capture_scene_key");
    }
    g_angle += g_opt.angle_step;
    rr_shutter_sample samples[RR_MAX_SAMPLES];
    memset(samples, 0, sizeof samples);
    for (int k = 0; k < n; ++k) {                               // sample (a * n_keys + j) * n_bands + b: position a, key j, band b, lens point k
        const int a = k / (n_keys * n_bands);
        samples[k].offset[0] = pos[2 * a]; samples[k].offset[1] = pos[2 * a + 1];
        samples[k].lens_offset[0] = lpos[2 * k]; samples[k].lens_offset[1] = lpos[2 * k + 1];
        samples[k].key = (uint32_t)(k / n_bands % n_keys);
        samples[k].band = (uint32_t)(k % n_bands);
    }
    if ((rc = rr_render_shutter(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, samples, (uint32_t)n, lens, nullptr,
                                g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_shutter");
    printf("shutter frame: %d positions x %d keys over %g rad x %d bands (Abbe number %g) of %d materials, %s, nested media\n", spp, n_keys, dt, n_bands,
           abbe, rows, lens && lens->radius > 0.0f ? "thin lens" : "pinhole");
    return RR_OK;
}

// the built-in light offsets: rr.light_pattern of the Python layer -- point k of n is (2 (k + 0.5) / n - 1, 2 (phi2(k) + 0.5 / m) - 1),
// phi2 the base-2 radical inverse, m the smallest power of two >= n, in double, rounded once
static void lightPattern(int n, float* out)
{
    int m = 1;
    while (m < n) m *= 2;
    for (int k = 0; k < n; ++k) {
        double phi = 0.0, f = 0.5;
        for (int i = k; i; i >>= 1) { phi += f * (double)(i & 1); f *= 0.5; }
        out[2 * k] = (float)(2.0 * (k + 0.5) / n - 1.0);
        out[2 * k + 1] = (float)(2.0 * (phi + 0.5 / m) - 1.0);
    }
}

int drawFrameLit(int spp, const rr_lens* lens, int n_bands, float abbe, int n_keys, float dt)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (g_mats.empty()) return fail(RR_ERR_STATE, "drawFrameLit: setMaterials first");
    if (n_bands < 1) n_bands = 1;
    const int keys = n_keys < 1 ? 1 : n_keys;
    if (spp <= 0 || keys > RR_MAX_SCENE_KEYS || spp * (long long)keys * n_bands > RR_MAX_SAMPLES)
        return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameLit: spp must be 1, 2, 4, 8 or 16, keys at most 16 and spp * keys * bands at most 64");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    const int n = spp * keys * n_bands;
    float pos[2 * RR_MAX_SAMPLES], lpos[2 * RR_MAX_SAMPLES], gpos[2 * RR_MAX_SAMPLES];
    if ((rc = rr_host_sample_pattern((uint32_t)spp, pos)) != RR_OK) return fail(rc, "rr_host_sample_pattern");
    if ((rc = rr_host_lens_pattern((uint32_t)n, lpos)) != RR_OK) return fail(rc, "rr_host_lens_pattern");
    lightPattern(spp, gpos);
    if ((rc = setBandSet(n_bands, abbe)) != RR_OK) return rc;
    if (n_keys < 1) {                                           // no shutter: the frame's scene as it stands is key 0
        if ((rc = rr_capture_scene_key(g_ctx, 0)) != RR_OK) return fail(rc, "rr_capture_scene_key");
    } else {
        // drawFrameShutter's keys with everything that stands in the scene turned: the mesh and, where there is one, the floor.  The
        // lights stay where they are, like the environment map
        std::vector<rr_instance_desc> base = g_floor_inst;
        if (base.empty()) {
            rr_instance_desc one;
            std::memset(&one, 0, sizeof one);
            one.transform[0] = one.transform[5] = one.transform[10] = 1.0f;
            one.instance_id_mask = 1u << 24;
            one.hitgroup_flags = RR_INSTANCE_FLAG_TRIANGLE_CULL_DISABLE << 24;
            one.blas = cubeMesh.raytracingGeometry().mesh_id;
            base.push_back(one);
        }
        for (int j = 0; j < n_keys; ++j) {
            const float d = n_keys > 1 ? dt * (float)j / (float)(n_keys - 1) : 0.0f, c = std::cos(d), s = std::sin(d);
            std::vector<rr_instance_desc> inst = base;
            for (size_t i = 0; i < inst.size(); ++i)
                for (int col = 0; col < 4; ++col) {             // rows 0 and 2 of R_y(d) * [A | t]
                    const float a0 = base[i].transform[col], a2 = base[i].transform[8 + col];
                    inst[i].transform[col] = c * a0 + s * a2;
                    inst[i].transform[8 + col] = c * a2 - s * a0;
                }
            if ((rc = rr_build_tlas(g_ctx, inst.data(), (uint32_t)inst.size())) != RR_OK) return fail(rc, "rr_build_tlas");
            if ((rc = rr_capture_scene_key(g_ctx, (uint32_t)j)) != RR_OK) return fail(rc, "rr_capture_scene_key");
        }
    }
    g_angle += g_opt.angle_step;
    rr_lit_sample samples[RR_MAX_SAMPLES];
    memset(samples, 0, sizeof samples);
    for (int k = 0; k < n; ++k) {                               // sample (a * keys + j) * n_bands + b: position a, key j, band b, lens point k, light point a
        const int a = k / (keys * n_bands);
        samples[k].offset[0] = pos[2 * a]; samples[k].offset[1] = pos[2 * a + 1];
        samples[k].lens_offset[0] = lpos[2 * k]; samples[k].lens_offset[1] = lpos[2 * k + 1];
        samples[k].light_offset[0] = gpos[2 * a]; samples[k].light_offset[1] = gpos[2 * a + 1];
        samples[k].key = (uint32_t)(k / n_bands % keys);
        samples[k].band = (uint32_t)(k % n_bands);
    }
    if ((rc = rr_render_lit(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, samples, (uint32_t)n, lens, nullptr,
                            g_back.data(), nullptr)) != RR_OK)
        return fail(rc, "rr_render_lit");
    printf("lit frame: %d positions x %d keys over %g rad x %d bands (Abbe number %g) of %d materials under %d lights, %s\n", spp, keys, n_keys < 1 ? 0.0f : dt,
           n_bands, abbe, (int)g_mats.size(), (int)g_lights.size(), lens && lens->radius > 0.0f ? "thin lens" : "pinhole");
    return RR_OK;
}

int drawFrameAdaptive(int base, int spp, float threshold, uint64_t* refined)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (base <= 0 || spp < base) return fail(RR_ERR_INVALID_ARGUMENT, "drawFrameAdaptive: need 1 <= base <= spp");
    rr_scene_constants sc;
    int rc = rr_host_camera_orbit(g_angle, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &sc);
    if (rc != RR_OK) return fail(rc, "rr_host_camera_orbit");
    g_angle += g_opt.angle_step;
    if ((rc = rr_render_adaptive(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &sc, &g_opt.dispatch, nullptr, (uint32_t)base, (uint32_t)spp,
                                 threshold, nullptr, g_back.data(), nullptr, nullptr, refined)) != RR_OK)
        return fail(rc, "rr_render_adaptive");
    return RR_OK;
}

// `for (;;) drawFrame();` (WinMain.cpp:49-59) without the per-frame fence wait and read-back: n_frames of the
// orbit, frames_per_dispatch depth slices per launch, in_flight launches overlapping.  The last frame lands in
// backBuffer().  The reference notes the missing overlap itself (RefractionDemo.cpp:519-521).
int pump(int n_frames, int frames_per_dispatch, int in_flight, rr_stats* stats)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (n_frames <= 0 || frames_per_dispatch <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "pump: frame counts must be positive");
    int rc = rr_set_frames_in_flight(g_ctx, (uint32_t)in_flight);
    if (rc != RR_OK) return fail(rc, "rr_set_frames_in_flight");
    rc = rr_render_orbit(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &g_opt.dispatch, &g_angle, g_opt.angle_step,
                         (uint32_t)n_frames, (uint32_t)frames_per_dispatch, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf);
    if (rc != RR_OK) return fail(rc, "rr_render_orbit");
    const uint32_t last = (uint32_t)((n_frames - 1) % frames_per_dispatch);
    if ((rc = rr_read_frame_slice(g_ctx, last, g_back.data(), nullptr)) != RR_OK) return fail(rc, "rr_read_frame_slice");
    if (stats && (rc = rr_get_stats(g_ctx, stats)) != RR_OK) return fail(rc, "rr_get_stats");
    return RR_OK;
}

// The frame loop with every frame delivered to host memory (frames[k*w*h*4 ...]), read-back overlapped with
// rendering (rr_render_orbit_to_host).  `frames` must hold n_frames frames; page-lock it for full PCIe speed.
int stream(int n_frames, int frames_per_dispatch, int in_flight, uint8_t* frames)
{
    if (!g_ctx) return fail(RR_ERR_STATE, "initialize first");
    if (n_frames <= 0 || frames_per_dispatch <= 0 || !frames) return fail(RR_ERR_INVALID_ARGUMENT, "stream: bad arguments");
    int rc = rr_set_frames_in_flight(g_ctx, (uint32_t)in_flight);
    if (rc != RR_OK) return fail(rc, "rr_set_frames_in_flight");
    rc = rr_render_orbit_to_host(g_ctx, (uint32_t)g_opt.width, (uint32_t)g_opt.height, &g_opt.dispatch, &g_angle, g_opt.angle_step,
                                 (uint32_t)n_frames, (uint32_t)frames_per_dispatch, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, frames);
    if (rc != RR_OK) return fail(rc, "rr_render_orbit_to_host");
    std::memcpy(g_back.data(), frames + (size_t)(n_frames - 1) * g_back.size(), g_back.size());
    return RR_OK;
}

int initializeSharded(const Options& opt, int rank, int world, const void* id128)
{
    int rc = initialize(opt);
    if (rc != RR_OK) return rc;
    if ((rc = rr_set_tile_partition(g_ctx, (uint32_t)rank, (uint32_t)world)) != RR_OK) return fail(rc, "rr_set_tile_partition");
    if ((rc = rr_comm_init(g_ctx, id128, rank, world, &g_comm)) != RR_OK) return fail(rc, "rr_comm_init");
    g_rank = rank; g_world = world;
    return RR_OK;
}

int pumpSharded(int n_frames, int frames_per_gather, rr_stats* stats)
{
    if (!g_ctx || !g_comm) return fail(RR_ERR_STATE, "initializeSharded first");
    if (n_frames <= 0 || frames_per_gather <= 0) return fail(RR_ERR_INVALID_ARGUMENT, "pumpSharded: frame counts must be positive");
    const uint32_t W = (uint32_t)g_opt.width, H = (uint32_t)g_opt.height;
    // The mesh-tile partition (rr_mesh_partition): only the tiles that touch the scene's screen rectangle are dealt to the ranks
    // and gathered; rank 0 renders the background tiles itself.  Buffers are sized for a batch whose rectangle is the whole
    // frame; a batch moves max_mesh_tiles_per_rank tiles per frame and rank.
    const uint32_t n_tiles = ((W + 31u) / 32u) * ((H + 31u) / 32u);
    const uint64_t tile_bytes = 32 * 32 * 3;                                      // RGB8
    const uint64_t rank_stride = (uint64_t)((n_tiles + (uint32_t)g_world - 1u) / (uint32_t)g_world) * tile_bytes * (uint64_t)frames_per_gather;
    const uint64_t bg_bytes = (uint64_t)n_tiles * tile_bytes * (uint64_t)frames_per_gather;
    const uint64_t raster = (uint64_t)W * H * 4;
    // Two buffer sets and two render lanes: batch b is rendered on lane b % 2 into set b % 2 while the gather of batch b - 1
    // (queued on the context's stream behind that lane's join) and its de-interleave run -- the gather travels under the next
    // render instead of after it.  Set b % 2 is free again when batch b + 2 starts: the context's stream, on which gather and
    // de-interleave of batch b were queued, is what lane b % 2 forks from.
    void *d_send[2] = { nullptr, nullptr }, *d_recv[2] = { nullptr, nullptr }, *d_bg[2] = { nullptr, nullptr }, *d_frames = nullptr;
    auto release = [&] { for (int k = 0; k < 2; ++k) { rr_device_free(g_ctx, d_send[k]); rr_device_free(g_ctx, d_recv[k]); rr_device_free(g_ctx, d_bg[k]); } rr_device_free(g_ctx, d_frames); };
    int rc = RR_OK;
    for (int k = 0; k < 2 && rc == RR_OK; ++k) {
        rc = rr_device_alloc(g_ctx, rank_stride, &d_send[k]);
        if (rc == RR_OK && g_rank == 0) rc = rr_device_alloc(g_ctx, rank_stride * (uint64_t)g_world, &d_recv[k]);
        if (rc == RR_OK && g_rank == 0) rc = rr_device_alloc(g_ctx, bg_bytes, &d_bg[k]);
    }
    if (rc == RR_OK && g_rank == 0) rc = rr_device_alloc(g_ctx, raster * (uint64_t)frames_per_gather, &d_frames);
    if (rc != RR_OK) { release(); return fail(rc, "rr_device_alloc"); }
    rr_dispatch_params p = g_opt.dispatch;
    int last_n = 0, pending_n = 0, pending_set = -1;
    rr_mesh_partition pending_part;
    std::memset(&pending_part, 0, sizeof pending_part);
    auto gather_pending = [&]() -> int {            // join the lane of the batch launched before, gather it, de-interleave on rank 0
        if (pending_set < 0) return RR_OK;
        const uint64_t frame_stride = (uint64_t)pending_part.max_mesh_tiles_per_rank * tile_bytes;
        int r = rr_lane_join(g_ctx, (uint32_t)pending_set);
        if (r != RR_OK) return fail(r, "rr_lane_join");
        r = rr_gather_frames(g_ctx, g_comm, g_rank, g_world, d_send[pending_set], d_recv[pending_set], frame_stride * (uint64_t)pending_n, 0);
        if (r != RR_OK) return fail(r, "rr_gather_frames");
        if (g_rank == 0) {
            r = rr_assemble_frames_mesh_rgb8(g_ctx, d_recv[pending_set], frame_stride * (uint64_t)pending_n, frame_stride, d_bg[pending_set],
                                             (uint64_t)pending_part.n_bg_tiles * tile_bytes, &pending_part, (uint32_t)pending_n, W, H, d_frames, raster);
            if (r != RR_OK) return fail(r, "rr_assemble_frames_mesh_rgb8");
        }
        last_n = pending_n; pending_set = -1;
        return RR_OK;
    };
    int b = 0;
    for (int k = 0; k < n_frames && rc == RR_OK; k += frames_per_gather, ++b) {
        const int n = n_frames - k < frames_per_gather ? n_frames - k : frames_per_gather;
        if (k > 0) p.flags |= RR_DISPATCH_KEEP_COUNTERS;
        rr_mesh_partition part;
        rc = rr_mesh_partition_for_orbit(g_ctx, W, H, g_angle, g_opt.angle_step, (uint32_t)n, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf, &part);
        if (rc != RR_OK) { fail(rc, "rr_mesh_partition_for_orbit"); break; }
        rc = rr_render_orbit_mesh_sharded_lane(g_ctx, W, H, &p, &g_angle, g_opt.angle_step, (uint32_t)n, g_opt.fov_y, g_opt.aspect, g_opt.zn, g_opt.zf,
                                               d_send[b & 1], (uint64_t)part.max_mesh_tiles_per_rank * tile_bytes, d_bg[b & 1],
                                               (uint64_t)part.n_bg_tiles * tile_bytes, (uint32_t)(b & 1));
        if (rc != RR_OK) { fail(rc, "rr_render_orbit_mesh_sharded_lane"); break; }
        if ((rc = gather_pending()) != RR_OK) break;
        pending_set = b & 1; pending_n = n; pending_part = part;
    }
    if (rc == RR_OK) rc = gather_pending();
    if (rc == RR_OK && g_rank == 0 && last_n > 0) {
        rc = rr_device_read(g_ctx, (const uint8_t*)d_frames + (uint64_t)(last_n - 1) * raster, g_back.data(), raster);
        if (rc != RR_OK) fail(rc, "rr_device_read");
    }
    if (rc == RR_OK) { rc = rr_wait(g_ctx); if (rc != RR_OK) fail(rc, "rr_wait"); }
    if (rc == RR_OK && stats && (rc = rr_get_stats(g_ctx, stats)) != RR_OK) fail(rc, "rr_get_stats");
    if (rc != RR_OK) (void)rr_wait(g_ctx);
    release();
    return rc;
}

const std::vector<uint8_t>& backBuffer() { return g_back; }
rr_context* context() { return g_ctx; }
float currentAngle() { return g_angle; }
const char* lastError() { return g_err.c_str(); }

void shutdown()
{
    if (g_comm) { rr_comm_destroy(g_comm); g_comm = nullptr; }
    if (g_ctx) {
        if (g_back_pinned) { rr_host_unregister(g_ctx, g_back.data()); g_back_pinned = false; }
        rr_destroy(g_ctx); g_ctx = nullptr;
    }
    g_mats.clear();
    g_table.clear();
    g_floor_inst.clear();
    g_lights.clear();
}

} // namespace RefractionDemo
