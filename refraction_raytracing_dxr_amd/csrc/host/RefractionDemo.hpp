// RefractionDemo.hpp -- headless mirror of the reference's host API (RefractionDemo.hpp:9-10):
//   void initialize(HWND, int width, int height)   ->  int initialize(const Options&)
//   void drawFrame()                               ->  int drawFrame()
// The window handle is gone (no swap chain); the literals of RefractionDemo.cpp become Options
// whose defaults are those literals.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "Mesh.hpp"

namespace RefractionDemo {

struct Options {
    int width = 1024, height = 768;                       // WinMain.cpp:44
    std::string mesh_path = "../shell.obj";               // RefractionDemo.cpp:537
    std::string env_path = "../envMap.hdr";               // RefractionDemo.cpp:527
    int device = 0;
    float fov_y = (float)(52.0f / 180.0 * 3.1415);        // RefractionDemo.cpp:559
    float aspect = (float)1.333;
    float zn = 1.0f, zf = 125.0f;
    float angle0 = 0.01f, angle_step = 0.01f;             // RefractionDemo.cpp:555,567
    rr_dispatch_params dispatch;                          // RayTracing.hlsl literals
    Options() { rr_default_dispatch_params(&dispatch); }
};

int initialize(const Options& opt);       // RefractionDemo.cpp:513-553; returns rr_status
int drawFrame();                          // RefractionDemo.cpp:557-612; returns rr_status
// drawFrame with spp primary rays per pixel (rr_render_samples, the built-in pattern of 1, 2, 4, 8 or 16 samples): the orbit
// advances as in drawFrame and the resolved frame lands in backBuffer()
int drawFrameSamples(int spp);
// drawFrameSamples through a thin lens (rr_render_lens, the built-in lens offsets): aperture radius and focus distance in world units
int drawFrameLens(int spp, float radius, float focus_distance);
// drawFrameSamples with dispersion (rr_render_spectral): the spp built-in positions crossed with the n_bands bands of
// rr_host_spectral_bands(n_bands, the dispatch's ior, abbe), sample a * n_bands + b being position a in band b; spp * n_bands <= 64
int drawFrameSpectral(int spp, int n_bands, float abbe);
// The material table of the scene (rr_set_materials).  Instance i is made of row i modulo n: the demo's one instance keeps hit-group
// index 0, which is row 0 of any table.  drawFrameMaterials is drawFrameSamples shaded with it (rr_render_materials): the glass's
// index of refraction and tint come from the table, the dispatch's ior is not used
int setMaterials(const rr_material* mats, int n);
int drawFrameMaterials(int spp);
// drawFrameMaterials with the nested-media ray tree (rr_render_nested): instances may sit inside, or overlap, other instances
int drawFrameNested(int spp);
// A lit table under the mesh (after setMaterials): an opaque floor -- cube.obj's twelve triangles scaled to (4, 0.1, 4), its top 0.05
// below the mesh's lowest vertex -- as a second instance made of a material row and an opaque surface row appended to the table
// (albedo, and specular in every channel), lit by n_lights lights and an ambient term of 0.05.  The scene gets a top level.
// drawFrameSurfaces is drawFrameNested shaded with them (rr_render_surfaces)
int setFloorAndLights(const float albedo[3], float specular, const rr_light* lights, int n_lights);
int drawFrameSurfaces(int spp);
// drawFrameNested composed with a lens and dispersion per material (rr_render_composed): the spp built-in positions crossed with
// n_bands bands, sample a * n_bands + b being position a in band b, each sample with the lens point of rr_host_lens_pattern(spp *
// n_bands); lens may be null (a pinhole).  The band set (rr_set_material_bands) gives every row of the table of setMaterials the
// indices of rr_host_spectral_bands(n_bands, its own ior, abbe) and every band that table's weights; n_bands <= 1: no dispersion.
// Prints one line that names the composition
int drawFrameComposed(int spp, const rr_lens* lens, int n_bands, float abbe);
// drawFrameComposed with a shutter (rr_render_shutter): the scene at n_keys orbit angles, the frame's own and up to dt beyond it
// (angle + j * dt / (n_keys - 1)), each captured as a scene key, and the spp positions crossed with the keys and the bands -- sample
// (a * n_keys + j) * n_bands + b being position a in key j and band b; spp * n_keys * n_bands <= 64.  The camera is what orbits here,
// so key j holds the mesh turned by the opposite angle about y under the frame's one camera; the environment map does not turn with
// it.  From the first call on the scene has a top level (one instance, updated per key).  Prints one line that names the frame
int drawFrameShutter(int spp, const rr_lens* lens, int n_bands, float abbe, int n_keys, float dt);
// drawFrameShutter over the opaque hit groups (rr_render_lit): the floor and lights of setFloorAndLights, if any, through the lens;
// n_keys < 1: no shutter, the frame's scene is captured as key 0.  With keys the mesh and the floor turn together, the lights stay.
// Position a of the spp takes point a of the built-in light pattern; setLightSoftness(S) makes every point light a square of
// half-edge S in the xz-plane (rr_set_light_shapes), 0 a point again
int setLightSoftness(float half_edge);
int drawFrameLit(int spp, const rr_lens* lens, int n_bands, float abbe, int n_keys, float dt);
// drawFrameSamples with base samples for every pixel and the rest of the spp only where the base samples show contrast above
// threshold (rr_render_adaptive); refined (may be null) receives the number of pixels that took all spp samples
int drawFrameAdaptive(int base, int spp, float threshold, uint64_t* refined);
// the frame loop as one call: no per-frame wait or read-back, `in_flight` launches overlapping (1..4)
int pump(int n_frames, int frames_per_dispatch, int in_flight, rr_stats* stats);
// the frame loop with every frame copied to host memory while the next ones render; frames: n_frames*w*h*4 bytes
int stream(int n_frames, int frames_per_dispatch, int in_flight, uint8_t* frames);
// Several GPUs, one process each (rank of world): frames shard by 32x32 tile, tile t to rank t % world; every rank renders
// its tiles of a batch of frames, ONE grouped RCCL gather brings them to rank 0, which de-interleaves them into whole frames.
// id128: the 128 bytes rank 0 got from rr_comm_unique_id, handed to every process.  The reference has a single adapter
// (RefractionDemo.cpp:163); this is the tile-parallel form of its frame loop.
int initializeSharded(const Options& opt, int rank, int world, const void* id128);
// n_frames of the orbit in batches of frames_per_gather; on rank 0 the last frame lands in backBuffer()
int pumpSharded(int n_frames, int frames_per_gather, rr_stats* stats);
// the frame drawFrame just produced (RGBA8, width*height*4), i.e. what Present would have shown
const std::vector<uint8_t>& backBuffer();
rr_context* context();
float currentAngle();
const char* lastError();
void shutdown();

} // namespace RefractionDemo
