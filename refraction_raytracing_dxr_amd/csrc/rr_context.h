// rr_context.h -- what the rr_capi*.cpp sources share: the owners of device memory, events and streams, struct rr_context,
// error reporting, and the few helpers that cross files.  Private: not installed, not part of include/rrdxr.h.
#pragma once
#include "../../include/rrdxr.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rr_choice.h"
#include "rr_launch.h"

namespace rr {

// Optional roctx ranges around the coarse steps (build, dispatch, assemble) so that `rocprofv3 --marker-trace`
// shows them next to the kernels.  The marker library is looked up at run time; without it the calls are no-ops.
struct Range {
    explicit Range(const char* name);
    ~Range();
};
// What the context allocates is held by these owners: each releases what it holds when it goes (errors ignored), so that an
// early return frees its temporaries and rr_destroy only has to wait for the streams.

// n units of `unit` bytes (by default: n elements of T) in device memory, or in page-locked host memory; size() is 0 while
// nothing is held
template <class T, bool Pinned = false> class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); }
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(n_, o.n_); } return *this; }
    ~Buf() { reset(); }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    void reset() { if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; n_ = 0; }
    hipError_t alloc(size_t n, size_t unit = sizeof(T))      // (what was held is released first)
    {
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n * unit, hipHostMallocDefault) : hipMalloc(&p, n * unit);
        if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = n; }
        return e;
    }
    int grow(rr_context* ctx, size_t n);
private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DevBuf = Buf<T>;
template <class T> using HostBuf = Buf<T, true>;

// an event or a stream, created with explicit flags
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)> class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept { std::swap(h_, o.h_); }     // (std::vector<Event>)
    ~Handle() { reset(); }
    H get() const { return h_; }
    void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
    hipError_t create(unsigned flags)
    {
        reset();
        const hipError_t e = Create(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
private:
    H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

struct MeshRes {
    DevBuf<float>    d_verts;        // n_verts * 8 floats
    DevBuf<uint32_t> d_idx;
    uint32_t  n_verts = 0, n_idx = 0, n_tris = 0;
    uint32_t  n_nodes() const { return n_tris > 1 ? n_tris - 1 : 1; }      // nodes of the BLAS
    DevBuf<BvhNode> nodes;           // fp32 hierarchy (builder output, rr_download_blas)
    DevBuf<QNode>   qnodes;          // what traversal reads: the same nodes with fp16 planes on the grid of the bounds
    QGrid     grid = { { 0, 0, 0 }, { 1, 1, 1 } };
    DevBuf<TriRec> tris;
    DevBuf<NrmRec> nrms;
    bool      built = false;
    float     bounds[6] = { 0, 0, 0, 0, 0, 0 };
    float     scale = 1.0f;          // max |bounds|
    uint32_t  depth = 0;
    // update builds (RR_BUILD_ALLOW_UPDATE / PERFORM_UPDATE)
    DevBuf<int32_t>  links;          // ALLOW_UPDATE builds: (parent << 1 | child slot) of every node (launch_keep_links)
    DevBuf<uint32_t> visit;          // ALLOW_UPDATE builds: n_tris-1 arrival counters of the refit
    DevBuf<uint32_t> d_upd;          // 8 words: refit bounds (ordered uints) [0,6), device vertex check [6] scratch, [7] sticky reject
    bool      allow_update = false;
    bool      stale = false;         // vertices replaced since the last build: the BLAS must be rebuilt or updated before a TLAS build
    bool      dev_pending = false;   // a device vertex update whose verdict (d_upd[7]) the next build reads
    uint64_t  version = 0;           // bumped by every successful build or update of the BLAS
};

// device block zeroed before every dispatch: counters, ray shards, error flag
struct CounterBlock {
    unsigned long long counters[16];
    static_assert(C_COUNT <= 16, "CounterBlock::counters holds every rr::Counter");
    uint32_t shards[RAY_SHARDS];
    uint32_t error;
    uint32_t pad[3];
};

// the k_stream_* buffers of one stream slot; render_stream gives the kernels a StreamDev of them
struct StreamSet {
    DevBuf<float4>   q[2];           // entries of 3 x float4 (q[1] is allocated last: its size is the set's queue capacity)
    DevBuf<uint32_t> fill[2];
    DevBuf<uint32_t> heads;          // head counters and, behind them, the chunk ticket counters
    DevBuf<float4>   slots;          // units of 4 x float4 per pixel
    DevBuf<uint8_t>  pending;        // one per pixel (allocated after slots: its size is the set's pixel count)
};

// One captured scene (rr_capture_scene_key): copies of everything fill_scene points a SceneDev at, in buffers the key owns, and
// what the host needs of the scene when a shutter frame uses the key.  Buffers are kept when the key is captured again and only
// grow; the record the kernel reads is slot `key` of rr_context::d_key_scenes
struct SceneKey {
    bool captured = false;
    DevBuf<InstDev> insts;
    DevBuf<QNode>   pool_qnodes, qnodes0;        // (qnodes0, tris0, nrms0: the mesh's own, for a scene without a top level)
    DevBuf<TriRec>  pool_tris, tris0;
    DevBuf<NrmRec>  pool_nrms, nrms0;
    SceneFacts facts = { false, 0, 0, 0, 0, false };     // scene_facts at the capture
    float    bounds[6] = { 0, 0, 0, 0, 0, 0 };           // scene_bounds
    uint32_t n_insts = 0, n_tris = 0, max_material = 0, mat0 = 0;
    uint64_t bytes() const
    {
        return insts.size() * sizeof(InstDev) + (pool_qnodes.size() + qnodes0.size()) * sizeof(QNode) +
               (pool_tris.size() + tris0.size()) * sizeof(TriRec) + (pool_nrms.size() + nrms0.size()) * sizeof(NrmRec);
    }
    void release() { *this = SceneKey(); }
};

} // namespace rr

using namespace rr;          // (every source that includes this is written in terms of rr's types, as rr_context is)

struct rr_context {
    int device = 0;
    int n_cus = 256;
    Stream      own_stream;          // (declared first: released last)
    hipStream_t stream = nullptr;
    std::string err;

    std::vector<MeshRes> meshes;

    DevBuf<float4> d_env;
    int env_w = 0, env_h = 0;

    // TLAS
    std::vector<rr_instance_desc> inst_host;
    DevBuf<InstDev> d_insts;
    DevBuf<BvhNode> d_pool_nodes;      // fp32 TLAS nodes (builder output)
    DevBuf<QNode>   d_pool_qnodes;     // flattened scene as traversal reads it: TLAS nodes, then every BLAS in use
    QGrid    scene_grid = { { 0, 0, 0 }, { 1, 1, 1 } };
    DevBuf<TriRec>  d_pool_tris;
    DevBuf<NrmRec>  d_pool_nrms;
    uint32_t n_pool_tris = 0, n_pool_nodes = 0;     // (n_pool_nodes: TLAS nodes, then those of every BLAS in use)
    uint32_t n_insts = 0, tlas_depth = 0;
    bool tlas_built = false;
    bool single_identity = false;
    float scene_scale = 1.0f;
    float scene_bounds[6] = { 0, 0, 0, 0, 0, 0 };   // world-space box of the whole scene (the TLAS root)
    // where each mesh sits in the pools (0xffffffff: not in the scene) and the BLAS version pooled there (TLAS updates re-pool
    // only what changed); TLAS ALLOW_UPDATE builds also keep the links and counters of the top level
    std::vector<uint32_t> pool_node_off, pool_tri_off;
    std::vector<uint64_t> pool_version;
    DevBuf<int32_t>  d_tlas_links;
    DevBuf<uint32_t> d_tlas_visit;
    bool tlas_refittable = false;

    DevBuf<float> d_screen;          // GenerateCameraRay's screen coordinates for frames of screen_w x screen_h: sx[W], sy[H]
    uint32_t screen_w = 0, screen_h = 0;     // (0: the tables are not valid)

    rr_scene_constants cam;
    bool cam_set = false;
    DevBuf<CamDev> d_cams;           // device-side constant buffer(s), one per depth slice
    // page-locked staging for the constants (a copy from pageable memory makes the runtime stage it itself, a few hundred
    // microseconds in front of every launch): four slots in turn, each guarded by an event recorded behind its copy
    static constexpr int CAM_SLOTS = 4;
    HostBuf<CamDev> h_cams[CAM_SLOTS];
    Event      h_cams_ev[CAM_SLOTS];
    bool       h_cams_busy[CAM_SLOTS] = {};
    uint32_t   h_cams_next = 0;

    uint32_t tile_rank = 0, tile_world = 1;

    // lanes: internal streams whose launches may overlap each other (rr_render_orbit_sharded_lane)
    static constexpr uint32_t MAX_LANES = 4;
    Stream      lane_stream[MAX_LANES];
    Event       lane_fork[MAX_LANES], lane_done[MAX_LANES];
    DevBuf<CamDev> lane_cams[MAX_LANES];
    bool        lane_busy[MAX_LANES] = {};
    uint32_t    frames_in_flight = 2;    // rr_set_frames_in_flight: launches of rr_render_orbit that may overlap
    size_t      frame_base = 0;          // element offset of the most recent dispatch inside d_rgba8 / d_f32

    // frame
    uint32_t W = 0, H = 0, frame_world = 0, frame_depth = 1;
    DevBuf<uint32_t> d_rgba8;        // world==1: W*H; else local tiles
    DevBuf<float4>   d_f32;
    DevBuf<uint32_t> d_assembled;    // rank-0 raster after rr_assemble_tiles
    bool      have_f32 = false, have_frame = false, have_assembled = false;
    uint64_t  last_pixels = 0;
    uint64_t  accum_pixels = 0;      // pixels of all dispatches since the counters were last zeroed
    bool      last_stats = false;

    DevBuf<CounterBlock> d_cnt;
    DevBuf<CounterBlock> d_cnt_trial;        // what the two renders of a kernel-choice measurement count into (thrown away)
    DevBuf<uint32_t> d_park[MAX_LANES + 1]; // k_render_lds: parked reflected rays, one slab per stream slot like the tickets
    char       last_kernel_name[96] = "";
    uint32_t   last_kernel = 0;      // render kernel of the last dispatch (rr_choice.h RenderKernel): 0 fused, 1 lds, 2 paths, 7 stream
    DevBuf<uint32_t> d_tickets;      // k_render_lds ticket words: one block per stream a launch can be on (lanes, then the context's stream)

    // diagnostics switches, read once at rr_create (never needed for correct results)
    DebugFacts dbg = { 0, 0, false };    // RR_DEBUG_KERNEL / _STACK / _TLAS32 (rr_choice.h): a forced kernel, wherever it can render the launch
    int  dbg_ticket_blocks = 0;      // RR_DEBUG_TICKET: 1 = k_render_lds treats the whole frame as the mesh rectangle, 2 = no rectangle
    bool dbg_group_trace = true;     // RR_DEBUG_GROUP_TRACE=0: k_render_paths never shares a ray between lanes
    bool dbg_async_set = false;
    uint32_t dbg_async[2] = { 2, 2 };    // RR_DEBUG_ASYNC="step,shade": issue thresholds of k_stream_rays in sixteenths of the live lanes
    bool dbg_tile_order = true;      // RR_DEBUG_TILE_ORDER=0: tiles in image order (DispatchDev::rt_*)
    int  dbg_shape = 0;              // RR_DEBUG_SHAPE: first k_render_lds workgroup shape to consider (rr_launch.h)
    int  dbg_refine_groups = 0;      // RR_DEBUG_REFINE_GROUPS: workgroups of k_adaptive_refine, which then loops over the list (0: the worst-case grid)
    std::string dbg_diag;            // RR_DEBUG_DIAG: file that receives per-wave diagnostics of Depth-1 dispatches

    // timing
    Event ev_begin, ev_end;
    std::vector<Event> kev;          // pairs
    uint32_t kev_used = 0;

    // k_stream_* (rr_render_stream.hip): ray queues, leaf slots and pixel marks of one pass; grown on demand, never shrunk.
    // One set per stream a launch can be on (the lanes, then the context's stream: launches on one stream are ordered, launches
    // on different lanes overlap), allocated when that stream first renders with the stream renderer.
    StreamSet strm[MAX_LANES + 1];
    size_t    strm_budget = 0;                       // bytes one set may take (stream_budget)
    ChoiceClass ch[3];                   // the measured kernel choices (rr_choice.h), by ChoiceClassId
    Event      ch_ev[4];

    // trace_rays scratch
    DevBuf<rr_ray_dev> d_rays;
    DevBuf<rr_hit_dev> d_hits;
    DevBuf<uint32_t>   d_counts;     // rr_query_rays_multi
    // the outputs of the host variants of rr_shade_rays, rr_render_samples and rr_render_adaptive (the frame buffers belong to the
    // dispatches).  One set for the three: each runs on the context's stream and synchronises before it returns, and grow waits
    // for that stream, so at most one call uses the set at any time
    DevBuf<float4>     d_out_f32;
    DevBuf<uint32_t>   d_out_rgba8, d_out_n;
    // rr_render_adaptive's own: its sample counts and its workspace, in units of 16 bytes
    DevBuf<uint32_t>   d_adaptive_taken;
    DevBuf<float4>     d_adaptive_ws;
    // the material table (rr_set_materials): n_mats rows at the head of d_mats, 0 = none set; max_material: the largest
    // hit-group index (hitgroup_flags & 0xffffff) among the instances of the current TLAS
    DevBuf<MatDev>     d_mats;
    uint32_t n_mats = 0, max_material = 0;
    // the surface table (rr_set_surfaces): n_surfs rows at the head of d_surfs, 0 = none set (every row is glass); and the lights
    // with the ambient term (rr_set_lights), which the surface kernels take by value.  Only the rr_*_surfaces calls and
    // rr_render_lit read them.  light_shapes: the shape table (rr_set_light_shapes), row i with light i, on == 0 while none is set;
    // rr_set_lights clears it, and only rr_render_lit reads it
    DevBuf<SurfDev>    d_surfs;
    uint32_t n_surfs = 0;
    LightsDev lights = {};
    LightShapesDev light_shapes = {};
    // transparent shadows (rr_set_shadow_steps): the cap on a shadow walk's TraceRay calls, 0 = off (any accepted hit occludes, the
    // first-hit kernels of rr_render_surfaces.hip and rr_render_lit.hip).  Read where the surface table is read; no other setter touches it
    uint32_t shadow_steps = 0;
    // the band set of rr_render_composed (rr_set_material_bands): n_bands copies of the table in force, each with a column of
    // indices of its own, one behind the other at the head of d_band_mats, and three weights per band at the head of d_band_w;
    // n_bands == 0: none set, the one band is d_mats itself with the weights of d_band_one (1, 1, 1; made with the first table).
    // mats_host: the rows of d_mats, which a band set is made from
    std::vector<MatDev> mats_host;
    DevBuf<MatDev>     d_band_mats;
    DevBuf<float>      d_band_w, d_band_one;
    uint32_t n_bands = 0;
    // the scene keys of rr_render_shutter (rr_capture_scene_key) and their records as the kernel reads them: RR_MAX_SCENE_KEYS
    // slots, allocated and zeroed at the first capture, slot k written when key k is captured.  key_host: the host copy a slot is
    // written from (it outlives the copy)
    SceneKey keys[RR_MAX_SCENE_KEYS];
    DevBuf<KeyDev> d_key_scenes;
    KeyDev key_host[RR_MAX_SCENE_KEYS] = {};
};

namespace rr {

int fail(rr_context* ctx, int code, const char* what, hipError_t e = hipSuccess);

#define RR_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) return fail(ctx, e_ == hipErrorOutOfMemory ? RR_ERR_OUT_OF_MEMORY : RR_ERR_DEVICE, #call, e_); \
    } while (0)

// as RR_HIP, but any failure is RR_ERR_DEVICE and reported as `what`
#define RR_HIP_MSG(call, what)                                                            \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) return fail(ctx, RR_ERR_DEVICE, what, e_);                  \
    } while (0)

// reallocates to n elements (size() 0 if that fails).  Waits for the context's stream first: what is in flight there may still
// read the old buffer.
template <class T, bool Pinned> int Buf<T, Pinned>::grow(rr_context* ctx, size_t n)
{
    RR_HIP(hipStreamSynchronize(ctx->stream));
    RR_HIP(alloc(n));
    return RR_OK;
}

// ---- rr_capi.cpp
int use_device(rr_context* ctx);
void fill_scene(const rr_context* ctx, SceneDev& sc);
uint32_t inst0_mask(const rr_context* ctx);
uint32_t scene_stack_need(const rr_context* ctx);
rr_dispatch_params params_or_default(const rr_dispatch_params* params);
// round-robin tiles of a W x H frame: tiles across, tiles, this rank's, the most any rank has
struct Tiles { uint32_t tiles_x, n_tiles, local, max_local; };
Tiles tile_counts(uint32_t W, uint32_t H, uint32_t rank, uint32_t world);
int join_lane(rr_context* ctx, uint32_t lane);
int join_lanes(rr_context* ctx);

// ---- rr_capi_dispatch.cpp
// mesh-tile partition: the partition the caller's tile buffers were checked against, where rank 0's background tiles go
struct MeshOut { const rr_mesh_partition* part; uint32_t* bg; size_t bg_stride_elems; };

// One dispatch.  h_cams: host copy of the depth slices' constants (may be null: no ordering hint); ext_tiles != null: compact tile
// output into caller memory with the given stride (sharded frames); out_slot: which of the frames_in_flight output regions (of
// out_slot_depth slices each) of the internal frame buffer this dispatch writes
struct DispatchRequest {
    uint32_t width = 0, height = 0, depth = 1;
    const CamDev* d_cams = nullptr; const rr_scene_constants* h_cams = nullptr;
    rr_dispatch_params params = {};
    uint32_t* ext_tiles = nullptr; size_t ext_stride_elems = 0;
    bool keep_counters = false;
    uint32_t out_slot = 0, out_slot_depth = 0;
    const MeshOut* mesh = nullptr;
};
int dispatch_impl(rr_context* ctx, const DispatchRequest& req);
int upload_cams(rr_context* ctx, const rr_scene_constants* c, size_t n);
int ensure_frame_buffers(rr_context* ctx, size_t elems, bool want_f32);
// the bounce limits and the IOR of a dispatch ("dispatch") or a radiance query ("shade_rays")
int check_shading_params(rr_context* ctx, const char* who, const rr_dispatch_params& p);
// waits for the context's stream, then reads the device error flag of what it rendered
int check_error_flag(rr_context* ctx, const char* what);
// what the kernel choice (rr_choice.h) knows of the scene
SceneFacts scene_facts(const rr_context* ctx);
// what the kernel choice knows of the request's launch, whose scene rectangle (pixels) is `rect`, and the kernel it picks before
// any measurement
struct LaunchPick { SceneFacts sf; LaunchFacts lf; KernelPick pk; };
LaunchPick pick_launch(const rr_context* ctx, const DispatchRequest& req, const uint32_t rect[4], bool compact);

} // namespace rr
