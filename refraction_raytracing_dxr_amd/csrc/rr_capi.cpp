// rr_capi.cpp -- the C ABI of include/rrdxr.h over HIP streams.
//
// Stands where RefractionDemo.cpp's D3D12 plumbing stood: createDevice (:142-172), Mesh::upload
// (Mesh.cpp:55-94), load_texture (:108-140), the two BuildRaytracingAccelerationStructure calls
// (:277-356), the per-frame constant-buffer copy (:566), DispatchRays (:580-594), the UAV ->
// backbuffer copy (:596-604) and the fence wait (:65-71).  Everything device-side is a kernel in
// rr_bvh_build.hip / rr_render.hip; this file only owns memory, call order and error reporting.
#include "../../include/rrdxr.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rr_choice.h"
#include "rr_launch.h"

using namespace rr;

static_assert(CHOICE_TILE == (uint32_t)TILE && CHOICE_STREAM_MAX_GEN == STREAM_MAX_GEN, "rr_choice.h mirrors rr_types.h");

static_assert(sizeof(rr_vertex) == 32, "Vertex stride (Mesh.cpp:45)");
static_assert(sizeof(rr_instance_desc) == 64, "D3D12_RAYTRACING_INSTANCE_DESC");
static_assert(sizeof(rr_scene_constants) == 80, "SceneConstants");
static_assert(sizeof(rr_ray) == sizeof(rr_ray_dev) && sizeof(rr_hit) == sizeof(rr_hit_dev), "ray/hit ABI");
static_assert(offsetof(rr_ray, instance_mask) == 36 && offsetof(rr_ray_dev, instance_mask) == 36, "rr_ray.instance_mask");

// Optional roctx ranges around the coarse steps (build, dispatch, assemble) so that `rocprofv3 --marker-trace`
// shows them next to the kernels.  The marker library is looked up at run time; without it the calls are no-ops.
#include <dlfcn.h>
// RCCL is looked up with dlopen (nothing links against it, and building needs no RCCL header): the two things of its ABI that
// cross this file are declared here -- the 128-byte unique id, passed by value to ncclCommInitRank, and ncclUint8 of ncclDataType_t
struct rr_nccl_unique_id { char internal[128]; };
enum { RR_NCCL_UINT8 = 1 };
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        for (const char* lib : { "librocprofiler-sdk-roctx.so", "libroctx64.so" }) {
            if (void* h = dlopen(lib, RTLD_LAZY | RTLD_LOCAL)) {
                push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
const Roctx& roctx() { static const Roctx r; return r; }
struct Range {
    explicit Range(const char* name) { if (roctx().push) roctx().push(name); }
    ~Range() { if (roctx().pop) roctx().pop(); }
};
} // namespace

namespace {

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

} // namespace

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
    // rr_shade_rays scratch (the host variant's outputs; the frame buffers belong to the dispatches)
    DevBuf<float4>     d_shade_f32;
    DevBuf<uint32_t>   d_shade_rgba8, d_shade_n;
};

namespace {

int fail(rr_context* ctx, int code, const char* what, hipError_t e = hipSuccess)
{
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}

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

uint32_t next_pow2(uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

// world -> object inverse of a 3x4 affine (adjugate / det, fixed operation order; mirrored by the oracle)
void affine_inverse(const float t[12], float inv[12])
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

float ord2f_host(uint32_t u)
{
    uint32_t v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

struct BuildScratch {
    BuildBuffers b{};
    DevBuf<char> raw;
};

// one allocation carved into the builder's scratch arrays (16-byte aligned pieces)
int alloc_build(rr_context* ctx, uint32_t n, BuildScratch& s)
{
    const uint32_t n_pad = next_pow2(n);
    auto al = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
    size_t o_box = 0;
    size_t o_keys = o_box + al((size_t)n * 6 * 4);
    size_t o_parent = o_keys + al((size_t)n_pad * 8);
    size_t o_child = o_parent + al((size_t)(2 * (size_t)n) * 4);
    size_t o_nbox = o_child + al((size_t)(2 * (size_t)n) * 4);
    size_t o_visit = o_nbox + al((size_t)(2 * (size_t)n) * 6 * 4);
    size_t o_scene = o_visit + al((size_t)n * 4);
    size_t o_depth = o_scene + al(6 * 4);
    size_t o_ploc = o_depth + al(4);
    size_t total = o_ploc + al((size_t)n * 8);
    RR_HIP(s.raw.alloc(total));
    char* base = s.raw.get();
    s.b.n = n; s.b.n_pad = n_pad;
    s.b.prim_box = (float*)(base + o_box);
    s.b.keys = (unsigned long long*)(base + o_keys);
    s.b.parent = (int32_t*)(base + o_parent);
    s.b.child = (int32_t*)(base + o_child);
    s.b.node_box = (float*)(base + o_nbox);
    s.b.visit = (uint32_t*)(base + o_visit);
    s.b.scene_box = (uint32_t*)(base + o_scene);
    s.b.depth = (uint32_t*)(base + o_depth);
    s.b.ploc = (uint32_t*)(base + o_ploc);
    return RR_OK;
}

int use_device(rr_context* ctx)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, RR_ERR_DEVICE, "hipSetDevice", e);
    return RR_OK;
}

// grid over a box {lo[3], hi[3]}: 65530 cells span the extent, counted from the centre (planes are stored as fp16
// cell counts, |q| <= 32768); a flat axis gets a tiny positive cell
QGrid make_grid(const float b[6])
{
    QGrid g;
    for (int k = 0; k < 3; ++k) {
        const float ext = b[3 + k] - b[k];
        const float mag = std::max(std::max(std::fabs(b[k]), std::fabs(b[3 + k])), 1e-30f);
        g.cell[k] = std::max(ext, mag * 1e-6f) / 65530.0f;
        g.org[k] = b[k] + 32765.0f * g.cell[k];      // fp16 planes are signed: the grid origin is the centre of the box
    }
    return g;
}

void fill_scene(const rr_context* ctx, SceneDev& sc)
{
    memset(&sc, 0, sizeof sc);
    const MeshRes* m0 = nullptr;
    if (ctx->single_identity) m0 = &ctx->meshes[(size_t)ctx->inst_host[0].blas];
    if (m0) {
        sc.blas0.nodes = m0->qnodes.get(); sc.blas0.grid = m0->grid; sc.blas0.tris = m0->tris.get(); sc.blas0.nrms = m0->nrms.get();
        sc.blas0.n_tris = m0->n_tris; sc.blas0.depth = m0->depth; sc.blas0.scale = m0->scale;
    }
    sc.pool_nodes = ctx->d_pool_qnodes.get(); sc.grid = ctx->scene_grid; sc.pool_tris = ctx->d_pool_tris.get(); sc.pool_nrms = ctx->d_pool_nrms.get();
    sc.insts = ctx->d_insts.get();
    sc.n_insts = ctx->n_insts;
    sc.n_pool_tris = ctx->n_pool_tris;
    sc.single_identity = ctx->single_identity ? 1u : 0u;
    sc.scale = ctx->scene_scale;
    sc.env = ctx->d_env.get();
    sc.env_w = ctx->env_w; sc.env_h = ctx->env_h;
}

// trace_rays scratch for n rays
int ensure_rays(rr_context* ctx, size_t n)
{
    if (n > ctx->d_hits.size()) if (int r = ctx->d_hits.grow(ctx, n)) return r;
    return n > ctx->d_rays.size() ? ctx->d_rays.grow(ctx, n) : RR_OK;
}

// InstanceMask of a single-identity scene's instance (the query kernels test it per ray before the walk)
uint32_t inst0_mask(const rr_context* ctx)
{
    return ctx->single_identity ? (ctx->inst_host[0].instance_id_mask >> 24) & 0xffu : 0xffu;
}

// deepest traversal stack the scene can need (near child followed, far child pushed)
uint32_t scene_stack_need(const rr_context* ctx)
{
    uint32_t blas_max = 0;
    for (uint32_t i = 0; i < ctx->n_insts; ++i) {
        const MeshRes& m = ctx->meshes[(size_t)ctx->inst_host[i].blas];
        if (m.depth > blas_max) blas_max = m.depth;
    }
    return ctx->single_identity ? blas_max : blas_max + ctx->tlas_depth;
}

} // namespace

extern "C" {

uint32_t rr_abi_version(void) { return RRDXR_ABI_VERSION; }

void rr_default_dispatch_params(rr_dispatch_params* p)
{
    if (!p) return;
    p->max_refract = 5;
    p->max_reflect = 2;
    p->ior = 1.3f;
    p->tmin_primary = 0.0001f;
    p->tmax_primary = 100.0f;
    p->tmin_secondary = 0.001f;
    p->tmax_secondary = 1000.0f;
    p->flags = 0;
}

int rr_create(int device_ordinal, rr_context** out)
{
    if (!out) return RR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RR_ERR_NO_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return RR_ERR_INVALID_ARGUMENT;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return RR_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RR_ERR_NO_DEVICE;   // the code object is gfx950 only
    rr_context* ctx = new (std::nothrow) rr_context();
    if (!ctx) return RR_ERR_OUT_OF_MEMORY;
    ctx->device = device_ordinal;
    ctx->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipSetDevice(device_ordinal) != hipSuccess || ctx->own_stream.create(hipStreamNonBlocking) != hipSuccess ||
        ctx->d_cnt.alloc(1) != hipSuccess || ctx->d_tickets.alloc((rr_context::MAX_LANES + 1) * LDS_TICKET_WORDS) != hipSuccess) {
        delete ctx;
        return RR_ERR_DEVICE;
    }
    ctx->stream = ctx->own_stream.get();
    (void)hipMemsetAsync(ctx->d_cnt.get(), 0, sizeof(CounterBlock), ctx->stream);
    (void)hipMemsetAsync(ctx->d_tickets.get(), 0, (rr_context::MAX_LANES + 1) * LDS_TICKET_WORDS * sizeof(uint32_t), ctx->stream);   // the kernel leaves them zero
    if (const char* e = getenv("RR_DEBUG_KERNEL"))
        ctx->dbg.kernel = !strcmp(e, "fused") ? 1 : !strcmp(e, "lds") ? 4 : !strcmp(e, "paths") ? 5 : !strcmp(e, "stream") ? 10 : 0;
    if (const char* e = getenv("RR_DEBUG_STACK")) ctx->dbg.stack = atoi(e);
    if (const char* e = getenv("RR_DEBUG_TICKET")) ctx->dbg_ticket_blocks = atoi(e);
    if (const char* e = getenv("RR_DEBUG_SHAPE")) ctx->dbg_shape = atoi(e);
    if (const char* e = getenv("RR_DEBUG_TLAS32")) ctx->dbg.tlas32 = atoi(e) != 0;
    if (const char* e = getenv("RR_DEBUG_TILE_ORDER")) ctx->dbg_tile_order = atoi(e) != 0;
    if (const char* e = getenv("RR_DEBUG_ASYNC")) { unsigned l = 2, sh = 2; if (sscanf(e, "%u,%u", &l, &sh) == 2 && l >= 1 && sh >= 1) { ctx->dbg_async[0] = l; ctx->dbg_async[1] = sh; ctx->dbg_async_set = true; } }
    if (const char* e = getenv("RR_DEBUG_DIAG")) ctx->dbg_diag = e;
    if (const char* e = getenv("RR_DEBUG_GROUP_TRACE")) ctx->dbg_group_trace = atoi(e) != 0;
    *out = ctx;
    return RR_OK;
}

int rr_destroy(rr_context* ctx)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (const Stream& s : ctx->lane_stream) if (s.get()) (void)hipStreamSynchronize(s.get());
    delete ctx;          // (its members release what it holds)
    return RR_OK;
}

const char* rr_last_error(const rr_context* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rr_set_stream(rr_context* ctx, void* hip_stream)
{
    if (int r = use_device(ctx)) return r;
    RR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = (hipStream_t)hip_stream;         // NULL is a stream too: HIP's default stream
    return RR_OK;
}

int rr_reset_stream(rr_context* ctx)
{
    if (int r = use_device(ctx)) return r;
    RR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = ctx->own_stream.get();
    return RR_OK;
}

namespace {
// the context's stream waits for everything submitted to the lanes
int join_lanes(rr_context* ctx)
{
    for (uint32_t l = 0; l < rr_context::MAX_LANES; ++l)
        if (ctx->lane_busy[l]) {
            RR_HIP(hipStreamWaitEvent(ctx->stream, ctx->lane_done[l].get(), 0));
            ctx->lane_busy[l] = false;
        }
    return RR_OK;
}
} // namespace

int rr_wait(rr_context* ctx)
{
    if (int r = use_device(ctx)) return r;
    if (int r = join_lanes(ctx)) return r;
    RR_HIP(hipStreamSynchronize(ctx->stream));
    return RR_OK;
}

int rr_set_frames_in_flight(rr_context* ctx, uint32_t n)
{
    if (int r = use_device(ctx)) return r;
    if (n == 0 || n > rr_context::MAX_LANES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_frames_in_flight: 1..4");
    ctx->frames_in_flight = n;
    return RR_OK;
}

int rr_lane_join(rr_context* ctx, uint32_t lane)
{
    if (int r = use_device(ctx)) return r;
    if (lane >= rr_context::MAX_LANES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_lane_join: lane out of range");
    if (ctx->lane_busy[lane]) {
        RR_HIP(hipStreamWaitEvent(ctx->stream, ctx->lane_done[lane].get(), 0));
        ctx->lane_busy[lane] = false;
    }
    return RR_OK;
}

int rr_upload_mesh(rr_context* ctx, const rr_vertex* verts, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices,
                   uint32_t* mesh_id)
{
    if (int r = use_device(ctx)) return r;
    if (!verts || !indices || !mesh_id || n_verts == 0 || n_indices < 3 || n_indices % 3 != 0)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_upload_mesh: need >= 1 triangle, n_indices % 3 == 0");
    for (uint32_t i = 0; i < n_indices; ++i)
        if (indices[i] >= n_verts) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_upload_mesh: index out of range");
    if (rr_host_validate_positions(verts, n_verts, nullptr) != RR_OK)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_upload_mesh: non-finite or huge (> 1e18) vertex position");
    MeshRes m;
    m.n_verts = n_verts; m.n_idx = n_indices; m.n_tris = n_indices / 3;
    RR_HIP(m.d_verts.alloc((size_t)n_verts * 8));
    if (hipError_t e = m.d_idx.alloc(n_indices)) return fail(ctx, RR_ERR_OUT_OF_MEMORY, "hipMalloc(indices)", e);
    // Mesh.cpp:76-79,88-91: memcpy into the mapped upload buffers
    RR_HIP_MSG(hipMemcpyAsync(m.d_verts.get(), verts, (size_t)n_verts * sizeof(rr_vertex), hipMemcpyHostToDevice, ctx->stream), "mesh upload");
    RR_HIP_MSG(hipMemcpyAsync(m.d_idx.get(), indices, (size_t)n_indices * 4, hipMemcpyHostToDevice, ctx->stream), "mesh upload");
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "mesh upload");   // caller keeps ownership of the host arrays
    ctx->meshes.push_back(std::move(m));
    *mesh_id = (uint32_t)ctx->meshes.size() - 1u;
    return RR_OK;
}

int rr_upload_envmap(rr_context* ctx, const float* rgb, int32_t w, int32_t h)
{
    if (int r = use_device(ctx)) return r;
    if (!rgb || w <= 0 || h <= 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_upload_envmap: null data or empty size");
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<float> staging;
    DevBuf<float4> env;
    RR_HIP(staging.alloc(n * 3));
    RR_HIP_MSG(env.alloc(n), "env upload");
    RR_HIP_MSG(hipMemcpyAsync(staging.get(), rgb, n * 12, hipMemcpyHostToDevice, ctx->stream), "env upload");   // RowPitch = x*3*4 (:128)
    RR_HIP_MSG(launch_env_pad(staging.get(), env.get(), (uint32_t)n, ctx->stream), "env upload");
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "env upload");
    ctx->d_env = std::move(env); ctx->env_w = w; ctx->env_h = h;
    return RR_OK;
}

int rr_build_blas(rr_context* ctx, uint32_t mesh_id) { return rr_build_blas_ex(ctx, mesh_id, RR_BUILD_PREFER_FAST_TRACE); }

} // extern "C"

namespace {

int ensure_upd(rr_context* ctx, MeshRes& m)
{
    if (m.d_upd.get()) return RR_OK;
    RR_HIP(m.d_upd.alloc(8));
    RR_HIP(hipMemsetAsync(m.d_upd.get(), 0, 8 * sizeof(uint32_t), ctx->stream));
    return RR_OK;
}

// the verdict of the device vertex updates since the last build (rr_update_mesh_vertices_device); clears it
int take_device_verdict(rr_context* ctx, MeshRes& m)
{
    if (!m.dev_pending) return RR_OK;
    uint32_t rejected = 0;
    RR_HIP(hipMemcpyAsync(&rejected, m.d_upd.get() + 7, 4, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipMemsetAsync(m.d_upd.get() + 7, 0, 4, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    m.dev_pending = false;
    if (rejected)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT,
                    "rr_build_blas: a device vertex update held a non-finite or huge (> 1e18) position and was not applied");
    return RR_OK;
}

void set_bounds(MeshRes& m, const uint32_t sb[6])
{
    for (int k = 0; k < 6; ++k) m.bounds[k] = ord2f_host(sb[k]);
    m.scale = 0.0f;
    for (int k = 0; k < 6; ++k) m.scale = std::max(m.scale, std::fabs(m.bounds[k]));
    m.grid = make_grid(m.bounds);
}

// PERFORM_UPDATE: the kept hierarchy over the mesh's current vertices -- one refit launch (leaf records, boxes, bounds), the
// bounds read back for the grid, one quantize launch.  Child refs and depth stay.
int refit_blas(rr_context* ctx, MeshRes& m)
{
    if (!m.built || !m.allow_update)
        return fail(ctx, RR_ERR_STATE, "rr_build_blas: PERFORM_UPDATE needs a BLAS built with RR_BUILD_ALLOW_UPDATE");
    const uint32_t n = m.n_tris;
    ctx->tlas_built = false;      // the pooled copies of this BLAS are stale until the TLAS is rebuilt or updated
    RR_HIP(launch_refit_blas(m.d_verts.get(), m.d_idx.get(), n, m.tris.get(), m.nrms.get(), m.nodes.get(), m.links.get(), m.visit.get(),
                             m.d_upd.get(), ctx->stream));
    uint32_t sb[6];
    RR_HIP(hipMemcpyAsync(sb, m.d_upd.get(), sizeof sb, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    set_bounds(m, sb);
    RR_HIP(launch_quantize_nodes(m.qnodes.get(), m.nodes.get(), n > 1 ? n - 1 : 1, m.grid, 0, 0, ctx->stream));
    m.stale = false;
    ++m.version;
    return RR_OK;
}

} // namespace

extern "C" {

int rr_build_blas_ex(rr_context* ctx, uint32_t mesh_id, uint32_t flags)
{
    const Range range_("rr_build_blas");
    if (int r = use_device(ctx)) return r;
    if (mesh_id >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_build_blas: unknown mesh id");
    MeshRes& m = ctx->meshes[mesh_id];
    if (int r = take_device_verdict(ctx, m)) return r;
    if (flags & RR_BUILD_PERFORM_UPDATE) return refit_blas(ctx, m);
    const uint32_t n = m.n_tris;
    if ((uint64_t)n * sizeof(QNode) >= 0x7fffffffull) return fail(ctx, RR_ERR_UNSUPPORTED, "rr_build_blas: mesh too large for 31-bit node refs");
    const bool keep = (flags & RR_BUILD_ALLOW_UPDATE) != 0;
    BuildScratch s;
    if (int r = alloc_build(ctx, n, s)) return r;
    m.nodes.reset(); m.qnodes.reset(); m.tris.reset(); m.nrms.reset(); m.links.reset(); m.visit.reset();
    m.built = false;
    m.allow_update = false;
    RR_HIP(m.nodes.alloc(n > 1 ? n - 1 : 1));
    RR_HIP(m.qnodes.alloc(n > 1 ? n - 1 : 1));
    RR_HIP(m.tris.alloc(n));
    RR_HIP(m.nrms.alloc(n));
    if (keep) {
        if (int r = ensure_upd(ctx, m)) return r;
        if (n > 1) {
            RR_HIP(m.links.alloc(2 * (size_t)n - 1));
            RR_HIP(m.visit.alloc(n - 1));
            RR_HIP(hipMemsetAsync(m.visit.get(), 0, (size_t)(n - 1) * sizeof(uint32_t), ctx->stream));
        }
    }
    s.b.nodes = m.nodes.get();
    RR_HIP(launch_tri_setup(m.d_verts.get(), m.d_idx.get(), n, s.b, ctx->stream));
    if ((flags & RR_BUILD_PREFER_FAST_TRACE) && !(flags & RR_BUILD_PREFER_FAST_BUILD) && n > 1 && n <= PLOC_MAX_PRIMS)
        RR_HIP(launch_ploc(s.b, ctx->stream));          // clustered hierarchy (fewer node visits)
    else
        RR_HIP(launch_lbvh(s.b, ctx->stream));          // Karras radix tree (fastest build, any size)
    if (keep) RR_HIP(launch_keep_links(s.b, m.links.get(), ctx->stream));
    RR_HIP(launch_pack_tris(m.d_verts.get(), m.d_idx.get(), s.b, m.tris.get(), m.nrms.get(), ctx->stream));
    uint32_t sb[6], depth = 0;
    RR_HIP(hipMemcpyAsync(sb, s.b.scene_box, sizeof sb, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipMemcpyAsync(&depth, s.b.depth, 4, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    set_bounds(m, sb);
    m.depth = depth;
    RR_HIP(launch_quantize_nodes(m.qnodes.get(), m.nodes.get(), n > 1 ? n - 1 : 1, m.grid, 0, 0, ctx->stream));
    if (depth > 64) return fail(ctx, RR_ERR_UNSUPPORTED, "rr_build_blas: LBVH deeper than the 64-entry traversal stack");
    m.built = true;
    m.allow_update = keep;
    m.stale = false;
    ++m.version;
    ctx->tlas_built = false;      // any TLAS built before refers to the old BLAS
    return RR_OK;
}

int rr_update_mesh_vertices(rr_context* ctx, uint32_t mesh_id, const rr_vertex* verts, uint32_t n_verts)
{
    if (int r = use_device(ctx)) return r;
    if (mesh_id >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_update_mesh_vertices: unknown mesh id");
    MeshRes& m = ctx->meshes[mesh_id];
    if (!verts || n_verts != m.n_verts)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_update_mesh_vertices: need the uploaded vertex count");
    if (rr_host_validate_positions(verts, n_verts, nullptr) != RR_OK)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_update_mesh_vertices: non-finite or huge (> 1e18) vertex position");
    RR_HIP(hipMemcpyAsync(m.d_verts.get(), verts, (size_t)n_verts * sizeof(rr_vertex), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));   // caller keeps ownership of the host array
    m.stale = true;
    return RR_OK;
}

int rr_update_mesh_vertices_device(rr_context* ctx, uint32_t mesh_id, const void* d_verts, uint32_t n_verts)
{
    if (int r = use_device(ctx)) return r;
    if (mesh_id >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_update_mesh_vertices_device: unknown mesh id");
    MeshRes& m = ctx->meshes[mesh_id];
    if (!d_verts || ((uintptr_t)d_verts & 3u) != 0 || n_verts != m.n_verts)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_update_mesh_vertices_device: need a 4-byte aligned pointer and the uploaded vertex count");
    if (int r = ensure_upd(ctx, m)) return r;
    RR_HIP(launch_update_verts(d_verts, m.d_verts.get(), n_verts, m.d_upd.get() + 6, ctx->stream));
    m.stale = true;
    m.dev_pending = true;
    return RR_OK;
}

} // extern "C"

namespace {

// per-instance device records, transforms + BLAS bounds (launch_inst_setup's layout) and the world-space scale of a scene
int tlas_inputs(rr_context* ctx, const rr_instance_desc* instances, uint32_t n, const std::vector<uint32_t>& node_off,
                std::vector<InstDev>& host, std::vector<float>& xb, float& scene_scale)
{
    static const float ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    host.assign(n, InstDev());
    xb.assign((size_t)n * 18, 0.0f);
    scene_scale = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {
        const rr_instance_desc& d = instances[i];
        const MeshRes& m = ctx->meshes[(size_t)d.blas];
        InstDev& o = host[i];
        memset(&o, 0, sizeof o);
        o.identity = memcmp(d.transform, ident, sizeof ident) == 0 ? 1u : 0u;
        if (o.identity) memcpy(o.inv, ident, sizeof ident);
        else {
            affine_inverse(d.transform, o.inv);
            for (int k = 0; k < 12; ++k)
                if (!std::isfinite(o.inv[k])) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_build_tlas: singular instance transform");
        }
        o.root = node_off[(size_t)d.blas] * (uint32_t)sizeof(QNode);     // byte offset, like every internal child ref
        o.scale = m.scale;
        o.grid = m.grid;
        for (int c = 0; c < 8; ++c) {       // world-space extent of the instance (for the TLAS box padding)
            const float x = (c & 1) ? m.bounds[3] : m.bounds[0], y = (c & 2) ? m.bounds[4] : m.bounds[1], z = (c & 4) ? m.bounds[5] : m.bounds[2];
            for (int r = 0; r < 3; ++r)
                scene_scale = std::max(scene_scale, std::fabs(d.transform[4 * r] * x + d.transform[4 * r + 1] * y + d.transform[4 * r + 2] * z + d.transform[4 * r + 3]));
        }
        o.flags = d.hitgroup_flags >> 24;
        o.mask = d.instance_id_mask >> 24;
        memcpy(&xb[(size_t)i * 12], d.transform, 48);
        memcpy(&xb[(size_t)n * 12 + (size_t)i * 6], m.bounds, 24);
    }
    return RR_OK;
}

// scene grid = the box of the TLAS root (node 0 holds the boxes of its two children)
void scene_from_root(rr_context* ctx, const BvhNode& root)
{
    float sb[6] = { 3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f };
    for (int k = 0; k < 2; ++k) {
        if (!(root.lox[k] <= root.hix[k])) continue;           // the empty second child of a one-instance TLAS
        sb[0] = std::min(sb[0], root.lox[k]); sb[1] = std::min(sb[1], root.loy[k]); sb[2] = std::min(sb[2], root.loz[k]);
        sb[3] = std::max(sb[3], root.hix[k]); sb[4] = std::max(sb[4], root.hiy[k]); sb[5] = std::max(sb[5], root.hiz[k]);
    }
    ctx->scene_grid = make_grid(sb);
    memcpy(ctx->scene_bounds, sb, sizeof sb);
}

// quantize + copy into the pools every BLAS of the scene whose version differs from the pooled one (all of them after a build)
// (`what` names the TLAS step in a failure)
int repool(rr_context* ctx, const char* what)
{
    // (pool_node_off covers the meshes that existed at the TLAS build; later uploads are not in the scene)
    for (size_t mi = 0; mi < ctx->pool_node_off.size(); ++mi) {
        if (ctx->pool_node_off[mi] == 0xffffffffu) continue;
        const MeshRes& m = ctx->meshes[mi];
        if (ctx->pool_version[mi] == m.version) continue;
        const uint32_t no = ctx->pool_node_off[mi], to = ctx->pool_tri_off[mi];
        RR_HIP_MSG(launch_quantize_nodes(ctx->d_pool_qnodes.get() + no, m.nodes.get(), m.n_tris > 1 ? m.n_tris - 1 : 1, m.grid, no, to, ctx->stream), what);
        RR_HIP_MSG(hipMemcpyAsync(ctx->d_pool_tris.get() + to, m.tris.get(), (size_t)m.n_tris * sizeof(TriRec), hipMemcpyDeviceToDevice, ctx->stream), what);
        RR_HIP_MSG(hipMemcpyAsync(ctx->d_pool_nrms.get() + to, m.nrms.get(), (size_t)m.n_tris * sizeof(NrmRec), hipMemcpyDeviceToDevice, ctx->stream), what);
        ctx->pool_version[mi] = m.version;
    }
    return RR_OK;
}

// what a successful TLAS build or update leaves in the context
int finish_tlas(rr_context* ctx, const rr_instance_desc* instances, uint32_t n, const InstDev& inst0, float scene_scale)
{
    ctx->inst_host.assign(instances, instances + n);
    ctx->n_insts = n;
    ctx->scene_scale = scene_scale;
    const rr_instance_desc& d0 = instances[0];
    ctx->single_identity = n == 1 && inst0.identity && (d0.hitgroup_flags >> 24) == 0 && ((d0.instance_id_mask >> 24) & 0xffu) != 0;
    if (scene_stack_need(ctx) > 64) return fail(ctx, RR_ERR_UNSUPPORTED, "rr_build_tlas: TLAS+BLAS deeper than the 64-entry stack");
    ctx->tlas_built = true;
    for (ChoiceClass& c : ctx->ch) c = ChoiceClass();         // a new scene: the kernels are chosen afresh
    return RR_OK;
}

// PERFORM_UPDATE of the top level: same instance count, same BLAS per slot; transforms, masks and flags may change
int refit_tlas(rr_context* ctx, const rr_instance_desc* instances, uint32_t n)
{
    if (!ctx->tlas_refittable) return fail(ctx, RR_ERR_STATE, "rr_build_tlas: PERFORM_UPDATE needs a TLAS built with RR_BUILD_ALLOW_UPDATE");
    if (n != ctx->n_insts) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_build_tlas: PERFORM_UPDATE needs the instance count of the build");
    for (uint32_t i = 0; i < n; ++i)
        if (instances[i].blas != ctx->inst_host[i].blas)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_build_tlas: PERFORM_UPDATE needs the same BLAS in every instance slot");
    std::vector<InstDev> host;
    std::vector<float> xb;
    float scene_scale = 0.0f;
    if (int r = tlas_inputs(ctx, instances, n, ctx->pool_node_off, host, xb, scene_scale)) return r;
    ctx->tlas_built = false;
    DevBuf<float> d_xb;
    RR_HIP(d_xb.alloc(xb.size()));
    const uint32_t n_tlas = n > 1 ? n - 1 : 1;
    BvhNode root;
    RR_HIP_MSG(hipMemcpyAsync(ctx->d_insts.get(), host.data(), (size_t)n * sizeof(InstDev), hipMemcpyHostToDevice, ctx->stream), "TLAS update");
    RR_HIP_MSG(hipMemcpyAsync(d_xb.get(), xb.data(), xb.size() * 4, hipMemcpyHostToDevice, ctx->stream), "TLAS update");
    RR_HIP_MSG(launch_refit_tlas(ctx->d_insts.get(), d_xb.get(), n, ctx->d_pool_nodes.get(), ctx->d_tlas_links.get(), ctx->d_tlas_visit.get(), ctx->stream),
               "TLAS update");
    RR_HIP_MSG(hipMemcpyAsync(&root, ctx->d_pool_nodes.get(), sizeof root, hipMemcpyDeviceToHost, ctx->stream), "TLAS update");
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "TLAS update");
    scene_from_root(ctx, root);
    RR_HIP_MSG(launch_quantize_nodes(ctx->d_pool_qnodes.get(), ctx->d_pool_nodes.get(), n_tlas, ctx->scene_grid, 0, 0, ctx->stream), "TLAS update");
    if (int r = repool(ctx, "TLAS update")) return r;
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "TLAS update");
    return finish_tlas(ctx, instances, n, host[0], scene_scale);
}

} // namespace

extern "C" {

int rr_build_tlas(rr_context* ctx, const rr_instance_desc* instances, uint32_t n) { return rr_build_tlas_ex(ctx, instances, n, 0u); }

int rr_build_tlas_ex(rr_context* ctx, const rr_instance_desc* instances, uint32_t n, uint32_t flags)
{
    const Range range_("rr_build_tlas");
    if (int r = use_device(ctx)) return r;
    if (!instances || n == 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_build_tlas: need >= 1 instance");
    for (uint32_t i = 0; i < n; ++i) {
        if (instances[i].blas >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_build_tlas: unknown BLAS");
        const MeshRes& m = ctx->meshes[(size_t)instances[i].blas];
        if (!m.built) return fail(ctx, RR_ERR_STATE, "rr_build_tlas: BLAS not built");
        if (m.stale) return fail(ctx, RR_ERR_STATE, "rr_build_tlas: BLAS out of date (its vertices changed): rebuild or update it first");
    }
    if (flags & RR_BUILD_PERFORM_UPDATE) return refit_tlas(ctx, instances, n);
    const bool keep = (flags & RR_BUILD_ALLOW_UPDATE) != 0;
    // pool layout: nodes [0, n_tlas) TLAS, then each distinct BLAS; triangles / normals concatenated
    const uint32_t n_tlas = n > 1 ? n - 1 : 1;
    std::vector<uint32_t> node_off(ctx->meshes.size(), 0xffffffffu), tri_off(ctx->meshes.size(), 0);
    uint32_t n_pool_nodes = n_tlas, n_pool_tris = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const size_t mi = (size_t)instances[i].blas;
        if (node_off[mi] != 0xffffffffu) continue;
        const MeshRes& m = ctx->meshes[mi];
        node_off[mi] = n_pool_nodes; tri_off[mi] = n_pool_tris;
        n_pool_nodes += m.n_tris > 1 ? m.n_tris - 1 : 1;
        n_pool_tris += m.n_tris;
    }
    if ((uint64_t)n_pool_tris + n >= 0x7fffffffull || (uint64_t)n_pool_nodes * sizeof(QNode) >= 0x7fffffffull)
        return fail(ctx, RR_ERR_UNSUPPORTED, "rr_build_tlas: scene too large for 31-bit node / leaf refs");
    std::vector<InstDev> host;
    std::vector<float> xb;
    float scene_scale = 0.0f;
    if (int r = tlas_inputs(ctx, instances, n, node_off, host, xb, scene_scale)) return r;
    ctx->tlas_built = false;
    ctx->tlas_refittable = false;
    ctx->d_insts.reset(); ctx->d_pool_nodes.reset(); ctx->d_pool_qnodes.reset(); ctx->d_pool_tris.reset(); ctx->d_pool_nrms.reset();
    ctx->d_tlas_links.reset(); ctx->d_tlas_visit.reset();
    RR_HIP(ctx->d_insts.alloc(n));
    RR_HIP(ctx->d_pool_nodes.alloc(n_tlas));
    RR_HIP(ctx->d_pool_qnodes.alloc(n_pool_nodes));
    RR_HIP(ctx->d_pool_tris.alloc(n_pool_tris));
    RR_HIP(ctx->d_pool_nrms.alloc(n_pool_tris));
    if (keep && n > 1) {
        RR_HIP(ctx->d_tlas_links.alloc(2 * (size_t)n - 1));
        RR_HIP(ctx->d_tlas_visit.alloc(n - 1));
        RR_HIP(hipMemsetAsync(ctx->d_tlas_visit.get(), 0, (size_t)(n - 1) * sizeof(uint32_t), ctx->stream));
    }
    ctx->pool_node_off = node_off;
    ctx->pool_tri_off = tri_off;
    ctx->pool_version.assign(ctx->meshes.size(), ~0ull);     // nothing pooled yet: repool copies every BLAS of the scene
    DevBuf<float> d_xb;
    RR_HIP(d_xb.alloc(xb.size()));
    BuildScratch s;
    if (int r = alloc_build(ctx, n, s)) return r;
    s.b.nodes = ctx->d_pool_nodes.get();
    s.b.leaf_ref_prim = 1;
    s.b.leaf_base = n_pool_tris;                  // an instance leaf is ~(n_pool_tris + instance index)
    RR_HIP_MSG(hipMemcpyAsync(ctx->d_insts.get(), host.data(), (size_t)n * sizeof(InstDev), hipMemcpyHostToDevice, ctx->stream), "TLAS build");
    RR_HIP_MSG(hipMemcpyAsync(d_xb.get(), xb.data(), xb.size() * 4, hipMemcpyHostToDevice, ctx->stream), "TLAS build");
    RR_HIP_MSG(launch_inst_setup(ctx->d_insts.get(), d_xb.get(), n, s.b, ctx->stream), "TLAS build");
    // (the top level keeps the Karras hierarchy: the clustered builder, tried on it in round 3, makes the 1 024-instance grid
    // 5 % slower on both renderers -- on a regular lattice every merged-box area ties)
    RR_HIP_MSG(launch_lbvh(s.b, ctx->stream), "TLAS build");
    if (keep) RR_HIP_MSG(launch_keep_links(s.b, ctx->d_tlas_links.get(), ctx->stream), "TLAS build");
    uint32_t depth = 0;
    BvhNode root;
    RR_HIP_MSG(hipMemcpyAsync(&depth, s.b.depth, 4, hipMemcpyDeviceToHost, ctx->stream), "TLAS build");
    RR_HIP_MSG(hipMemcpyAsync(&root, ctx->d_pool_nodes.get(), sizeof root, hipMemcpyDeviceToHost, ctx->stream), "TLAS build");
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "TLAS build");
    scene_from_root(ctx, root);
    RR_HIP_MSG(launch_quantize_nodes(ctx->d_pool_qnodes.get(), ctx->d_pool_nodes.get(), n_tlas, ctx->scene_grid, 0, 0, ctx->stream), "TLAS build");
    if (int r = repool(ctx, "TLAS build")) return r;
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "TLAS build");
    ctx->n_pool_tris = n_pool_tris; ctx->n_pool_nodes = n_pool_nodes;
    ctx->tlas_depth = depth;
    ctx->tlas_refittable = keep;
    return finish_tlas(ctx, instances, n, host[0], scene_scale);
}

int rr_set_camera(rr_context* ctx, const rr_scene_constants* constants)
{
    if (!ctx || !constants) return RR_ERR_INVALID_ARGUMENT;
    ctx->cam = *constants;
    ctx->cam_set = true;
    return RR_OK;
}

int rr_set_tile_partition(rr_context* ctx, uint32_t rank, uint32_t world)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    if (world == 0 || rank >= world) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_tile_partition: need rank < world");
    ctx->tile_rank = rank; ctx->tile_world = world;
    return RR_OK;
}

// round-robin tiles of a W x H frame: tiles across, tiles, this rank's, the most any rank has
struct Tiles { uint32_t tiles_x, n_tiles, local, max_local; };
static Tiles tile_counts(uint32_t W, uint32_t H, uint32_t rank, uint32_t world)
{
    const uint32_t tiles_x = (W + TILE - 1) / TILE, n_tiles = tiles_x * ((H + TILE - 1) / TILE);
    return { tiles_x, n_tiles, n_tiles > rank ? (n_tiles - rank + world - 1) / world : 0, (n_tiles + world - 1) / world };
}

int rr_local_tile_count(rr_context* ctx, uint32_t width, uint32_t height, uint32_t* n_tiles, uint32_t* max_tiles_any_rank)
{
    if (!ctx || width == 0 || height == 0) return RR_ERR_INVALID_ARGUMENT;
    const Tiles t = tile_counts(width, height, ctx->tile_rank, ctx->tile_world);
    if (n_tiles) *n_tiles = t.local;
    if (max_tiles_any_rank) *max_tiles_any_rank = t.max_local;
    return RR_OK;
}

namespace {

int ensure_cams(rr_context* ctx, size_t n)
{
    return n <= ctx->d_cams.size() ? RR_OK : ctx->d_cams.grow(ctx, n < 64 ? 64 : n);
}

// DispatchRays(W, H, depth): slice f uses the constants d_cams[f] and writes to out + f*stride.
// ext_tiles != null: compact tile output into caller memory with the given stride (sharded frames).
int ensure_frame_buffers(rr_context* ctx, size_t elems, bool want_f32)
{
    if (elems > ctx->d_rgba8.size())
        if (int r = ctx->d_rgba8.grow(ctx, elems)) return r;
    if (want_f32 && elems > ctx->d_f32.size()) return ctx->d_f32.grow(ctx, elems);
    return RR_OK;
}

int ensure_lane(rr_context* ctx, uint32_t lane)
{
    if (ctx->lane_stream[lane].get()) return RR_OK;
    RR_HIP(ctx->lane_stream[lane].create(hipStreamNonBlocking));
    RR_HIP(ctx->lane_fork[lane].create(hipEventDisableTiming));
    RR_HIP(ctx->lane_done[lane].create(hipEventDisableTiming));
    return RR_OK;
}


// ---- k_stream_* : buffers and passes ----------------------------------------------------------------------------------
// One pass renders `fc` consecutive slices of the dispatch.  Worst case per pixel of the ray kernels' blocks: four rays alive in
// one generation (max_reflect <= 2), so a queue holds 4 x pixels entries plus what the waves' 1 024-entry reservations can
// leave unused; slots are 64 B and the mark 1 B per pixel.  A pass is sized to stay inside the budget of its buffer set: a sixth
// of the memory free when the renderer is first used, at most 48 GB -- every kernel of a pass ends in a tail of a few long
// chains, so passes should be few (the 1 024-instance scene at 2160p, Depth 16: 4.04 / 3.68 / 3.49 / 3.39 ms per frame with
// 6 / 12 / 24 / 48 GB, i.e. 2 / 4 / 8 / 16 slices per pass).  The buffers are kept for the life of the context.
constexpr size_t STREAM_BUDGET_MAX = (size_t)48 << 30, STREAM_BUDGET_MIN = (size_t)1 << 30;
constexpr uint32_t STREAM_BLK = 1024;

size_t stream_budget(rr_context* ctx)
{
    if (ctx->strm_budget == 0) {
        size_t free_b = 0, total_b = 0;
        size_t b = STREAM_BUDGET_MAX;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) b = std::min(b, free_b / 6u);
        if (const char* e = getenv("RR_DEBUG_STREAM_BUDGET_GB")) { const long g = atol(e); if (g > 0 && g <= 200) b = (size_t)g << 30; }
        ctx->strm_budget = std::max(b, STREAM_BUDGET_MIN);
    }
    return ctx->strm_budget;
}

// nodes of a BLAS as k_render_lds holds them in LDS
uint32_t lds_node_bytes(const MeshRes& m) { return (m.n_tris > 1 ? m.n_tris - 1 : 1) * (uint32_t)sizeof(QNode); }

// what the kernel choice (rr_choice.h) knows of the scene
SceneFacts scene_facts(const rr_context* ctx)
{
    SceneFacts s = { ctx->single_identity, scene_stack_need(ctx), 0, ctx->n_pool_nodes, ctx->n_pool_tris + ctx->n_insts, false };
    if (ctx->single_identity && !ctx->inst_host.empty()) {
        const MeshRes& m0 = ctx->meshes[(size_t)ctx->inst_host[0].blas];
        s.blas_tris = m0.n_tris;
        s.lds_fits = ctx->dbg.stack == 0 && m0.n_tris < 32768u && lds_kernel_shape(lds_node_bytes(m0), s.need + 1, nullptr, ctx->dbg_shape) >= 0;
    }
    return s;
}

// what the kernel choice knows of a launch of `depth` slices whose scene rectangle (pixels) is `rect`
LaunchFacts launch_facts(const rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth, const uint32_t rect[4],
                         const rr_dispatch_params& p, bool compact, bool mesh)
{
    return { depth, ((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE), ctx->tile_world, compact, mesh,
             rect[2] > rect[0] && rect[3] > rect[1], (double)(rect[2] - rect[0]) * (double)(rect[3] - rect[1]) / ((double)width * (double)height),
             p.max_refract, p.max_reflect, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) != 0, !ctx->dbg_diag.empty() && ctx->single_identity };
}

// the buffer set of the stream the dispatch is on (launches on one stream are ordered: one set per stream)
uint32_t stream_slot(const rr_context* ctx)
{
    for (uint32_t l = 0; l < rr_context::MAX_LANES; ++l) if (ctx->lane_stream[l].get() && ctx->stream == ctx->lane_stream[l].get()) return l;
    return rr_context::MAX_LANES;
}

struct StreamPlan { uint32_t fc, n_wg; size_t cap, pixels; };

// wave-blocks of `frames` slices that the ray kernels render: the tiles that touch the scene's screen rectangle come first in
// launch order (under the mesh-tile partition: this rank's mesh tiles), in groups of eight tiles
size_t stream_rect_wb(const DispatchDev& a, uint32_t frames)
{
    const size_t all = (size_t)a.blocks_per_frame * frames * 4u;
    if (!a.mesh_part && a.rt_w == 0u) return all;
    const size_t tiles = a.mesh_part ? (size_t)a.n_mesh_local : (size_t)a.rt_w * a.rt_h;
    return std::min(all, ((tiles + 7u) / 8u) * 128u * frames);
}

StreamPlan stream_plan(rr_context* ctx, const DispatchDev& a, uint32_t depth)
{
    auto bytes = [&](uint32_t frames, StreamPlan& pl) -> size_t {
        const size_t wb = stream_rect_wb(a, frames);
        pl.pixels = wb * 64u;
        pl.n_wg = (uint32_t)std::min<size_t>((size_t)ctx->n_cus * 6u, std::max<size_t>(1u, (wb + 15u) / 16u));     // six workgroups of the ray kernels fit a CU
        pl.cap = ((4u * pl.pixels + (size_t)pl.n_wg * 4u * STREAM_BLK + STREAM_BLK - 1u) / STREAM_BLK) * STREAM_BLK;
        return 2u * pl.cap * 48u + 2u * (pl.cap / 64u) * 4u + pl.pixels * 65u;
    };
    StreamPlan pl{ 1, 1, 0, 0 };
    uint32_t fc = depth;
    const size_t budget = stream_budget(ctx);
    while (fc > 1u && bytes(fc, pl) > budget) fc = (fc + 1u) / 2u;
    (void)bytes(fc, pl);
    pl.fc = fc;
    return pl;
}

int ensure_stream_buffers(rr_context* ctx, const StreamPlan& pl)
{
    if (pl.cap > 0xffffffffull || pl.pixels > 0xffffffffull) return fail(ctx, RR_ERR_UNSUPPORTED, "stream renderer: pass too large for 32-bit ray indices");
    StreamSet& sd = ctx->strm[stream_slot(ctx)];
    if (!sd.heads.get())      // head counters and, behind them, the chunk ticket counters: one block, zeroed by one memset per pass
        RR_HIP(sd.heads.alloc(STREAM_MAX_GEN + STREAM_MAX_GEN * 8u * 16u));
    if (pl.cap > sd.q[1].size()) {
        RR_HIP(hipStreamSynchronize(ctx->stream));          // (this stream is the set's only user)
        sd.q[0].reset(); sd.q[1].reset(); sd.fill[0].reset(); sd.fill[1].reset();
        for (int k = 0; k < 2; ++k) RR_HIP(sd.fill[k].alloc(pl.cap / 64u));
        for (int k = 0; k < 2; ++k) RR_HIP(sd.q[k].alloc(pl.cap, 48u));
    }
    if (pl.pixels > sd.pending.size()) {
        RR_HIP(hipStreamSynchronize(ctx->stream));
        sd.slots.reset(); sd.pending.reset();
        RR_HIP(sd.slots.alloc(pl.pixels, 64u));
        RR_HIP(sd.pending.alloc(pl.pixels));
    }
    return RR_OK;
}

// the whole dispatch through the generation-per-kernel renderer, `fc` slices per pass
int render_stream(rr_context* ctx, const SceneDev& sc, const DispatchDev& a, uint32_t depth, int need, bool stats)
{
    const StreamPlan pl = stream_plan(ctx, a, depth);
    if (int r = ensure_stream_buffers(ctx, pl)) return r;
    const StreamSet& set = ctx->strm[stream_slot(ctx)];
    StreamDev s = { { set.q[0].get(), set.q[1].get() }, { set.fill[0].get(), set.fill[1].get() }, set.heads.get(), set.heads.get() + STREAM_MAX_GEN,
                    set.slots.get(), set.pending.get(), (uint32_t)set.q[1].size(), 0u };
    for (uint32_t f0 = 0; f0 < depth; f0 += pl.fc) {
        const uint32_t fc = std::min(pl.fc, depth - f0);
        DispatchDev b = a;
        // lanes (in sixteenths of the wave's live lanes) a step / a shading pass needs to be issued: measured on the
        // 1 024-instance scene (tools/exp_stream_sweep.sh; RR_DEBUG_ASYNC overrides)
        if (!ctx->dbg_async_set) { b.async_leaf_num = 2u; b.async_shade_num = 8u; }
        b.cams = a.cams + f0;
        b.n_frames = fc;
        b.n_blocks = a.blocks_per_frame * fc;
        b.out_rgba8 = a.out_rgba8 + (size_t)f0 * a.frame_stride;
        if (a.out_f32) b.out_f32 = a.out_f32 + (size_t)f0 * a.frame_stride;
        s.n_rect_wb = (uint32_t)stream_rect_wb(a, fc);
        RR_HIP(launch_render_stream(sc, b, s, need, pl.n_wg, stats, ctx->stream));
    }
    return RR_OK;
}

// mesh-tile partition: the partition the caller's tile buffers were checked against, where rank 0's background tiles go
struct MeshOut { const rr_mesh_partition* part; uint32_t* bg; size_t bg_stride_elems; };

// where a dispatch's slices go: this rank's tiles and the output's element layout (elements are 32-bit words)
struct Layout : Tiles {
    rr_mesh_partition part; uint32_t n_mesh_local;          // mesh: the caller's partition, this rank's mesh tiles
    bool want_f32, compact, rgb8;
    size_t slice_elems, stride, out_base;
};

// checks the request, lays out (and allocates) its output and GenerateCameraRay's screen tables for the frame size
int layout_dispatch(rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth, const rr_scene_constants* h_cams,
                    const rr_dispatch_params& p, uint32_t* ext_tiles, size_t ext_stride_elems, uint32_t out_slot,
                    uint32_t out_slot_depth, const MeshOut* mesh, Layout& o)
{
    if (width == 0 || height == 0 || width > 32768 || height > 32768 || depth == 0 || depth > 65535)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "dispatch: bad frame size or depth");
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "dispatch: build the BLAS and TLAS first");
    if (p.max_refract < 0 || p.max_refract > 65535 || p.max_reflect < 0)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "dispatch: negative bounce limit");
    if (p.max_reflect > 8) return fail(ctx, RR_ERR_UNSUPPORTED, "dispatch: max_reflect > 8 (parked-ray registers)");
    if (!(p.ior > 0.0f)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "dispatch: ior must be > 0");

    static_cast<Tiles&>(o) = tile_counts(width, height, ctx->tile_rank, ctx->tile_world);
    memset(&o.part, 0, sizeof o.part); o.n_mesh_local = 0;
    if (mesh) {         // mesh tiles dealt round robin, background tiles to rank 0: this rank's tiles are its mesh tiles, then those
        if (!ext_tiles || !(p.flags & RR_DISPATCH_TILES_RGB8) || !h_cams || !mesh->part) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "mesh partition: RGB8 tile buffers and host constants");
        // the partition is the caller's (its buffers were sized and checked against it), never recomputed here
        o.part = *mesh->part;
        if (o.part.world != ctx->tile_world || o.part.tiles_x != o.tiles_x || o.part.n_tiles != o.n_tiles) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "mesh partition: not one of this launch");
        o.n_mesh_local = rr_host_mesh_tiles_of_rank(&o.part, ctx->tile_rank);
        if (ctx->tile_rank == 0 && o.part.n_bg_tiles && !mesh->bg) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "mesh partition: rank 0 needs the background tile buffer");
        o.local = o.n_mesh_local + (ctx->tile_rank == 0 ? o.part.n_bg_tiles : 0);
        o.max_local = o.part.max_mesh_tiles_per_rank;
    }
    o.want_f32 = (p.flags & RR_DISPATCH_FLOAT_OUTPUT) != 0;
    o.compact = ctx->tile_world > 1 || ext_tiles != nullptr;
    o.rgb8 = (p.flags & RR_DISPATCH_TILES_RGB8) != 0;
    if (o.rgb8 && !ext_tiles) return fail(ctx, RR_ERR_UNSUPPORTED, "dispatch: RGB8 tiles only exist in external tile buffers (rr_render_orbit_sharded)");
    // an RGB8 tile is 3/4 of an RGBA8 tile
    o.slice_elems = o.compact ? (size_t)o.max_local * TILE * TILE * (o.rgb8 ? 3 : 4) / 4 : (size_t)width * height;
    o.stride = ext_tiles ? ext_stride_elems : o.slice_elems;
    if (ext_tiles && o.want_f32) return fail(ctx, RR_ERR_UNSUPPORTED, "dispatch: float output is not available for external tile buffers");
    o.out_base = ext_tiles ? 0 : o.slice_elems * out_slot_depth * out_slot;
    if (!ext_tiles)
        if (int r = ensure_frame_buffers(ctx, o.out_base + o.slice_elems * depth, o.want_f32)) return r;
    if (width != ctx->screen_w || height != ctx->screen_h) {     // new frame size: new tables (nothing in flight may still read the old ones)
        RR_HIP(hipDeviceSynchronize());
        ctx->screen_w = ctx->screen_h = 0;
        RR_HIP(ctx->d_screen.alloc((size_t)width + height));
        RR_HIP(launch_screen_tables(ctx->d_screen.get(), width, height, ctx->stream));
        RR_HIP(hipStreamSynchronize(ctx->stream));
        ctx->screen_w = width; ctx->screen_h = height;
    }
    return RR_OK;
}

// the tiles of the rectangle x0, y0, w, h (tile units) come first in launch order (DispatchDev::rt_*)
void set_rect_tiles(DispatchDev& a, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
    a.rt_x0 = x0; a.rt_y0 = y0; a.rt_w = w; a.rt_h = h;
    a.rt_div_w = (uint32_t)(0x100000000ull / w) + 1u;
    a.rt_div_o = a.tiles_x > w ? (uint32_t)(0x100000000ull / (a.tiles_x - w)) + 1u : 0u;
}

// DispatchRays(W, H, depth): slice f uses the constants d_cams[f] and writes to out + f * stride
DispatchDev make_dispatch(const rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth, const CamDev* d_cams,
                          const rr_scene_constants* h_cams, const rr_dispatch_params& p, uint32_t* ext_tiles, const MeshOut* mesh,
                          const Layout& o)
{
    DispatchDev a;
    memset(&a, 0, sizeof a);
    a.sx = ctx->d_screen.get(); a.sy = ctx->d_screen.get() + width;
    a.async_leaf_num = ctx->dbg_async[0]; a.async_shade_num = ctx->dbg_async[1];
    a.group_trace = ctx->dbg_group_trace ? 1u : 0u;
    uint32_t hr[4];     // where the scene can be seen at all in these slices
    (void)rr_host_screen_rect(ctx->scene_bounds, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) ? nullptr : h_cams, depth, width, height, hr);
    a.hx0 = hr[0]; a.hy0 = hr[1]; a.hx1 = hr[2]; a.hy1 = hr[3];
    a.W = width; a.H = height; a.tiles_x = o.tiles_x; a.n_tiles = o.n_tiles;
    if (mesh) {
        a.mesh_part = 1u; a.n_mesh_local = o.n_mesh_local; a.n_rect_tiles = o.part.n_mesh_tiles; a.mesh_rounds = o.part.rank0_rounds;
        a.out_bg = mesh->bg; a.bg_stride = mesh->bg_stride_elems;
        if (o.part.rect_w) set_rect_tiles(a, o.part.rect_x0, o.part.rect_y0, o.part.rect_w, o.part.rect_h);
    } else if (ctx->dbg_tile_order && ctx->tile_world == 1 && o.n_tiles < 65536u && a.hx1 > a.hx0 && a.hy1 > a.hy0) {
        // unsharded frames: the tiles that touch the rectangle are rendered first
        const uint32_t tiles_y = (height + TILE - 1) / TILE;
        const uint32_t x0 = a.hx0 / TILE, y0 = a.hy0 / TILE;
        const uint32_t x1 = std::min(o.tiles_x, (a.hx1 + TILE - 1) / TILE), y1 = std::min(tiles_y, (a.hy1 + TILE - 1) / TILE);
        if (x1 > x0 && y1 > y0 && (x1 - x0) * (y1 - y0) < o.n_tiles) set_rect_tiles(a, x0, y0, x1 - x0, y1 - y0);
    }
    a.cams = d_cams; a.n_frames = depth;
    a.blocks_per_frame = ((o.local + 7u) & ~7u) * 4u;
    a.frame_stride = o.stride;
    a.tile_rank = ctx->tile_rank; a.tile_world = ctx->tile_world; a.n_local_tiles = o.local;
    a.n_blocks = a.blocks_per_frame * depth;
    a.compact_out = o.compact ? (o.rgb8 ? 2u : 1u) : 0u;
    a.tonemap = (p.flags & RR_DISPATCH_TONEMAP_REINHARD) ? 1u : 0u;
    a.max_refract = p.max_refract; a.max_reflect = p.max_reflect;
    a.ior = p.ior; a.inv_ior = 1.0f / p.ior;
    a.tmin_p = p.tmin_primary; a.tmax_p = p.tmax_primary; a.tmin_s = p.tmin_secondary; a.tmax_s = p.tmax_secondary;
    a.out_rgba8 = ext_tiles ? ext_tiles : ctx->d_rgba8.get() + o.out_base;
    a.out_f32 = o.want_f32 ? ctx->d_f32.get() + o.out_base : nullptr;
    a.counters = ctx->d_cnt.get()->counters; a.ray_shards = ctx->d_cnt.get()->shards; a.error_flag = &ctx->d_cnt.get()->error;
    return a;
}

// one render launch of a dispatch: what the kernels read, and what their host sides need besides
struct Launch {
    SceneDev sc;
    DispatchDev a;
    uint32_t need;
    const rr_scene_constants* h_cams; const rr_dispatch_params* p;      // (h_cams may be null: no ordering hint)
    FusedVariant fused;
};

// k_render_lds parks reflected rays in a slab per stream slot (allocated at first use: outside anything that is timed)
int ensure_lds_park(rr_context* ctx, uint32_t slot, int max_reflect)
{
    const size_t park_need = (size_t)ctx->n_cus * 32 * (max_reflect <= 2 ? 2u : 8u) * 8 * 64;     // words: at most 32 waves per CU
    return ctx->d_park[slot].size() < park_need ? ctx->d_park[slot].grow(ctx, park_need) : RR_OK;
}

// k_render_lds: the reference's scene with a node array small enough for LDS (its own meshes up to shell.obj): persistent
// workgroups, nodes read from LDS
int launch_lds(rr_context* ctx, const Launch& L, bool stats)
{
    const MeshRes& m0 = ctx->meshes[(size_t)ctx->inst_host[0].blas];
    LdsDispatch q;
    memset(&q, 0, sizeof q);
    const uint32_t slot = stream_slot(ctx);
    q.tickets = ctx->d_tickets.get() + (size_t)slot * LDS_TICKET_WORDS;
    q.park_slots = L.p->max_reflect <= 2 ? 2u : 8u;
    if (int r = ensure_lds_park(ctx, slot, L.p->max_reflect)) return r;
    q.park = ctx->d_park[slot].get();
    uint32_t rect[4];
    (void)rr_host_screen_rect(m0.bounds, ((ctx->dbg_ticket_blocks & 3) == 1 || (L.p->flags & RR_DISPATCH_DEBUG_NO_CULL)) ? nullptr : L.h_cams, L.a.n_frames,
                     L.a.W, L.a.H, rect);
    // experiments (RR_DEBUG_TICKET): low bits 1 = whole frame in phase 1, 2 = no phase 1, 3 = phase 1 at every depth;
    // +16: eight queues, a wave starts on its XCD's; +32: parked rays in registers
    if ((ctx->dbg_ticket_blocks & 3) == 2) rect[2] = rect[0];
    // eight queues, a wave starts on its XCD's: an XCD then works on every eighth slice, which its L2 rewards
    // (monkey.obj Depth 64: 90 us per frame, 104 with 32 queues entered by wave number)
    q.n_queues = (ctx->dbg_ticket_blocks & 64) ? 64u : (ctx->dbg_ticket_blocks & 128) ? LDS_QUEUES : 8u;   // launch_render_lds caps it at the grid size
    q.home_xcc = (ctx->dbg_ticket_blocks & 16) ? 0u : 1u;
    q.rx0 = rect[0]; q.ry0 = rect[1]; q.rx1 = rect[2]; q.ry1 = rect[3];
    q.node_bytes = lds_node_bytes(m0);
    q.stack_entries = L.need + 1;                     // the tree's depth bounds the stack; one entry to spare
    RR_HIP(launch_render_lds(L.sc, L.a, q, ctx->n_cus, stats, ctx->stream, ctx->dbg_shape));
    return RR_OK;
}

int launch_kernel(rr_context* ctx, const Launch& L, int kernel, bool stats)
{
    if (kernel == K_STREAM) return render_stream(ctx, L.sc, L.a, L.a.n_frames, (int)L.need, stats);
    if (kernel == K_LDS) return launch_lds(ctx, L, stats);
    if (kernel == K_PATHS) RR_HIP(launch_render_paths(L.sc, L.a, (int)L.need, stats, ctx->stream));
    else RR_HIP(launch_render_fused(L.sc, L.a, L.fused.stack, L.fused.pend, stats, ctx->stream, L.fused.stack16));
    return RR_OK;
}

// A kernel-choice measurement: both candidates render the dispatch into a counter block of their own (the dispatch's are the
// caller's), after the other lanes' launches (they would be timed along); A once untimed (clocks come back), then A and B timed.
int time_candidates(rr_context* ctx, Launch L, int cand_a, int cand_b, float ms[2])
{
    if (cand_b == K_STREAM) if (int r = ensure_stream_buffers(ctx, stream_plan(ctx, L.a, L.a.n_frames))) return r;
    if (cand_a == K_LDS || cand_b == K_LDS) if (int r = ensure_lds_park(ctx, stream_slot(ctx), L.p->max_reflect)) return r;
    for (Event& e : ctx->ch_ev) if (!e.get()) RR_HIP(e.create(hipEventDefault));
    if (!ctx->d_cnt_trial.get()) RR_HIP(ctx->d_cnt_trial.alloc(1));
    RR_HIP(hipDeviceSynchronize());
    RR_HIP(hipMemsetAsync(ctx->d_cnt_trial.get(), 0, sizeof(CounterBlock), ctx->stream));
    L.a.counters = ctx->d_cnt_trial.get()->counters; L.a.ray_shards = ctx->d_cnt_trial.get()->shards; L.a.error_flag = &ctx->d_cnt_trial.get()->error;
    if (int r = launch_kernel(ctx, L, cand_a, false)) return r;
    for (int c = 0; c < 2; ++c) {
        RR_HIP(hipEventRecord(ctx->ch_ev[2 * c].get(), ctx->stream));
        if (int r = launch_kernel(ctx, L, c == 0 ? cand_a : cand_b, false)) return r;
        RR_HIP(hipEventRecord(ctx->ch_ev[2 * c + 1].get(), ctx->stream));
    }
    RR_HIP(hipEventSynchronize(ctx->ch_ev[3].get()));
    RR_HIP(hipEventElapsedTime(&ms[0], ctx->ch_ev[0].get(), ctx->ch_ev[1].get()));
    RR_HIP(hipEventElapsedTime(&ms[1], ctx->ch_ev[2].get(), ctx->ch_ev[3].get()));
    return RR_OK;
}

// the kernel that renders the launch: forced by RR_DEBUG_KERNEL, or its class's measured choice (measured now if that is due)
int choose_kernel(rr_context* ctx, const Launch& L, const KernelPick& pk, const LaunchFacts& lf, int& kernel)
{
    kernel = pk.kernel;
    if (pk.cls == CLS_NONE) return RR_OK;
    KernelChoice* const ch = ctx->ch[pk.cls].find(choice_key(L.a.W, L.a.H, *L.p, L.a.n_frames));
    if (measure_due(*ch, lf.rect_share, lf.no_cull)) {
        float ms[2] = { 0.0f, 0.0f };
        if (int r = time_candidates(ctx, L, pk.cand_a, pk.cand_b, ms)) return r;
        record_timings(*ch, ms[0], ms[1], lf.rect_share);
        if (getenv("RR_DEBUG_CHOICE"))
            fprintf(stderr, "[rr] kernel choice: depth %u candidate %d: default %.3f ms, candidate %.3f ms (%.3f)%s\n", L.a.n_frames, pk.cand_b, ms[0], ms[1],
                    ms[1] / ms[0], ch->choice == 2 ? " -> candidate" : ch->choice == 1 ? " -> default" : " (once more)");
    }
    kernel = chosen_kernel(pk, ch, lf.rect_share);
    return RR_OK;
}

// out_slot: which of the frames_in_flight output regions of the internal frame buffer this dispatch writes;
// h_cams: host copy of the depth slices' constants (may be null: no ordering hint)
int dispatch_impl(rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth, const CamDev* d_cams,
                  const rr_scene_constants* h_cams, const rr_dispatch_params& p, uint32_t* ext_tiles, size_t ext_stride_elems,
                  bool keep_counters, uint32_t out_slot = 0, uint32_t out_slot_depth = 0, const MeshOut* mesh = nullptr)
{
    Layout o;
    if (int r = layout_dispatch(ctx, width, height, depth, h_cams, p, ext_tiles, ext_stride_elems, out_slot, out_slot_depth, mesh, o)) return r;
    Launch L;
    fill_scene(ctx, L.sc);
    L.a = make_dispatch(ctx, width, height, depth, d_cams, h_cams, p, ext_tiles, mesh, o);
    L.need = scene_stack_need(ctx); L.h_cams = h_cams; L.p = &p;

    DevBuf<unsigned long long> d_diag;          // RR_DEBUG_DIAG: per-wave records of the launch
    const size_t diag_waves = std::max<size_t>(((size_t)L.a.n_blocks + (size_t)((L.a.hx1 - L.a.hx0) / 8u + 1u) * ((L.a.hy1 - L.a.hy0) / 8u + 1u) * depth) * 4 * 2, (size_t)ctx->n_cus * 32);
    if (!ctx->dbg_diag.empty() && ctx->single_identity) {
        RR_HIP(d_diag.alloc(diag_waves * 8));
        RR_HIP(hipMemsetAsync(d_diag.get(), 0, diag_waves * 64, ctx->stream));
        L.a.diag = d_diag.get();
    }
    const uint32_t filled = mesh ? o.n_mesh_local : o.local;       // slots of the (gathered) tile buffer this rank writes
    const size_t tile_bytes = (size_t)TILE * TILE * (o.rgb8 ? 3 : 4);
    if (o.compact && filled < o.max_local)           // keep the gathered tail deterministic
        for (uint32_t f = 0; f < depth; ++f)
            RR_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(L.a.out_rgba8 + f * o.stride) + filled * tile_bytes, 0, (o.max_local - filled) * tile_bytes, ctx->stream));

    const SceneFacts sf = scene_facts(ctx);
    const uint32_t rect[4] = { L.a.hx0, L.a.hy0, L.a.hx1, L.a.hy1 };
    const LaunchFacts lf = launch_facts(ctx, width, height, depth, rect, p, o.compact, mesh != nullptr);
    L.fused = fused_variant(sf, depth, p.max_reflect, ctx->dbg);
    int kernel = K_FUSED;
    if (int r = choose_kernel(ctx, L, pick_kernel(sf, lf, ctx->dbg), lf, kernel)) return r;

    const bool stats = (p.flags & RR_DISPATCH_COLLECT_STATS) != 0;
    const bool keep = keep_counters || (p.flags & RR_DISPATCH_KEEP_COUNTERS) != 0;
    if (!keep) RR_HIP(hipMemsetAsync(ctx->d_cnt.get(), 0, sizeof(CounterBlock), ctx->stream));
    const bool timed = (p.flags & RR_DISPATCH_TIME_KERNEL) != 0;      // between a pair of rr_kernel_time events
    if (timed) {
        if (ctx->kev_used >= 4096) return fail(ctx, RR_ERR_STATE, "dispatch: 4096 timed dispatches pending, call rr_kernel_time");
        for (Event e; ctx->kev.size() < (size_t)(ctx->kev_used + 1) * 2; ctx->kev.push_back(std::move(e))) RR_HIP(e.create(hipEventDefault));
        RR_HIP(hipEventRecord(ctx->kev[(size_t)ctx->kev_used * 2].get(), ctx->stream));
    }
    if (int r = launch_kernel(ctx, L, kernel, stats)) return r;
    if (timed) { RR_HIP(hipEventRecord(ctx->kev[(size_t)ctx->kev_used * 2 + 1].get(), ctx->stream)); ++ctx->kev_used; }
    if (d_diag.get()) {       // experiments only: dump per-wave {start, cycles, max rays per lane, loop trips}
        std::vector<unsigned long long> h(diag_waves * 8);
        RR_HIP(hipStreamSynchronize(ctx->stream));
        RR_HIP(hipMemcpy(h.data(), d_diag.get(), h.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(ctx->dbg_diag.c_str(), "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    }

    snprintf(ctx->last_kernel_name, sizeof ctx->last_kernel_name, "%s", kernel == K_STREAM ? last_stream_kernel_name() : last_render_kernel_name());
    ctx->last_kernel = (uint32_t)kernel;
    ctx->W = width; ctx->H = height; ctx->frame_world = ctx->tile_world; ctx->frame_depth = depth;
    ctx->have_f32 = o.want_f32; ctx->have_frame = ext_tiles == nullptr; ctx->have_assembled = false;
    if (!ext_tiles) ctx->frame_base = o.out_base;
    ctx->last_stats = stats;
    ctx->last_pixels = owned_pixels(width, height, ctx->tile_rank, ctx->tile_world, mesh ? &o.part : nullptr) * depth;
    ctx->accum_pixels = (keep ? ctx->accum_pixels : 0) + ctx->last_pixels;
    return RR_OK;
}

int upload_cams(rr_context* ctx, const rr_scene_constants* c, size_t n)
{
    static_assert(sizeof(CamDev) == sizeof(rr_scene_constants), "constant buffer layout");
    if (int r = ensure_cams(ctx, n)) return r;
    const int slot = (int)(ctx->h_cams_next++ % rr_context::CAM_SLOTS);
    if (ctx->h_cams_busy[slot]) { RR_HIP(hipEventSynchronize(ctx->h_cams_ev[slot].get())); ctx->h_cams_busy[slot] = false; }
    if (ctx->h_cams[slot].size() < n) RR_HIP(ctx->h_cams[slot].alloc(n < 64 ? 64 : n));
    if (!ctx->h_cams_ev[slot].get()) RR_HIP(ctx->h_cams_ev[slot].create(hipEventDisableTiming));
    memcpy(ctx->h_cams[slot].get(), c, n * sizeof(CamDev));
    RR_HIP(hipMemcpyAsync(ctx->d_cams.get(), ctx->h_cams[slot].get(), n * sizeof(CamDev), hipMemcpyHostToDevice, ctx->stream));   // copy_to_buffer, :566
    RR_HIP(hipEventRecord(ctx->h_cams_ev[slot].get(), ctx->stream));
    ctx->h_cams_busy[slot] = true;
    return RR_OK;
}

rr_dispatch_params params_or_default(const rr_dispatch_params* params)
{
    rr_dispatch_params p;
    return params ? *params : (rr_default_dispatch_params(&p), p);
}

// waits for the context's stream, then reads the device error flag of what it rendered
int check_error_flag(rr_context* ctx, const char* what)
{
    RR_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t err = 0;
    RR_HIP(hipMemcpy(&err, &ctx->d_cnt.get()->error, 4, hipMemcpyDeviceToHost));
    return err ? fail(ctx, RR_ERR_TRAVERSAL_OVERFLOW, what) : RR_OK;
}

// drawFrame loop: camera constants for n consecutive orbit angles (RefractionDemo.cpp:559-565), the angle advanced past them (:567)
int orbit_cams(rr_context* ctx, const char* what, float& angle, float angle_step, uint32_t n, float fov_y, float aspect, float zn, float zf,
               std::vector<rr_scene_constants>& cams)
{
    cams.resize(n);
    for (uint32_t k = 0; k < n; ++k, angle += angle_step)
        if (int rc = rr_host_camera_orbit(angle, fov_y, aspect, zn, zf, &cams[k])) return fail(ctx, rc, what);
    return RR_OK;
}

// zero the counters where every lane will see it (before the fork); the launches then keep adding to them
int zero_counters_before_fork(rr_context* ctx, rr_dispatch_params& p)
{
    if (p.flags & RR_DISPATCH_KEEP_COUNTERS) return RR_OK;
    RR_HIP(hipMemsetAsync(ctx->d_cnt.get(), 0, sizeof(CounterBlock), ctx->stream));
    ctx->accum_pixels = 0; p.flags |= RR_DISPATCH_KEEP_COUNTERS;
    return RR_OK;
}

// the lane starts after everything submitted to the context's stream so far
int fork_lane(rr_context* ctx, uint32_t lane)
{
    RR_HIP(hipEventRecord(ctx->lane_fork[lane].get(), ctx->stream));
    RR_HIP(hipStreamWaitEvent(ctx->lane_stream[lane].get(), ctx->lane_fork[lane].get(), 0));
    return RR_OK;
}

// Launches on a forked lane (rr_render_orbit_sharded_lane): while the scope lasts, the lane's stream and constant buffer are
// the context's (no reuse race between lanes; a lane is one stream, its launches stay in order)
struct LaneScope {
    rr_context* const ctx;
    const uint32_t lane;
    const hipStream_t stream; const uint32_t in_flight;
    LaneScope(rr_context* c, uint32_t l) : ctx(c), lane(l), stream(c->stream), in_flight(c->frames_in_flight)
    {
        ctx->stream = ctx->lane_stream[lane].get(); std::swap(ctx->d_cams, ctx->lane_cams[lane]);
        ctx->frames_in_flight = 1;
    }
    ~LaneScope() { std::swap(ctx->d_cams, ctx->lane_cams[lane]); ctx->stream = stream; ctx->frames_in_flight = in_flight; }
    int done(int rc, const char* what)      // the lane's end, behind what `rc` reports on
    {
        if (rc != RR_OK) return rc;
        if (hipError_t e = hipEventRecord(ctx->lane_done[lane].get(), ctx->stream)) return fail(ctx, RR_ERR_DEVICE, what, e);
        ctx->lane_busy[lane] = true;
        return RR_OK;
    }
};

} // namespace

int rr_dispatch_rays(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params)
{
    const Range range_("rr_dispatch_rays");
    if (int r = use_device(ctx)) return r;
    if (!ctx->cam_set) return fail(ctx, RR_ERR_STATE, "rr_dispatch_rays: rr_set_camera first");
    rr_dispatch_params p = params_or_default(params);
    if (int r = upload_cams(ctx, &ctx->cam, 1)) return r;
    return dispatch_impl(ctx, width, height, 1, ctx->d_cams.get(), &ctx->cam, p, nullptr, 0, false);
}

int rr_dispatch_rays_batch(rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth,
                           const rr_scene_constants* constants, const rr_dispatch_params* params)
{
    if (int r = use_device(ctx)) return r;
    if (!constants || depth == 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_dispatch_rays_batch: need depth >= 1 constants");
    rr_dispatch_params p = params_or_default(params);
    if (int r = upload_cams(ctx, constants, depth)) return r;
    return dispatch_impl(ctx, width, height, depth, ctx->d_cams.get(), constants, p, nullptr, 0, false);
}

int rr_read_frame_slice(rr_context* ctx, uint32_t slice, uint8_t* rgba8, float* rgba32f)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->have_frame) return fail(ctx, RR_ERR_STATE, "rr_read_frame: nothing dispatched");
    const size_t n = (size_t)ctx->W * ctx->H;
    if (ctx->have_assembled) {
        if (rgba32f || slice) return fail(ctx, RR_ERR_STATE, "rr_read_frame: only slice 0 / RGBA8 of an assembled frame");
        if (rgba8) RR_HIP(hipMemcpyAsync(rgba8, ctx->d_assembled.get(), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        if (ctx->frame_world != 1) return fail(ctx, RR_ERR_STATE, "rr_read_frame: sharded frame, gather + rr_assemble_tiles first");
        if (slice >= ctx->frame_depth) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_read_frame: slice beyond the dispatch depth");
        if (rgba32f && !ctx->have_f32) return fail(ctx, RR_ERR_STATE, "rr_read_frame: dispatch with RR_DISPATCH_FLOAT_OUTPUT");
        if (rgba8) RR_HIP(hipMemcpyAsync(rgba8, ctx->d_rgba8.get() + ctx->frame_base + slice * n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (rgba32f) RR_HIP(hipMemcpyAsync(rgba32f, ctx->d_f32.get() + ctx->frame_base + slice * n, n * 16, hipMemcpyDeviceToHost, ctx->stream));
    }
    return check_error_flag(ctx, "traversal stack overflow: frame invalid");
}

int rr_read_frame(rr_context* ctx, uint8_t* rgba8, float* rgba32f) { return rr_read_frame_slice(ctx, 0, rgba8, rgba32f); }

int rr_export_tiles(rr_context* ctx, void* d_dst)
{
    if (int r = use_device(ctx)) return r;
    if (!d_dst) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_export_tiles: null destination");
    if (!ctx->have_frame || ctx->frame_world < 2) return fail(ctx, RR_ERR_STATE, "rr_export_tiles: no sharded frame");
    const Tiles t = tile_counts(ctx->W, ctx->H, ctx->tile_rank, ctx->frame_world);
    RR_HIP(hipMemcpyAsync(d_dst, ctx->d_rgba8.get() + ctx->frame_base, (size_t)t.max_local * TILE * TILE * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return RR_OK;
}

int rr_assemble_tiles(rr_context* ctx, const void* d_gathered, uint32_t world, void* d_frame)
{
    if (int r = use_device(ctx)) return r;
    if (!d_gathered || world == 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_tiles: bad arguments");
    if (!ctx->have_frame || ctx->W == 0) return fail(ctx, RR_ERR_STATE, "rr_assemble_tiles: dispatch first (frame size)");
    const Tiles t = tile_counts(ctx->W, ctx->H, 0, world);
    uint32_t* dst = (uint32_t*)d_frame;
    if (!dst) {
        const size_t n = (size_t)ctx->W * ctx->H;
        if (n > ctx->d_assembled.size())
            if (int r = ctx->d_assembled.grow(ctx, n)) return r;
        dst = ctx->d_assembled.get();
    }
    RR_HIP(launch_assemble_tiles((const uint32_t*)d_gathered, dst, ctx->W, ctx->H, t.tiles_x, t.n_tiles, world, t.max_local, ctx->stream));
    if (!d_frame) ctx->have_assembled = true;
    return RR_OK;
}

namespace {

// drawFrame loop: camera constants for n_frames consecutive orbit angles go to the device constant
// buffer in one copy; the frames are then dispatched in batches of `batch` depth slices.
int orbit_impl(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
               float angle_step, uint32_t n_frames, uint32_t batch, float fov_y, float aspect, float zn, float zf,
               uint32_t* ext_tiles, size_t ext_stride_elems, uint8_t* host_out = nullptr)
{
    const Range range_("rr_render_orbit");
    if (!angle) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "render_orbit: null angle");
    if (n_frames == 0) return RR_OK;
    if (batch == 0) batch = 1;
    rr_dispatch_params p = params_or_default(params);
    std::vector<rr_scene_constants> cams;
    if (int r = orbit_cams(ctx, "render_orbit: camera", *angle, angle_step, n_frames, fov_y, aspect, zn, zf, cams)) return r;
    ctx->cam = cams.back(); ctx->cam_set = true;
    if (int r = upload_cams(ctx, cams.data(), n_frames)) return r;
    const bool keep_first = (p.flags & RR_DISPATCH_KEEP_COUNTERS) != 0;
    const uint32_t n_batches = (n_frames + batch - 1) / batch;
    // frames in flight: consecutive launches go to alternating lanes so that the long-running waves at the end of
    // one overlap the start of the next.  Not for timed dispatches (their durations must be exclusive).
    uint32_t lanes = ctx->frames_in_flight < n_batches ? ctx->frames_in_flight : n_batches;
    if ((p.flags & RR_DISPATCH_TIME_KERNEL) || !ctx->dbg_diag.empty()) lanes = 1;
    // k_render_lds is persistent -- its workgroups hold every CU until the launch is over --, so two of its launches in flight only
    // get in each other's way (sphere.obj Depth 64: 145 us per frame one at a time, 167 with two in flight).  Does it render the
    // first launch?  (As dispatch_impl would pick it, changing no choice.)
    bool one_kernel_at_a_time = false;
    if (ctx->tlas_built && width && height) {
        const uint32_t d = batch < n_frames ? batch : n_frames;
        uint32_t rect[4];
        (void)rr_host_screen_rect(ctx->scene_bounds, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) ? nullptr : cams.data(), d, width, height, rect);
        const LaunchFacts lf = launch_facts(ctx, width, height, d, rect, p, ctx->tile_world > 1 || ext_tiles, false);
        const KernelPick pk = pick_kernel(scene_facts(ctx), lf, ctx->dbg);
        const KernelChoice* ch = pk.cls == CLS_NONE ? nullptr : ctx->ch[pk.cls].peek(choice_key(width, height, p, d));
        one_kernel_at_a_time = chosen_kernel(pk, ch, lf.rect_share) == K_LDS;
        if (lanes > 1 && one_kernel_at_a_time) lanes = 1;
    }
    if (host_out) {          // streaming to host: the copy of one region overlaps the rendering of the other
        if (ext_tiles || ctx->tile_world != 1 || (p.flags & RR_DISPATCH_FLOAT_OUTPUT))
            return fail(ctx, RR_ERR_UNSUPPORTED, "render_orbit_to_host: whole RGBA8 frames of an unsharded context only");
        lanes = ctx->frames_in_flight > 2 ? ctx->frames_in_flight : 2;
    }
    if (lanes <= 1) {
        for (uint32_t k = 0; k < n_frames; k += batch) {
            const uint32_t d = n_frames - k < batch ? n_frames - k : batch;
            uint32_t* ext = ext_tiles ? ext_tiles + (size_t)k * ext_stride_elems : nullptr;
            if (int rc = dispatch_impl(ctx, width, height, d, ctx->d_cams.get() + k, cams.data() + k, p, ext, ext_stride_elems, k > 0 || keep_first)) return rc;
        }
        return RR_OK;
    }
    if (!ext_tiles) {        // all output regions exist before anything overlaps
        if (width == 0 || height == 0 || width > 32768 || height > 32768) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "dispatch: bad frame size or depth");
        const Tiles t = tile_counts(width, height, ctx->tile_rank, ctx->tile_world);
        const size_t slice_elems = ctx->tile_world > 1 ? (size_t)t.max_local * TILE * TILE : (size_t)width * height;
        if (int r = ensure_frame_buffers(ctx, slice_elems * batch * lanes, (p.flags & RR_DISPATCH_FLOAT_OUTPUT) != 0)) return r;
    }
    if (int r = zero_counters_before_fork(ctx, p)) return r;
    for (uint32_t l = 0; l < lanes; ++l) {
        if (int r = ensure_lane(ctx, l)) return r;
        if (ctx->lane_busy[l]) { RR_HIP(hipStreamWaitEvent(ctx->stream, ctx->lane_done[l].get(), 0)); ctx->lane_busy[l] = false; }
    }
    RR_HIP(hipEventRecord(ctx->lane_fork[0].get(), ctx->stream));          // after the constants upload and the counter reset
    for (uint32_t l = 0; l < lanes; ++l) RR_HIP(hipStreamWaitEvent(ctx->lane_stream[l].get(), ctx->lane_fork[0].get(), 0));
    hipStream_t main_stream = ctx->stream;
    int rc = RR_OK;
    for (uint32_t k = 0, b = 0; k < n_frames && rc == RR_OK; k += batch, ++b) {
        const uint32_t d = n_frames - k < batch ? n_frames - k : batch;
        uint32_t* ext = ext_tiles ? ext_tiles + (size_t)k * ext_stride_elems : nullptr;
        ctx->stream = ctx->lane_stream[b % lanes].get();
        // (streaming to host keeps two regions for the copies' sake; the persistent kernel's launches still go one after the other)
        if (one_kernel_at_a_time && b > 0 && hipStreamWaitEvent(ctx->stream, ctx->lane_fork[(b - 1) % lanes].get(), 0) != hipSuccess)
            rc = fail(ctx, RR_ERR_DEVICE, "render_orbit: lane order");
        if (rc == RR_OK) rc = dispatch_impl(ctx, width, height, d, ctx->d_cams.get() + k, cams.data() + k, p, ext, ext_stride_elems, true, b % lanes, batch);
        if (rc == RR_OK && one_kernel_at_a_time && hipEventRecord(ctx->lane_fork[b % lanes].get(), ctx->stream) != hipSuccess)
            rc = fail(ctx, RR_ERR_DEVICE, "render_orbit: lane order");
        if (rc == RR_OK && host_out) {      // same lane: the region is not rendered into again before this copy is done
            const size_t fb = (size_t)width * height * 4;
            hipError_t e = hipMemcpyAsync(host_out + (size_t)k * fb, ctx->d_rgba8.get() + ctx->frame_base, (size_t)d * fb, hipMemcpyDeviceToHost, ctx->stream);
            if (e != hipSuccess) rc = fail(ctx, RR_ERR_DEVICE, "render_orbit_to_host: copy", e);
        }
        ctx->stream = main_stream;
    }
    for (uint32_t l = 0; l < lanes; ++l) {                          // join: the caller's stream is ordered after every lane
        hipError_t e = hipEventRecord(ctx->lane_done[l].get(), ctx->lane_stream[l].get());
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->lane_done[l].get(), 0);
        if (e != hipSuccess && rc == RR_OK) rc = fail(ctx, RR_ERR_DEVICE, "render_orbit: lane join", e);
    }
    return rc;
}

} // namespace

int rr_render_orbit(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                    float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch, float fov_y, float aspect, float zn,
                    float zf)
{
    if (int r = use_device(ctx)) return r;
    return orbit_impl(ctx, width, height, params, angle, angle_step, n_frames, frames_per_dispatch, fov_y, aspect, zn, zf,
                      nullptr, 0);
}

int rr_render_orbit_to_host(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                            float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch, float fov_y, float aspect, float zn,
                            float zf, uint8_t* host_rgba8)
{
    if (int r = use_device(ctx)) return r;
    if (!host_rgba8) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_to_host: null host buffer");
    if (int r = orbit_impl(ctx, width, height, params, angle, angle_step, n_frames, frames_per_dispatch, fov_y, aspect, zn, zf,
                           nullptr, 0, host_rgba8)) return r;
    return check_error_flag(ctx, "device error flag set: frames invalid");          // every frame is in host memory on return
}

int rr_render_orbit_sharded(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                            float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch, float fov_y, float aspect,
                            float zn, float zf, void* d_tiles, uint64_t frame_stride_bytes)
{
    if (int r = use_device(ctx)) return r;
    if (!d_tiles) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_sharded: null tile buffer");
    const Tiles t = tile_counts(width ? width : 1, height ? height : 1, ctx->tile_rank, ctx->tile_world);
    const uint64_t bpp = (params && (params->flags & RR_DISPATCH_TILES_RGB8)) ? 3 : 4;
    if (frame_stride_bytes < (uint64_t)t.max_local * TILE * TILE * bpp || (frame_stride_bytes & 3u))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_sharded: frame stride smaller than a tile buffer");
    return orbit_impl(ctx, width, height, params, angle, angle_step, n_frames, frames_per_dispatch, fov_y, aspect, zn, zf,
                      (uint32_t*)d_tiles, (size_t)(frame_stride_bytes / 4));
}

int rr_render_orbit_sharded_lane(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                                 float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch, float fov_y, float aspect,
                                 float zn, float zf, void* d_tiles, uint64_t frame_stride_bytes, uint32_t lane)
{
    if (int r = use_device(ctx)) return r;
    if (lane >= rr_context::MAX_LANES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_sharded_lane: lane out of range");
    if (int r = ensure_lane(ctx, lane)) return r;
    rr_dispatch_params p = params_or_default(params);
    if (int r = zero_counters_before_fork(ctx, p)) return r;
    if (int r = fork_lane(ctx, lane)) return r;
    LaneScope scope(ctx, lane);
    return scope.done(rr_render_orbit_sharded(ctx, width, height, &p, angle, angle_step, n_frames, frames_per_dispatch, fov_y, aspect, zn,
                                               zf, d_tiles, frame_stride_bytes), "rr_render_orbit_sharded_lane: event");
}

int rr_mesh_partition_for_orbit(rr_context* ctx, uint32_t width, uint32_t height, float angle, float angle_step, uint32_t n_frames,
                                float fov_y, float aspect, float zn, float zf, rr_mesh_partition* out)
{
    if (!ctx || !out || n_frames == 0) return RR_ERR_INVALID_ARGUMENT;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_mesh_partition_for_orbit: build the BLAS and TLAS first");
    std::vector<rr_scene_constants> cams;
    if (int r = orbit_cams(ctx, "rr_mesh_partition_for_orbit: camera", angle, angle_step, n_frames, fov_y, aspect, zn, zf, cams)) return r;
    return rr_host_mesh_partition(ctx->scene_bounds, cams.data(), n_frames, width, height, ctx->tile_world, out);
}

int rr_render_orbit_mesh_sharded_lane(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                                      float angle_step, uint32_t n_frames, float fov_y, float aspect, float zn, float zf, void* d_mesh_tiles,
                                      uint64_t mesh_stride_bytes, void* d_bg_tiles, uint64_t bg_stride_bytes, uint32_t lane)
{
    const Range range_("rr_render_orbit_mesh_sharded");
    if (int r = use_device(ctx)) return r;
    if (lane >= rr_context::MAX_LANES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_mesh_sharded_lane: lane out of range");
    if (!angle || !d_mesh_tiles || n_frames == 0 || (mesh_stride_bytes & 3u) || (bg_stride_bytes & 3u))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_mesh_sharded_lane: bad arguments");
    if (int r = ensure_lane(ctx, lane)) return r;
    rr_dispatch_params p = params_or_default(params);
    p.flags |= RR_DISPATCH_TILES_RGB8;
    std::vector<rr_scene_constants> cams;
    if (int r = orbit_cams(ctx, "render_orbit: camera", *angle, angle_step, n_frames, fov_y, aspect, zn, zf, cams)) return r;
    // the one partition of this launch: its buffers are checked against it and the kernel renders it (DEBUG_NO_CULL: the whole
    // frame is mesh tiles, as rr_host_mesh_partition(bounds, NULL, ...) says)
    rr_mesh_partition part;
    if (rr_host_mesh_partition(ctx->scene_bounds, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) ? nullptr : cams.data(), n_frames, width, height,
                               ctx->tile_world, &part) != RR_OK)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "mesh partition");
    if (mesh_stride_bytes < (uint64_t)part.max_mesh_tiles_per_rank * TILE * TILE * 3 ||
        (ctx->tile_rank == 0 && part.n_bg_tiles && (!d_bg_tiles || bg_stride_bytes < (uint64_t)part.n_bg_tiles * TILE * TILE * 3)))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_mesh_sharded_lane: tile buffers smaller than rr_mesh_partition_for_orbit says");
    if (int r = zero_counters_before_fork(ctx, p)) return r;
    ctx->cam = cams.back(); ctx->cam_set = true;
    if (int r = fork_lane(ctx, lane)) return r;
    LaneScope scope(ctx, lane);
    int rc = upload_cams(ctx, cams.data(), n_frames);
    const MeshOut mo = { &part, (uint32_t*)d_bg_tiles, (size_t)(bg_stride_bytes / 4) };
    if (rc == RR_OK) rc = dispatch_impl(ctx, width, height, n_frames, ctx->d_cams.get(), cams.data(), p, (uint32_t*)d_mesh_tiles, (size_t)(mesh_stride_bytes / 4), true, 0, 0, &mo);
    return scope.done(rc, "rr_render_orbit_mesh_sharded_lane: event");
}

int rr_assemble_frames_mesh_rgb8(rr_context* ctx, const void* d_gathered, uint64_t rank_stride_bytes, uint64_t frame_stride_bytes,
                                 const void* d_bg_tiles, uint64_t bg_stride_bytes, const rr_mesh_partition* part, uint32_t n_frames,
                                 uint32_t width, uint32_t height, void* d_frames, uint64_t out_stride_bytes)
{
    const Range range_("rr_assemble_frames_mesh_rgb8");
    if (int r = use_device(ctx)) return r;
    if (!d_gathered || !d_frames || !part || part->world == 0 || width == 0 || height == 0 ||
        ((rank_stride_bytes | frame_stride_bytes | bg_stride_bytes | out_stride_bytes | (uint64_t)(uintptr_t)d_gathered | (uint64_t)(uintptr_t)d_bg_tiles) & 3u))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames_mesh_rgb8: bad arguments (strides and buffers are 4-byte aligned)");
    const uint32_t tiles_x = (width + TILE - 1) / TILE, n_tiles = tiles_x * ((height + TILE - 1) / TILE);
    if (part->tiles_x != tiles_x || part->n_tiles != n_tiles || part->n_mesh_tiles + part->n_bg_tiles != n_tiles ||
        (part->rect_w == 0 ? part->n_bg_tiles != 0 : (part->rect_w * part->rect_h != part->n_mesh_tiles || part->rect_x0 + part->rect_w > tiles_x ||
                                                      (part->rect_y0 + part->rect_h) * tiles_x > n_tiles)))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames_mesh_rgb8: the partition is not one of this frame size");
    if (frame_stride_bytes < (uint64_t)part->max_mesh_tiles_per_rank * TILE * TILE * 3 || out_stride_bytes < (uint64_t)width * height * 4 ||
        (part->n_bg_tiles && (!d_bg_tiles || bg_stride_bytes < (uint64_t)part->n_bg_tiles * TILE * TILE * 3)))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames_mesh_rgb8: stride too small");
    const MeshPartDev mp = { part->tiles_x, part->n_tiles, part->rect_x0, part->rect_y0, part->rect_w, part->rect_h, part->world, part->rank0_rounds };
    RR_HIP(launch_assemble_frames_mesh_rgb8((const uint8_t*)d_gathered, (const uint8_t*)d_bg_tiles, (uint32_t*)d_frames, width, height, mp, rank_stride_bytes,
                                            frame_stride_bytes, bg_stride_bytes, out_stride_bytes / 4, n_frames, ctx->stream));
    return RR_OK;
}

int rr_assemble_frames(rr_context* ctx, const void* d_gathered, uint32_t world, uint64_t rank_stride_bytes,
                       uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t width, uint32_t height, void* d_frames,
                       uint64_t out_stride_bytes)
{
    const Range range_("rr_assemble_frames");
    if (int r = use_device(ctx)) return r;
    if (!d_gathered || !d_frames || world == 0 || width == 0 || height == 0 || ((rank_stride_bytes | frame_stride_bytes | out_stride_bytes) & 3u))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames: bad arguments");
    const Tiles t = tile_counts(width, height, 0, world);
    if (frame_stride_bytes < (uint64_t)t.max_local * TILE * TILE * 4 || out_stride_bytes < (uint64_t)width * height * 4)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames: stride too small");
    RR_HIP(launch_assemble_frames((const uint32_t*)d_gathered, (uint32_t*)d_frames, width, height, t.tiles_x, t.n_tiles, world,
                                  rank_stride_bytes / 4, frame_stride_bytes / 4, out_stride_bytes / 4, n_frames, ctx->stream));
    return RR_OK;
}

int rr_assemble_frames_rgb8(rr_context* ctx, const void* d_gathered, uint32_t world, uint64_t rank_stride_bytes,
                            uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t width, uint32_t height, void* d_frames,
                            uint64_t out_stride_bytes)
{
    const Range range_("rr_assemble_frames_rgb8");
    if (int r = use_device(ctx)) return r;
    if (!d_gathered || !d_frames || world == 0 || width == 0 || height == 0 ||
        ((rank_stride_bytes | frame_stride_bytes | out_stride_bytes | (uint64_t)(uintptr_t)d_gathered) & 3u))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames_rgb8: bad arguments (strides and buffers are 4-byte aligned)");
    const Tiles t = tile_counts(width, height, 0, world);
    if (frame_stride_bytes < (uint64_t)t.max_local * TILE * TILE * 3 || out_stride_bytes < (uint64_t)width * height * 4)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_assemble_frames_rgb8: stride too small");
    RR_HIP(launch_assemble_frames_rgb8((const uint8_t*)d_gathered, (uint32_t*)d_frames, width, height, t.tiles_x, t.n_tiles, world,
                                       rank_stride_bytes, frame_stride_bytes, out_stride_bytes / 4, n_frames, ctx->stream));
    return RR_OK;
}

// ---- RCCL, looked up at run time ---------------------------------------------------------------------------------
namespace {
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, rr_nccl_unique_id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
    Rccl()
    {
        // a process that already holds an RCCL (PyTorch's) must use that one: two copies of its globals do not mix
        const char* names[] = { "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so" };
        for (const char* n : names) if (!lib) lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        for (const char* n : names) if (!lib) lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!lib) return;
        GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        Send = (decltype(Send))dlsym(lib, "ncclSend");
        Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        ok = GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv;
    }
};
extern "C++" const Rccl& rccl() { static const Rccl r; return r; }      // (this translation unit's tail is inside extern "C")
static_assert(sizeof(rr_nccl_unique_id) == 128, "rr_comm_unique_id hands out 128 bytes");
} // namespace

int rr_comm_unique_id(void* id128)
{
    if (!id128) return RR_ERR_INVALID_ARGUMENT;
    if (!rccl().ok) return RR_ERR_UNSUPPORTED;                    // no librccl.so on this machine
    return rccl().GetUniqueId(id128) == 0 ? RR_OK : RR_ERR_DEVICE;
}

int rr_comm_init(rr_context* ctx, const void* id128, int rank, int world, void** comm)
{
    if (int r = use_device(ctx)) return r;                        // the communicator belongs to the context's device
    if (!id128 || !comm || world < 1 || rank < 0 || rank >= world) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_comm_init: bad arguments");
    if (!rccl().ok) return fail(ctx, RR_ERR_UNSUPPORTED, "rr_comm_init: librccl.so not found");
    rr_nccl_unique_id id;
    memcpy(&id, id128, sizeof id);
    *comm = nullptr;
    const int e = rccl().CommInitRank(comm, world, id, rank);
    if (e != 0) { ctx->err = std::string("ncclCommInitRank: ") + (rccl().GetErrorString ? rccl().GetErrorString(e) : "error"); return RR_ERR_DEVICE; }
    return RR_OK;
}

int rr_comm_destroy(void* comm)
{
    if (!comm) return RR_OK;
    if (!rccl().ok) return RR_ERR_UNSUPPORTED;
    return rccl().CommDestroy(comm) == 0 ? RR_OK : RR_ERR_DEVICE;
}

int rr_gather_frames(rr_context* ctx, void* comm, int rank, int world, const void* d_send, void* d_recv, uint64_t bytes_per_rank, int root)
{
    const Range range_("rr_gather_frames");
    if (int r = use_device(ctx)) return r;
    if (!comm || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || !d_send || (rank == root && !d_recv))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_gather_frames: bad arguments");
    if (!rccl().ok) return fail(ctx, RR_ERR_UNSUPPORTED, "rr_gather_frames: librccl.so not found");
    if (bytes_per_rank == 0) return RR_OK;
    const Rccl& R = rccl();
    int e = R.GroupStart();
    if (e == 0) e = R.Send(d_send, (size_t)bytes_per_rank, (int)RR_NCCL_UINT8, root, comm, ctx->stream);
    if (rank == root)
        for (int r = 0; r < world && e == 0; ++r)
            e = R.Recv((char*)d_recv + (size_t)r * bytes_per_rank, (size_t)bytes_per_rank, (int)RR_NCCL_UINT8, r, comm, ctx->stream);
    const int e2 = R.GroupEnd();
    if (e == 0) e = e2;
    if (e != 0) { ctx->err = std::string("rr_gather_frames: ") + (R.GetErrorString ? R.GetErrorString(e) : "RCCL error"); return RR_ERR_DEVICE; }
    return RR_OK;
}

int rr_device_alloc(rr_context* ctx, uint64_t bytes, void** d_ptr)
{
    if (int r = use_device(ctx)) return r;
    if (!d_ptr || bytes == 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_device_alloc: bad arguments");
    RR_HIP(hipMalloc(d_ptr, (size_t)bytes));
    return RR_OK;
}

int rr_device_free(rr_context* ctx, void* d_ptr)
{
    if (int r = use_device(ctx)) return r;
    if (d_ptr) { RR_HIP(hipStreamSynchronize(ctx->stream)); RR_HIP(hipFree(d_ptr)); }
    return RR_OK;
}

int rr_device_read(rr_context* ctx, const void* d_src, void* host_dst, uint64_t bytes)
{
    if (int r = use_device(ctx)) return r;
    if (!d_src || !host_dst) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_device_read: null pointer");
    RR_HIP(hipMemcpyAsync(host_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    return RR_OK;
}

int rr_timing_begin(rr_context* ctx)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->ev_end.get()) { RR_HIP(ctx->ev_begin.create(hipEventDefault)); RR_HIP(ctx->ev_end.create(hipEventDefault)); }
    RR_HIP(hipEventRecord(ctx->ev_begin.get(), ctx->stream));
    return RR_OK;
}

int rr_timing_end(rr_context* ctx, float* elapsed_ms)
{
    if (int r = use_device(ctx)) return r;
    if (!elapsed_ms || !ctx->ev_end.get()) return fail(ctx, RR_ERR_STATE, "rr_timing_end: rr_timing_begin first");
    RR_HIP(hipEventRecord(ctx->ev_end.get(), ctx->stream));
    RR_HIP(hipEventSynchronize(ctx->ev_end.get()));
    RR_HIP(hipEventElapsedTime(elapsed_ms, ctx->ev_begin.get(), ctx->ev_end.get()));
    return RR_OK;
}

int rr_kernel_time(rr_context* ctx, float* sum_ms, uint32_t* n_launches)
{
    if (int r = use_device(ctx)) return r;
    if (!sum_ms || !n_launches) return RR_ERR_INVALID_ARGUMENT;
    RR_HIP(hipStreamSynchronize(ctx->stream));
    double sum = 0.0;
    for (uint32_t i = 0; i < ctx->kev_used; ++i) {
        float ms = 0.0f;
        RR_HIP(hipEventElapsedTime(&ms, ctx->kev[(size_t)i * 2].get(), ctx->kev[(size_t)i * 2 + 1].get()));
        sum += ms;
    }
    *sum_ms = (float)sum;
    *n_launches = ctx->kev_used;
    ctx->kev_used = 0;
    return RR_OK;
}

int rr_get_stats(rr_context* ctx, rr_stats* out)
{
    if (int r = use_device(ctx)) return r;
    if (!out) return RR_ERR_INVALID_ARGUMENT;
    if (int r = join_lanes(ctx)) return r;
    CounterBlock h;
    RR_HIP_MSG(hipMemcpyAsync(&h, ctx->d_cnt.get(), sizeof(CounterBlock), hipMemcpyDeviceToHost, ctx->stream), "rr_get_stats");
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "rr_get_stats");
    memset(out, 0, sizeof *out);
    uint64_t rays = 0;
    for (int i = 0; i < RAY_SHARDS; ++i) rays += h.shards[i];
    out->rays = rays;
    out->pixels = ctx->accum_pixels;
    out->primary = ctx->accum_pixels;
    out->secondary = rays - out->primary;
    out->stats_valid = ctx->last_stats ? 1u : 0u;
    if (ctx->last_stats) {
        out->hits = h.counters[C_HITS]; out->misses = h.counters[C_MISSES]; out->terminal_hits = h.counters[C_TERMINAL];
        out->tir = h.counters[C_TIR]; out->node_visits = h.counters[C_NODES]; out->tri_tests = h.counters[C_TRIS];
        out->node_trips = h.counters[C_NODE_TRIPS]; out->leaf_trips = h.counters[C_LEAF_TRIPS];
        out->shade_passes = h.counters[C_PASSES]; out->waves = h.counters[C_WAVES]; out->background_waves = h.counters[C_BG_WAVES];
        out->clock_ticks = h.counters[C_CLK_TICKS]; out->clock_ref_ticks = h.counters[C_CLK_REAL];
    }
    memcpy(out->render_kernel_name, ctx->last_kernel_name, sizeof out->render_kernel_name);
    out->traversal_overflow = h.error;
    out->bvh_depth = scene_stack_need(ctx);
    out->render_kernel = ctx->last_kernel;
    return RR_OK;
}

int rr_trace_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, rr_hit* hits)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_trace_rays: build the BLAS and TLAS first");
    if (n == 0) return RR_OK;
    if (!rays || !hits) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_trace_rays: null arrays");
    if (int r = ensure_rays(ctx, n)) return r;
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(hipMemsetAsync(&ctx->d_cnt.get()->error, 0, 4, ctx->stream));
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(launch_trace_rays(sc, ctx->d_rays.get(), n, ctx->d_hits.get(), &ctx->d_cnt.get()->error, scene_stack_need(ctx) <= 31 ? 31 : 64, ctx->stream));
    RR_HIP(hipMemcpyAsync(hits, ctx->d_hits.get(), (size_t)n * sizeof(rr_hit_dev), hipMemcpyDeviceToHost, ctx->stream));
    uint32_t err = 0;
    RR_HIP(hipMemcpyAsync(&err, &ctx->d_cnt.get()->error, 4, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    if (err) return fail(ctx, RR_ERR_TRAVERSAL_OVERFLOW, "traversal stack overflow");
    return RR_OK;
}

int rr_query_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, rr_hit* hits)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_query_rays: build the BLAS and TLAS first");
    if (n == 0) return RR_OK;
    if (!rays || !hits) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_query_rays: null arrays");
    if (int r = ensure_rays(ctx, n)) return r;
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(launch_query_rays(sc, ctx->d_rays.get(), n, ctx->d_hits.get(), inst0_mask(ctx), scene_stack_need(ctx) <= 31 ? 31 : 64, ctx->stream));
    RR_HIP(hipMemcpyAsync(hits, ctx->d_hits.get(), (size_t)n * sizeof(rr_hit_dev), hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    return RR_OK;
}

int rr_query_rays_device(rr_context* ctx, const void* d_rays, uint32_t n, void* d_hits)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_query_rays_device: build the BLAS and TLAS first");
    if (n == 0) return RR_OK;
    if (!d_rays || !d_hits || ((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_hits & 3u) != 0)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_query_rays_device: need a 16-byte aligned ray and a 4-byte aligned hit pointer");
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(launch_query_rays(sc, static_cast<const rr_ray_dev*>(d_rays), n, static_cast<rr_hit_dev*>(d_hits), inst0_mask(ctx),
                             scene_stack_need(ctx) <= 31 ? 31 : 64, ctx->stream));
    return RR_OK;
}

int rr_query_rays_multi(rr_context* ctx, const rr_ray* rays, uint32_t n, uint32_t k, rr_hit* hits, uint32_t* counts)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_query_rays_multi: build the BLAS and TLAS first");
    if (k > RR_QUERY_MAX_HITS || (k == 0 && !counts))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_query_rays_multi: need 1 <= k <= 16, or k == 0 with counts");
    if (n == 0) return RR_OK;
    if (!rays || (k && !hits)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_query_rays_multi: null arrays");
    const size_t nk = (size_t)n * k;
    if (int r = ensure_rays(ctx, n)) return r;
    if (nk > ctx->d_hits.size()) if (int r = ctx->d_hits.grow(ctx, nk)) return r;
    if (counts && n > ctx->d_counts.size()) if (int r = ctx->d_counts.grow(ctx, n)) return r;
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(launch_query_multi(sc, ctx->d_rays.get(), n, k, ctx->d_hits.get(), counts ? ctx->d_counts.get() : nullptr, inst0_mask(ctx),
                              scene_stack_need(ctx) <= 31 ? 31 : 64, ctx->stream));
    if (k) RR_HIP(hipMemcpyAsync(hits, ctx->d_hits.get(), nk * sizeof(rr_hit_dev), hipMemcpyDeviceToHost, ctx->stream));
    if (counts) RR_HIP(hipMemcpyAsync(counts, ctx->d_counts.get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    return RR_OK;
}

int rr_query_rays_multi_device(rr_context* ctx, const void* d_rays, uint32_t n, uint32_t k, void* d_hits, void* d_counts)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_query_rays_multi_device: build the BLAS and TLAS first");
    if (k > RR_QUERY_MAX_HITS || (k == 0 && !d_counts))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_query_rays_multi_device: need 1 <= k <= 16, or k == 0 with counts");
    if (n == 0) return RR_OK;
    if (!d_rays || (k && !d_hits) || ((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_hits & 3u) != 0 || ((uintptr_t)d_counts & 3u) != 0)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT,
                    "rr_query_rays_multi_device: need a 16-byte aligned ray and 4-byte aligned hit and count pointers");
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(launch_query_multi(sc, static_cast<const rr_ray_dev*>(d_rays), n, k, static_cast<rr_hit_dev*>(d_hits),
                              static_cast<uint32_t*>(d_counts), inst0_mask(ctx), scene_stack_need(ctx) <= 31 ? 31 : 64, ctx->stream));
    return RR_OK;
}

extern "C++" {
namespace {

// checks a radiance query's parameters and launches it: d_* are device pointers, any output may be null.  Touches nothing of
// the context but its error text: no counters, no frame, no kernel choice.
int shade_impl(rr_context* ctx, const char* who, const rr_ray_dev* d_rays, uint32_t n, const rr_dispatch_params& p, float4* d_f32,
               uint32_t* d_rgba8, uint32_t* d_n)
{
    if (p.max_refract < 0 || p.max_refract > 65535 || p.max_reflect < 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "shade_rays: negative bounce limit");
    if (p.max_reflect > 8) return fail(ctx, RR_ERR_UNSUPPORTED, "shade_rays: max_reflect > 8 (parked-ray registers)");
    if (!(p.ior > 0.0f)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "shade_rays: ior must be > 0");
    SceneDev sc;
    fill_scene(ctx, sc);
    DispatchDev a;                  // what shade_ray and store_pixel read
    memset(&a, 0, sizeof a);
    a.tonemap = (p.flags & RR_DISPATCH_TONEMAP_REINHARD) ? 1u : 0u;
    a.max_refract = p.max_refract; a.max_reflect = p.max_reflect;
    a.ior = p.ior; a.inv_ior = 1.0f / p.ior;
    a.tmin_s = p.tmin_secondary; a.tmax_s = p.tmax_secondary;
    // the kernel of a launch of many slices: a batch of rays is that, not a frame that ends on its longest wave
    const FusedVariant v = fused_variant(scene_facts(ctx), 64u, p.max_reflect, ctx->dbg);
    if (hipError_t e = launch_shade_rays(sc, a, d_rays, n, d_f32, d_rgba8, d_n, v.stack, v.pend, v.stack16, ctx->stream))
        return fail(ctx, RR_ERR_DEVICE, who, e);
    return RR_OK;
}

} // namespace
} // extern "C++"

int rr_shade_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f, uint8_t* rgba8,
                  uint32_t* n_rays)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_shade_rays: build the BLAS and TLAS first");
    if (n == 0) return RR_OK;
    if (!rgba32f && !rgba8) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_shade_rays: need rgba32f or rgba8");
    if (!rays) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_shade_rays: null rays");
    const rr_dispatch_params p = params_or_default(params);
    if (n > ctx->d_rays.size()) if (int r = ctx->d_rays.grow(ctx, n)) return r;
    if (rgba32f && n > ctx->d_shade_f32.size()) if (int r = ctx->d_shade_f32.grow(ctx, n)) return r;
    if (rgba8 && n > ctx->d_shade_rgba8.size()) if (int r = ctx->d_shade_rgba8.grow(ctx, n)) return r;
    if (n_rays && n > ctx->d_shade_n.size()) if (int r = ctx->d_shade_n.grow(ctx, n)) return r;
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    if (int r = shade_impl(ctx, "rr_shade_rays", ctx->d_rays.get(), n, p, rgba32f ? ctx->d_shade_f32.get() : nullptr,
                           rgba8 ? ctx->d_shade_rgba8.get() : nullptr, n_rays ? ctx->d_shade_n.get() : nullptr)) return r;
    if (rgba32f) RR_HIP(hipMemcpyAsync(rgba32f, ctx->d_shade_f32.get(), (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (rgba8) RR_HIP(hipMemcpyAsync(rgba8, ctx->d_shade_rgba8.get(), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (n_rays) RR_HIP(hipMemcpyAsync(n_rays, ctx->d_shade_n.get(), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    return RR_OK;
}

int rr_shade_rays_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f, void* d_rgba8,
                         void* d_n_rays)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_shade_rays_device: build the BLAS and TLAS first");
    if (n == 0) return RR_OK;
    if (!d_rgba32f && !d_rgba8) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_shade_rays_device: need d_rgba32f or d_rgba8");
    if (!d_rays || ((uintptr_t)d_rays & 15u) != 0 || ((uintptr_t)d_rgba32f & 15u) != 0 || ((uintptr_t)d_rgba8 & 3u) != 0 ||
        ((uintptr_t)d_n_rays & 3u) != 0)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT,
                    "rr_shade_rays_device: need 16-byte aligned ray and float pointers and 4-byte aligned rgba8 and count pointers");
    return shade_impl(ctx, "rr_shade_rays_device", static_cast<const rr_ray_dev*>(d_rays), n, params_or_default(params),
                      static_cast<float4*>(d_rgba32f), static_cast<uint32_t*>(d_rgba8), static_cast<uint32_t*>(d_n_rays));
}

int rr_env_lookup(rr_context* ctx, const float* dirs, uint32_t n, float* rgb)
{
    if (int r = use_device(ctx)) return r;
    if ((!dirs || !rgb) && n) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_env_lookup: null buffers");
    if (n == 0) return RR_OK;
    DevBuf<float> d_in, d_out;
    RR_HIP(d_in.alloc((size_t)n * 3));
    RR_HIP_MSG(d_out.alloc((size_t)n * 3), "rr_env_lookup");
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP_MSG(hipMemcpyAsync(d_in.get(), dirs, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream), "rr_env_lookup");
    RR_HIP_MSG(launch_env_lookup(sc, d_in.get(), n, d_out.get(), ctx->stream), "rr_env_lookup");
    RR_HIP_MSG(hipMemcpyAsync(rgb, d_out.get(), (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream), "rr_env_lookup");
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), "rr_env_lookup");
    return RR_OK;
}

int rr_download_blas(rr_context* ctx, uint32_t mesh_id, void* nodes, uint32_t* n_nodes, void* tris, uint32_t* n_tris)
{
    if (int r = use_device(ctx)) return r;
    if (mesh_id >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_download_blas: unknown mesh id");
    const MeshRes& m = ctx->meshes[mesh_id];
    if (!m.built) return fail(ctx, RR_ERR_STATE, "rr_download_blas: BLAS not built");
    const uint32_t nn = m.n_tris > 1 ? m.n_tris - 1 : 1;
    if (n_nodes) *n_nodes = nn;
    if (n_tris) *n_tris = m.n_tris;
    RR_HIP(hipStreamSynchronize(ctx->stream));
    if (nodes) RR_HIP(hipMemcpy(nodes, m.nodes.get(), (size_t)nn * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (tris) RR_HIP(hipMemcpy(tris, m.tris.get(), (size_t)m.n_tris * sizeof(TriRec), hipMemcpyDeviceToHost));
    return RR_OK;
}

int rr_host_register(rr_context* ctx, void* p, size_t bytes)
{
    if (int r = use_device(ctx)) return r;
    if (!p || bytes == 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_host_register: null buffer");
    RR_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return RR_OK;
}

int rr_host_unregister(rr_context* ctx, void* p)
{
    if (int r = use_device(ctx)) return r;
    if (!p) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_host_unregister: null buffer");
    RR_HIP(hipHostUnregister(p));
    return RR_OK;
}

int rr_download_qnodes(rr_context* ctx, uint32_t mesh_id, void* qnodes, uint32_t* n_nodes, float grid_org_cell[6])
{
    if (int r = use_device(ctx)) return r;
    if (mesh_id >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_download_qnodes: unknown mesh id");
    const MeshRes& m = ctx->meshes[mesh_id];
    if (!m.built) return fail(ctx, RR_ERR_STATE, "rr_download_qnodes: BLAS not built");
    const uint32_t nn = m.n_tris > 1 ? m.n_tris - 1 : 1;
    if (n_nodes) *n_nodes = nn;
    if (grid_org_cell) { memcpy(grid_org_cell, m.grid.org, 12); memcpy(grid_org_cell + 3, m.grid.cell, 12); }
    RR_HIP(hipStreamSynchronize(ctx->stream));
    if (qnodes) RR_HIP(hipMemcpy(qnodes, m.qnodes.get(), (size_t)nn * sizeof(QNode), hipMemcpyDeviceToHost));
    return RR_OK;
}

} // extern "C"
