// rr_capi.cpp -- the C ABI of include/rrdxr.h over HIP streams.
//
// Stands where RefractionDemo.cpp's D3D12 plumbing stood: createDevice (:142-172), Mesh::upload
// (Mesh.cpp:55-94), load_texture (:108-140), the two BuildRaytracingAccelerationStructure calls
// (:277-356), the per-frame constant-buffer copy (:566), DispatchRays (:580-594), the UAV ->
// backbuffer copy (:596-604) and the fence wait (:65-71).  Everything device-side is a kernel in
// rr_bvh_build.hip / rr_render_*.hip / rr_query*.hip / rr_frame.hip; this file only owns memory, call order and error reporting.
// (Builds, dispatch, orbit loops, queries and RCCL are in the other rr_capi_*.cpp; what they share is in rr_context.h.)
#include "rr_context.h"

#include <dlfcn.h>
#include <new>

static_assert(CHOICE_TILE == (uint32_t)TILE && CHOICE_STREAM_MAX_GEN == STREAM_MAX_GEN, "rr_choice.h mirrors rr_types.h");

static_assert(sizeof(rr_vertex) == 32, "Vertex stride (Mesh.cpp:45)");
static_assert(sizeof(rr_instance_desc) == 64, "D3D12_RAYTRACING_INSTANCE_DESC");
static_assert(sizeof(rr_scene_constants) == 80, "SceneConstants");
static_assert(sizeof(rr_ray) == sizeof(rr_ray_dev) && sizeof(rr_hit) == sizeof(rr_hit_dev), "ray/hit ABI");
static_assert(offsetof(rr_ray, instance_mask) == 36 && offsetof(rr_ray_dev, instance_mask) == 36, "rr_ray.instance_mask");

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
} // namespace

namespace rr {
Range::Range(const char* name) { if (roctx().push) roctx().push(name); }
Range::~Range() { if (roctx().pop) roctx().pop(); }

int fail(rr_context* ctx, int code, const char* what, hipError_t e)
{
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}

int use_device(rr_context* ctx)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, RR_ERR_DEVICE, "hipSetDevice", e);
    return RR_OK;
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

Tiles tile_counts(uint32_t W, uint32_t H, uint32_t rank, uint32_t world)
{
    const uint32_t tiles_x = (W + TILE - 1) / TILE, n_tiles = tiles_x * ((H + TILE - 1) / TILE);
    return { tiles_x, n_tiles, n_tiles > rank ? (n_tiles - rank + world - 1) / world : 0, (n_tiles + world - 1) / world };
}

int join_lane(rr_context* ctx, uint32_t lane)
{
    if (ctx->lane_busy[lane]) {
        RR_HIP(hipStreamWaitEvent(ctx->stream, ctx->lane_done[lane].get(), 0));
        ctx->lane_busy[lane] = false;
    }
    return RR_OK;
}

// the context's stream waits for everything submitted to the lanes
int join_lanes(rr_context* ctx)
{
    for (uint32_t l = 0; l < rr_context::MAX_LANES; ++l)
        if (int r = join_lane(ctx, l)) return r;
    return RR_OK;
}

rr_dispatch_params params_or_default(const rr_dispatch_params* params)
{
    rr_dispatch_params p;
    return params ? *params : (rr_default_dispatch_params(&p), p);
}
} // namespace rr

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
    if (const char* e = getenv("RR_DEBUG_REFINE_GROUPS")) ctx->dbg_refine_groups = std::max(atoi(e), 0);
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
    return join_lane(ctx, lane);
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

int rr_local_tile_count(rr_context* ctx, uint32_t width, uint32_t height, uint32_t* n_tiles, uint32_t* max_tiles_any_rank)
{
    if (!ctx || width == 0 || height == 0) return RR_ERR_INVALID_ARGUMENT;
    const Tiles t = tile_counts(width, height, ctx->tile_rank, ctx->tile_world);
    if (n_tiles) *n_tiles = t.local;
    if (max_tiles_any_rank) *max_tiles_any_rank = t.max_local;
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

int rr_download_blas(rr_context* ctx, uint32_t mesh_id, void* nodes, uint32_t* n_nodes, void* tris, uint32_t* n_tris)
{
    if (int r = use_device(ctx)) return r;
    if (mesh_id >= ctx->meshes.size()) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_download_blas: unknown mesh id");
    const MeshRes& m = ctx->meshes[mesh_id];
    if (!m.built) return fail(ctx, RR_ERR_STATE, "rr_download_blas: BLAS not built");
    const uint32_t nn = m.n_nodes();
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
    const uint32_t nn = m.n_nodes();
    if (n_nodes) *n_nodes = nn;
    if (grid_org_cell) { memcpy(grid_org_cell, m.grid.org, 12); memcpy(grid_org_cell + 3, m.grid.cell, 12); }
    RR_HIP(hipStreamSynchronize(ctx->stream));
    if (qnodes) RR_HIP(hipMemcpy(qnodes, m.qnodes.get(), (size_t)nn * sizeof(QNode), hipMemcpyDeviceToHost));
    return RR_OK;
}

int rr_download_tlas(rr_context* ctx, void* nodes, void* qnodes, uint32_t* n_nodes, float grid_org_cell[6])
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_download_tlas: TLAS not built");
    const uint32_t nn = ctx->n_insts > 1 ? ctx->n_insts - 1 : 1;
    if (n_nodes) *n_nodes = nn;
    if (grid_org_cell) { memcpy(grid_org_cell, ctx->scene_grid.org, 12); memcpy(grid_org_cell + 3, ctx->scene_grid.cell, 12); }
    RR_HIP(hipStreamSynchronize(ctx->stream));
    if (nodes) RR_HIP(hipMemcpy(nodes, ctx->d_pool_nodes.get(), (size_t)nn * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (qnodes) RR_HIP(hipMemcpy(qnodes, ctx->d_pool_qnodes.get(), (size_t)nn * sizeof(QNode), hipMemcpyDeviceToHost));
    return RR_OK;
}
} // extern "C"
