// rr_capi_orbit.cpp -- the drawFrame loop (RefractionDemo.cpp:559-604) as batched launches: rr_render_orbit*, lanes, the
// mesh-tile partition of an orbit, and the assembly of gathered tile buffers into frames.
#include "rr_context.h"

namespace {
int ensure_lane(rr_context* ctx, uint32_t lane)
{
    if (ctx->lane_stream[lane].get()) return RR_OK;
    RR_HIP(ctx->lane_stream[lane].create(hipStreamNonBlocking));
    RR_HIP(ctx->lane_fork[lane].create(hipEventDisableTiming));
    RR_HIP(ctx->lane_done[lane].create(hipEventDisableTiming));
    return RR_OK;
}

struct Projection { float fov_y, aspect, zn, zf; };

// drawFrame loop: camera constants for n consecutive orbit angles (RefractionDemo.cpp:559-565), the angle advanced past them (:567)
int orbit_cams(rr_context* ctx, const char* what, float& angle, float angle_step, uint32_t n, const Projection& pr,
               std::vector<rr_scene_constants>& cams)
{
    cams.resize(n);
    for (uint32_t k = 0; k < n; ++k, angle += angle_step)
        if (int rc = rr_host_camera_orbit(angle, pr.fov_y, pr.aspect, pr.zn, pr.zf, &cams[k])) return fail(ctx, rc, what);
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

// frames of width x height along an orbit: n_frames angles from *angle on (advanced past them), in launches of `batch` slices;
// ext_tiles != null: compact tile output into caller memory, one frame every ext_stride_elems; host_out != null: whole RGBA8
// frames streamed to host memory
struct OrbitRequest {
    uint32_t width = 0, height = 0;
    const rr_dispatch_params* params = nullptr;
    float* angle = nullptr; float angle_step = 0.0f;
    uint32_t n_frames = 0, batch = 1;
    Projection proj = {};
    uint32_t* ext_tiles = nullptr; size_t ext_stride_elems = 0;
    uint8_t* host_out = nullptr;
};

// drawFrame loop: camera constants for n_frames consecutive orbit angles go to the device constant
// buffer in one copy; the frames are then dispatched in batches of `batch` depth slices.
int orbit_impl(rr_context* ctx, const OrbitRequest& req)
{
    const Range range_("rr_render_orbit");
    const uint32_t width = req.width, height = req.height, n_frames = req.n_frames, batch = req.batch ? req.batch : 1;
    uint32_t* const ext_tiles = req.ext_tiles; const size_t ext_stride_elems = req.ext_stride_elems;
    if (!req.angle) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "render_orbit: null angle");
    if (n_frames == 0) return RR_OK;
    rr_dispatch_params p = params_or_default(req.params);
    std::vector<rr_scene_constants> cams;
    if (int r = orbit_cams(ctx, "render_orbit: camera", *req.angle, req.angle_step, n_frames, req.proj, cams)) return r;
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
    // first launch?  (dispatch_impl's pick, changing no choice.)
    bool one_kernel_at_a_time = false;
    if (ctx->tlas_built && width && height) {
        const DispatchRequest first = { .width = width, .height = height, .depth = batch < n_frames ? batch : n_frames, .h_cams = cams.data(), .params = p };
        uint32_t rect[4];
        (void)rr_host_screen_rect(ctx->scene_bounds, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) ? nullptr : cams.data(), first.depth, width, height, rect);
        const LaunchPick k = pick_launch(ctx, first, rect, ctx->tile_world > 1 || ext_tiles);
        const KernelChoice* ch = k.pk.cls == CLS_NONE ? nullptr : ctx->ch[k.pk.cls].peek(choice_key(width, height, p, first.depth));
        one_kernel_at_a_time = chosen_kernel(k.pk, ch, k.lf.rect_share) == K_LDS;
        if (lanes > 1 && one_kernel_at_a_time) lanes = 1;
    }
    uint8_t* const host_out = req.host_out;
    if (host_out) {          // streaming to host: the copy of one region overlaps the rendering of the other
        if (ext_tiles || ctx->tile_world != 1 || (p.flags & RR_DISPATCH_FLOAT_OUTPUT))
            return fail(ctx, RR_ERR_UNSUPPORTED, "render_orbit_to_host: whole RGBA8 frames of an unsharded context only");
        lanes = ctx->frames_in_flight > 2 ? ctx->frames_in_flight : 2;
    }
    if (lanes <= 1) {
        for (uint32_t k = 0; k < n_frames; k += batch) {
            const uint32_t d = n_frames - k < batch ? n_frames - k : batch;
            uint32_t* ext = ext_tiles ? ext_tiles + (size_t)k * ext_stride_elems : nullptr;
            if (int rc = dispatch_impl(ctx, { .width = width, .height = height, .depth = d, .d_cams = ctx->d_cams.get() + k, .h_cams = cams.data() + k, .params = p,
                                              .ext_tiles = ext, .ext_stride_elems = ext_stride_elems, .keep_counters = k > 0 || keep_first })) return rc;
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
        if (int r = join_lane(ctx, l)) return r;
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
        if (rc == RR_OK)
            rc = dispatch_impl(ctx, { .width = width, .height = height, .depth = d, .d_cams = ctx->d_cams.get() + k, .h_cams = cams.data() + k, .params = p,
                                      .ext_tiles = ext, .ext_stride_elems = ext_stride_elems, .keep_counters = true, .out_slot = b % lanes, .out_slot_depth = batch });
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

extern "C" {
int rr_render_orbit(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                    float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch, float fov_y, float aspect, float zn,
                    float zf)
{
    if (int r = use_device(ctx)) return r;
    return orbit_impl(ctx, { .width = width, .height = height, .params = params, .angle = angle, .angle_step = angle_step, .n_frames = n_frames,
                             .batch = frames_per_dispatch, .proj = { fov_y, aspect, zn, zf } });
}

int rr_render_orbit_to_host(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params, float* angle,
                            float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch, float fov_y, float aspect, float zn,
                            float zf, uint8_t* host_rgba8)
{
    if (int r = use_device(ctx)) return r;
    if (!host_rgba8) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_render_orbit_to_host: null host buffer");
    if (int r = orbit_impl(ctx, { .width = width, .height = height, .params = params, .angle = angle, .angle_step = angle_step, .n_frames = n_frames,
                                  .batch = frames_per_dispatch, .proj = { fov_y, aspect, zn, zf }, .host_out = host_rgba8 })) return r;
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
    return orbit_impl(ctx, { .width = width, .height = height, .params = params, .angle = angle, .angle_step = angle_step, .n_frames = n_frames,
                             .batch = frames_per_dispatch, .proj = { fov_y, aspect, zn, zf }, .ext_tiles = (uint32_t*)d_tiles,
                             .ext_stride_elems = (size_t)(frame_stride_bytes / 4) });
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
    if (int r = orbit_cams(ctx, "rr_mesh_partition_for_orbit: camera", angle, angle_step, n_frames, { fov_y, aspect, zn, zf }, cams)) return r;
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
    if (int r = orbit_cams(ctx, "render_orbit: camera", *angle, angle_step, n_frames, { fov_y, aspect, zn, zf }, cams)) return r;
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
    if (rc == RR_OK)
        rc = dispatch_impl(ctx, { .width = width, .height = height, .depth = n_frames, .d_cams = ctx->d_cams.get(), .h_cams = cams.data(), .params = p,
                                  .ext_tiles = (uint32_t*)d_mesh_tiles, .ext_stride_elems = (size_t)(mesh_stride_bytes / 4), .keep_counters = true, .mesh = &mo });
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
} // extern "C"
