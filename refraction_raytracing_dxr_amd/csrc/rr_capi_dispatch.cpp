// rr_capi_dispatch.cpp -- DispatchRays (RefractionDemo.cpp:580-594): output layout, DispatchDev, the stream renderer's buffers
// and passes, the choice of the render kernel and its timing, the launch; reading frames back and assembling tiles.
#include "rr_context.h"

namespace {
int ensure_cams(rr_context* ctx, size_t n)
{
    return n <= ctx->d_cams.size() ? RR_OK : ctx->d_cams.grow(ctx, n < 64 ? 64 : n);
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
uint32_t lds_node_bytes(const MeshRes& m) { return m.n_nodes() * (uint32_t)sizeof(QNode); }

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

// where a dispatch's slices go: this rank's tiles and the output's element layout (elements are 32-bit words)
struct Layout : Tiles {
    rr_mesh_partition part; uint32_t n_mesh_local;          // mesh: the caller's partition, this rank's mesh tiles
    bool want_f32, compact, rgb8;
    size_t slice_elems, stride, out_base;
};

// checks the request, lays out (and allocates) its output and GenerateCameraRay's screen tables for the frame size
int layout_dispatch(rr_context* ctx, const DispatchRequest& req, Layout& o)
{
    const uint32_t width = req.width, height = req.height, depth = req.depth;
    const rr_dispatch_params& p = req.params; uint32_t* const ext_tiles = req.ext_tiles; const MeshOut* const mesh = req.mesh;
    if (width == 0 || height == 0 || width > 32768 || height > 32768 || depth == 0 || depth > 65535)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "dispatch: bad frame size or depth");
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "dispatch: build the BLAS and TLAS first");
    if (int r = check_shading_params(ctx, "dispatch", p)) return r;

    static_cast<Tiles&>(o) = tile_counts(width, height, ctx->tile_rank, ctx->tile_world);
    memset(&o.part, 0, sizeof o.part); o.n_mesh_local = 0;
    if (mesh) {         // mesh tiles dealt round robin, background tiles to rank 0: this rank's tiles are its mesh tiles, then those
        if (!ext_tiles || !(p.flags & RR_DISPATCH_TILES_RGB8) || !req.h_cams || !mesh->part) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "mesh partition: RGB8 tile buffers and host constants");
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
    o.stride = ext_tiles ? req.ext_stride_elems : o.slice_elems;
    if (ext_tiles && o.want_f32) return fail(ctx, RR_ERR_UNSUPPORTED, "dispatch: float output is not available for external tile buffers");
    o.out_base = ext_tiles ? 0 : o.slice_elems * req.out_slot_depth * req.out_slot;
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

// the launch counts into the device block `c`
void point_counters(DispatchDev& a, CounterBlock* c) { a.counters = c->counters; a.ray_shards = c->shards; a.error_flag = &c->error; }

// DispatchRays(W, H, depth): slice f uses the constants d_cams[f] and writes to out + f * stride
DispatchDev make_dispatch(const rr_context* ctx, const DispatchRequest& req, const Layout& o)
{
    const uint32_t width = req.width, height = req.height, depth = req.depth;
    const rr_dispatch_params& p = req.params; const MeshOut* const mesh = req.mesh;
    DispatchDev a;
    memset(&a, 0, sizeof a);
    a.sx = ctx->d_screen.get(); a.sy = ctx->d_screen.get() + width;
    a.async_leaf_num = ctx->dbg_async[0]; a.async_shade_num = ctx->dbg_async[1];
    a.group_trace = ctx->dbg_group_trace ? 1u : 0u;
    uint32_t hr[4];     // where the scene can be seen at all in these slices
    (void)rr_host_screen_rect(ctx->scene_bounds, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) ? nullptr : req.h_cams, depth, width, height, hr);
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
    a.cams = req.d_cams; a.n_frames = depth;
    a.blocks_per_frame = ((o.local + 7u) & ~7u) * 4u;
    a.frame_stride = o.stride;
    a.tile_rank = ctx->tile_rank; a.tile_world = ctx->tile_world; a.n_local_tiles = o.local;
    a.n_blocks = a.blocks_per_frame * depth;
    a.compact_out = o.compact ? (o.rgb8 ? 2u : 1u) : 0u;
    a.tonemap = (p.flags & RR_DISPATCH_TONEMAP_REINHARD) ? 1u : 0u;
    a.max_refract = p.max_refract; a.max_reflect = p.max_reflect;
    a.ior = p.ior; a.inv_ior = inv_ior_of(p.ior);
    a.tmin_p = p.tmin_primary; a.tmax_p = p.tmax_primary; a.tmin_s = p.tmin_secondary; a.tmax_s = p.tmax_secondary;
    a.out_rgba8 = req.ext_tiles ? req.ext_tiles : ctx->d_rgba8.get() + o.out_base;
    a.out_f32 = o.want_f32 ? ctx->d_f32.get() + o.out_base : nullptr;
    point_counters(a, ctx->d_cnt.get());
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
    point_counters(L.a, ctx->d_cnt_trial.get());
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
} // namespace

namespace rr {
int ensure_frame_buffers(rr_context* ctx, size_t elems, bool want_f32)
{
    if (elems > ctx->d_rgba8.size())
        if (int r = ctx->d_rgba8.grow(ctx, elems)) return r;
    if (want_f32 && elems > ctx->d_f32.size()) return ctx->d_f32.grow(ctx, elems);
    return RR_OK;
}

int check_shading_params(rr_context* ctx, const char* who, const rr_dispatch_params& p)
{
    const std::string w(who);
    if (p.max_refract < 0 || p.max_refract > 65535 || p.max_reflect < 0)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": negative bounce limit").c_str());
    if (p.max_reflect > 8) return fail(ctx, RR_ERR_UNSUPPORTED, (w + ": max_reflect > 8 (parked-ray registers)").c_str());
    if (!(p.ior > 0.0f)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": ior must be > 0").c_str());
    return RR_OK;
}

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

LaunchPick pick_launch(const rr_context* ctx, const DispatchRequest& req, const uint32_t rect[4], bool compact)
{
    const rr_dispatch_params& p = req.params;
    LaunchPick k;
    k.sf = scene_facts(ctx);
    k.lf = { req.depth, ((req.width + TILE - 1) / TILE) * ((req.height + TILE - 1) / TILE), ctx->tile_world, compact, req.mesh != nullptr,
             rect[2] > rect[0] && rect[3] > rect[1], (double)(rect[2] - rect[0]) * (double)(rect[3] - rect[1]) / ((double)req.width * (double)req.height),
             p.max_refract, p.max_reflect, (p.flags & RR_DISPATCH_DEBUG_NO_CULL) != 0, !ctx->dbg_diag.empty() && ctx->single_identity };
    k.pk = pick_kernel(k.sf, k.lf, ctx->dbg);
    return k;
}

int dispatch_impl(rr_context* ctx, const DispatchRequest& req)
{
    const uint32_t width = req.width, height = req.height, depth = req.depth;
    const rr_dispatch_params& p = req.params; uint32_t* const ext_tiles = req.ext_tiles; const MeshOut* const mesh = req.mesh;
    Layout o;
    if (int r = layout_dispatch(ctx, req, o)) return r;
    Launch L;
    fill_scene(ctx, L.sc);
    L.a = make_dispatch(ctx, req, o);
    L.need = scene_stack_need(ctx); L.h_cams = req.h_cams; L.p = &p;

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

    const uint32_t rect[4] = { L.a.hx0, L.a.hy0, L.a.hx1, L.a.hy1 };
    const LaunchPick k = pick_launch(ctx, req, rect, o.compact);
    L.fused = fused_variant(k.sf, depth, p.max_reflect, ctx->dbg);
    int kernel = K_FUSED;
    if (int r = choose_kernel(ctx, L, k.pk, k.lf, kernel)) return r;

    const bool stats = (p.flags & RR_DISPATCH_COLLECT_STATS) != 0;
    const bool keep = req.keep_counters || (p.flags & RR_DISPATCH_KEEP_COUNTERS) != 0;
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

    snprintf(ctx->last_kernel_name, sizeof ctx->last_kernel_name, "%s", last_render_kernel_name());
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

int check_error_flag(rr_context* ctx, const char* what)
{
    RR_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t err = 0;
    RR_HIP(hipMemcpy(&err, &ctx->d_cnt.get()->error, 4, hipMemcpyDeviceToHost));
    return err ? fail(ctx, RR_ERR_TRAVERSAL_OVERFLOW, what) : RR_OK;
}
} // namespace rr

extern "C" {
int rr_dispatch_rays(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params)
{
    const Range range_("rr_dispatch_rays");
    if (int r = use_device(ctx)) return r;
    if (!ctx->cam_set) return fail(ctx, RR_ERR_STATE, "rr_dispatch_rays: rr_set_camera first");
    if (int r = upload_cams(ctx, &ctx->cam, 1)) return r;
    return dispatch_impl(ctx, { .width = width, .height = height, .depth = 1, .d_cams = ctx->d_cams.get(), .h_cams = &ctx->cam,
                                .params = params_or_default(params) });
}

int rr_dispatch_rays_batch(rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth,
                           const rr_scene_constants* constants, const rr_dispatch_params* params)
{
    if (int r = use_device(ctx)) return r;
    if (!constants || depth == 0) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_dispatch_rays_batch: need depth >= 1 constants");
    if (int r = upload_cams(ctx, constants, depth)) return r;
    return dispatch_impl(ctx, { .width = width, .height = height, .depth = depth, .d_cams = ctx->d_cams.get(), .h_cams = constants,
                                .params = params_or_default(params) });
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
} // extern "C"
