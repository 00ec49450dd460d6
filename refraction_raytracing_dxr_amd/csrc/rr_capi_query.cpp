// rr_capi_query.cpp -- rays of the caller's: the hit queries (rr_trace_rays, rr_query_rays*), the table setters, rr_env_lookup, and
// the ray-tree entry points, which come in host / _device pairs of two families, each behind one shell:
//   rays_shell   rr_shade_rays, _materials, _nested, _surfaces: the caller's rays.  Refuses, in this order: no TLAS; what the
//                family's table check refuses; (n == 0 returns); no colour output; the ray pointer (null; _device: or misaligned);
//                _device: misaligned outputs; then, behind the staging of a host call, what check_shading_params refuses.
//   frame_shell  rr_render_samples, _adaptive, _lens, _spectral, _materials, _nested, _surfaces, _composed, _shutter, _lit: a W x H
//                frame.  Refuses: no TLAS where the pair asks that before its own check (the three table pairs); what the pair's
//                check refuses (check_samples and its kin, which hold the no-colour-output refusal); _device: misaligned outputs.
// A host variant stages its arrays through the context's scratch around the launch its device variant makes; a _device variant
// returns from its shell before any of that, so it allocates, copies and waits for nothing.
#include "rr_context.h"

namespace {
// trace_rays scratch for n rays
int ensure_rays(rr_context* ctx, size_t n)
{
    if (n > ctx->d_hits.size()) if (int r = ctx->d_hits.grow(ctx, n)) return r;
    return n > ctx->d_rays.size() ? ctx->d_rays.grow(ctx, n) : RR_OK;
}

// stack entries of the query kernels' instantiation
int query_stack(const rr_context* ctx) { return scene_stack_need(ctx) <= 31 ? 31 : 64; }

// the launches of rr_query_rays* and rr_query_rays_multi*: d_* are device pointers
int query_impl(rr_context* ctx, const rr_ray_dev* d_rays, uint32_t n, rr_hit_dev* d_hits)
{
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(launch_query_rays(sc, d_rays, n, d_hits, inst0_mask(ctx), query_stack(ctx), ctx->stream));
    return RR_OK;
}

int query_multi_impl(rr_context* ctx, const rr_ray_dev* d_rays, uint32_t n, uint32_t k, rr_hit_dev* d_hits, uint32_t* d_counts)
{
    SceneDev sc;
    fill_scene(ctx, sc);
    RR_HIP(launch_query_multi(sc, d_rays, n, k, d_hits, d_counts, inst0_mask(ctx), query_stack(ctx), ctx->stream));
    return RR_OK;
}

// the fields of a radiance query's or a supersampled frame's DispatchDev that shade_ray and store_pixel read
DispatchDev shading_args(const rr_dispatch_params& p)
{
    DispatchDev a;
    memset(&a, 0, sizeof a);
    a.tonemap = (p.flags & RR_DISPATCH_TONEMAP_REINHARD) ? 1u : 0u;
    a.max_refract = p.max_refract; a.max_reflect = p.max_reflect;
    a.ior = p.ior; a.inv_ior = inv_ior_of(p.ior);
    a.tmin_s = p.tmin_secondary; a.tmax_s = p.tmax_secondary;
    return a;
}

// The host variants' outputs pass through the context's one staged set (rr_context.h).  stage: grows what the call wants to n
// elements and gives the launch its device pointers.  fetch: copies back to the caller's arrays (null: not wanted) and waits.
int stage(rr_context* ctx, size_t n, bool want_f32, bool want_rgba8, bool want_n, ShadeOut& out)
{
    if (want_f32 && n > ctx->d_out_f32.size()) if (int r = ctx->d_out_f32.grow(ctx, n)) return r;
    if (want_rgba8 && n > ctx->d_out_rgba8.size()) if (int r = ctx->d_out_rgba8.grow(ctx, n)) return r;
    if (want_n && n > ctx->d_out_n.size()) if (int r = ctx->d_out_n.grow(ctx, n)) return r;
    out = { want_f32 ? ctx->d_out_f32.get() : nullptr, want_rgba8 ? ctx->d_out_rgba8.get() : nullptr, want_n ? ctx->d_out_n.get() : nullptr };
    return RR_OK;
}
int fetch(rr_context* ctx, size_t n, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    if (rgba32f) RR_HIP(hipMemcpyAsync(rgba32f, ctx->d_out_f32.get(), n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (rgba8) RR_HIP(hipMemcpyAsync(rgba8, ctx->d_out_rgba8.get(), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (n_rays) RR_HIP(hipMemcpyAsync(n_rays, ctx->d_out_n.get(), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));
    return RR_OK;
}

// The outputs as an entry point takes them: host arrays, or with `device` device pointers; any may be null (not wanted).  n_taken
// is rr_render_adaptive's second count array, of which the shells look at the alignment alone.
struct CallerOut { void* f32; void* rgba8; void* n_rays; bool device; void* n_taken = nullptr; };

// a refusal in the entry point's name (the text is put together only here, where a call fails)
int refuse(rr_context* ctx, int code, const char* who, const char* what) { return fail(ctx, code, (std::string(who) + what).c_str()); }

// what the _device variants refuse of their output pointers (null passes: not wanted), with the entry point's own message
int check_out_alignment(rr_context* ctx, const CallerOut& o, const char* who, const char* what)
{
    const bool ok = ((uintptr_t)o.f32 & 15u) == 0 && (((uintptr_t)o.rgba8 | (uintptr_t)o.n_rays | (uintptr_t)o.n_taken) & 3u) == 0;
    return ok ? RR_OK : refuse(ctx, RR_ERR_INVALID_ARGUMENT, who, what);
}

// a _device variant's outputs as the launch takes them
ShadeOut device_out(const CallerOut& o) { return { static_cast<float4*>(o.f32), static_cast<uint32_t*>(o.rgba8), static_cast<uint32_t*>(o.n_rays) }; }

// The frame shell (the header comment has the order of its refusals).  who: the entry point's name; tlas_first: the pair refuses
// a missing TLAS before its own check; check(have_colour) is that check, launch(out) the launch of the checked frame, whose
// `out` holds device pointers.  A _device call returns from the first branch: nothing staged, copied or waited for.
template <class Check, class Launch>
int frame_shell(rr_context* ctx, const char* who, uint32_t width, uint32_t height, const CallerOut& o, bool tlas_first, Check check, Launch launch)
{
    if (int r = use_device(ctx)) return r;
    if (tlas_first && !ctx->tlas_built) return refuse(ctx, RR_ERR_STATE, who, ": build the BLAS and TLAS first");
    if (int r = check(o.f32 || o.rgba8)) return r;
    if (o.device) {
        if (int r = check_out_alignment(ctx, o, who, ": need a 16-byte aligned float pointer and 4-byte aligned rgba8 and count pointers")) return r;
        return launch(device_out(o));
    }
    const size_t n = (size_t)width * height;
    ShadeOut out;
    if (int r = stage(ctx, n, o.f32, o.rgba8, o.n_rays, out)) return r;
    if (int r = launch(out)) return r;
    return fetch(ctx, n, static_cast<float*>(o.f32), static_cast<uint8_t*>(o.rgba8), static_cast<uint32_t*>(o.n_rays));
}

// One tree of the rays family: the name check_shading_params refuses under (null: the entry point's own), what the family asks
// of the scene's tables (null: nothing; p is the caller's parameters, whose ior a table check replaces), and the launch.
struct RayTree {
    const char* params_name;
    int (*check_tables)(rr_context* ctx, const char* who, rr_dispatch_params& p);
    hipError_t (*launch)(rr_context* ctx, const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* d_rays, uint32_t n, const ShadeOut& out, const FusedVariant& v);
};

// checks a radiance query's parameters and launches it: d_rays is a device pointer.  Touches nothing of
// the context but its error text: no counters, no frame, no kernel choice.
int shade_impl(rr_context* ctx, const char* who, const RayTree& tree, const rr_ray_dev* d_rays, uint32_t n, const rr_dispatch_params& p, const ShadeOut& out)
{
    if (int r = check_shading_params(ctx, tree.params_name ? tree.params_name : who, p)) return r;
    SceneDev sc;
    fill_scene(ctx, sc);
    const DispatchDev a = shading_args(p);
    // the kernel of a launch of many slices: a batch of rays is that, not a frame that ends on its longest wave
    const FusedVariant v = fused_variant(scene_facts(ctx), 64u, p.max_reflect, ctx->dbg);
    if (hipError_t e = tree.launch(ctx, sc, a, d_rays, n, out, v)) return fail(ctx, RR_ERR_DEVICE, who, e);
    return RR_OK;
}

// The rays shell (the header comment has the order of its refusals): rays and o hold host arrays, or with o.device device pointers
int rays_shell(rr_context* ctx, const char* who, const RayTree& tree, const void* rays, uint32_t n, const rr_dispatch_params* params, const CallerOut& o)
{
    if (int r = use_device(ctx)) return r;
    if (!ctx->tlas_built) return refuse(ctx, RR_ERR_STATE, who, ": build the BLAS and TLAS first");
    rr_dispatch_params p = params_or_default(params);
    if (tree.check_tables) if (int r = tree.check_tables(ctx, who, p)) return r;
    if (n == 0) return RR_OK;
    if (!o.f32 && !o.rgba8) return refuse(ctx, RR_ERR_INVALID_ARGUMENT, who, o.device ? ": need d_rgba32f or d_rgba8" : ": need rgba32f or rgba8");
    if (o.device) {
        const char* const align = ": need 16-byte aligned ray and float pointers and 4-byte aligned rgba8 and count pointers";
        if (!rays || ((uintptr_t)rays & 15u) != 0) return refuse(ctx, RR_ERR_INVALID_ARGUMENT, who, align);
        if (int r = check_out_alignment(ctx, o, who, align)) return r;
        return shade_impl(ctx, who, tree, static_cast<const rr_ray_dev*>(rays), n, p, device_out(o));
    }
    if (!rays) return refuse(ctx, RR_ERR_INVALID_ARGUMENT, who, ": null rays");
    if (n > ctx->d_rays.size()) if (int r = ctx->d_rays.grow(ctx, n)) return r;
    ShadeOut out;
    if (int r = stage(ctx, n, o.f32, o.rgba8, o.n_rays, out)) return r;
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    if (int r = shade_impl(ctx, who, tree, ctx->d_rays.get(), n, p, out)) return r;
    return fetch(ctx, n, static_cast<float*>(o.f32), static_cast<uint8_t*>(o.rgba8), static_cast<uint32_t*>(o.n_rays));
}

hipError_t shade_plain(rr_context* ctx, const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* d_rays, uint32_t n, const ShadeOut& out, const FusedVariant& v)
{
    return launch_shade_rays(sc, a, d_rays, n, out, v, ctx->stream);
}
const RayTree kShadeRays = { "shade_rays", nullptr, shade_plain };

// a supersampled frame as its two entry points take it (pointers of the caller's: host memory)
struct SamplesReq {
    const char* who;
    uint32_t width, height;
    const rr_scene_constants* constants; const rr_dispatch_params* params; const float* offsets; uint32_t n_samples;
};

// what both variants of rr_render_samples refuse before they look at their outputs' memory or allocate anything (bounce limits
// and ior included); fills the offsets.  live: the frame traces the live scene, which must be built (a shutter frame traces keys)
int check_samples(rr_context* ctx, const SamplesReq& q, bool have_colour, SampleOffsets& off, bool live = true)
{
    const std::string w(q.who);
    if (live && !ctx->tlas_built) return fail(ctx, RR_ERR_STATE, (w + ": build the BLAS and TLAS first").c_str());
    if (!q.constants) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": null constants").c_str());
    if (q.width == 0 || q.height == 0 || q.width > 32768u || q.height > 32768u)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": width and height must be 1..32768").c_str());
    if (!have_colour) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need rgba32f or rgba8").c_str());
    if (int r = check_shading_params(ctx, "render_samples", params_or_default(q.params))) return r;
    memset(&off, 0, sizeof off);
    if (!q.offsets) {
        if (rr_host_sample_pattern(q.n_samples, off.v)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": the built-in patterns have 1, 2, 4, 8 or 16 samples").c_str());
        return RR_OK;
    }
    if (q.n_samples == 0 || q.n_samples > RR_MAX_SAMPLES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need 1 <= n_samples <= 64").c_str());
    for (uint32_t i = 0; i < 2 * q.n_samples; ++i) {
        if (!(q.offsets[i] >= 0.0f && q.offsets[i] <= 1.0f))        // (NaN fails both comparisons)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": offsets must lie in [0, 1]").c_str());
        off.v[i] = q.offsets[i];
    }
    return RR_OK;
}

// what the launch of a checked supersampled or adaptive frame takes: the scene, the frame's shading arguments with its screen
// rectangle (lens: the rectangle of its whole disk, rr_host_lens_screen_rect), the camera and the scene's kernel variant
struct FrameArgs { SceneDev sc; DispatchDev a; CamDev cam; FusedVariant v; };
// everything of FrameArgs but the scene, for what is traced having the world-space box `bounds` and the facts `sf`
FrameArgs frame_args_of(rr_context* ctx, const SamplesReq& q, const rr_lens* lens, const float bounds[6], const SceneFacts& sf)
{
    const rr_dispatch_params p = params_or_default(q.params);
    FrameArgs f;
    memset(&f.sc, 0, sizeof f.sc);
    f.a = shading_args(p);
    f.a.W = q.width; f.a.H = q.height;
    f.a.tmin_p = p.tmin_primary; f.a.tmax_p = p.tmax_primary;
    uint32_t hr[4];
    const rr_scene_constants* const seen = (p.flags & RR_DISPATCH_DEBUG_NO_CULL) ? nullptr : q.constants;
    if (lens) (void)rr_host_lens_screen_rect(bounds, seen, lens, q.width, q.height, hr);
    else (void)rr_host_screen_rect(bounds, seen, 1, q.width, q.height, hr);
    f.a.hx0 = hr[0]; f.a.hy0 = hr[1]; f.a.hx1 = hr[2]; f.a.hy1 = hr[3];
    memcpy(f.cam.M, q.constants->proj_inv, sizeof f.cam.M);
    memcpy(f.cam.cam, q.constants->camera_loc, sizeof f.cam.cam);
    // the kernel of a launch of many slices, as a radiance query's: S trees per lane, not a frame that ends on its longest wave
    f.v = fused_variant(sf, 64u, p.max_reflect, ctx->dbg);
    return f;
}
FrameArgs frame_args(rr_context* ctx, const SamplesReq& q, const rr_lens* lens = nullptr)
{
    FrameArgs f = frame_args_of(ctx, q, lens, ctx->scene_bounds, scene_facts(ctx));
    fill_scene(ctx, f.sc);
    return f;
}

// One tree of the supersampled frames that differ in nothing else (samples, materials, nested, surfaces): what the pair asks of
// the scene's tables before check_samples (null: nothing, and no TLAS refusal of its own), and the launch.
struct FrameTree {
    int (*check_tables)(rr_context* ctx, const char* who, rr_dispatch_params& p);
    hipError_t (*launch)(rr_context* ctx, const FrameArgs& f, const SampleOffsets& off, uint32_t n_samples, const ShadeOut& out);
};

// Both variants of such a frame, through the frame shell.  The launch touches nothing of the context but its error text, and it
// allocates and copies nothing: constants and offsets travel as kernel arguments.  With a table check q.params becomes its result.
int samples_pair(rr_context* ctx, SamplesReq q, const FrameTree& tree, const CallerOut& o)
{
    rr_dispatch_params p = params_or_default(q.params);
    if (tree.check_tables) q.params = &p;
    SampleOffsets off;
    return frame_shell(ctx, q.who, q.width, q.height, o, tree.check_tables != nullptr,
                       [&](bool have_colour) {
                           if (tree.check_tables) if (int r = tree.check_tables(ctx, q.who, p)) return r;
                           return check_samples(ctx, q, have_colour, off);
                       },
                       [&](const ShadeOut& out) {
                           if (hipError_t e = tree.launch(ctx, frame_args(ctx, q), off, q.n_samples, out)) return fail(ctx, RR_ERR_DEVICE, q.who, e);
                           return (int)RR_OK;
                       });
}

hipError_t frame_plain(rr_context* ctx, const FrameArgs& f, const SampleOffsets& off, uint32_t n_samples, const ShadeOut& out)
{
    return launch_render_samples(f.sc, f.a, f.cam, off, n_samples, out, f.v, ctx->stream);
}
const FrameTree kSamples = { nullptr, frame_plain };

// an adaptive frame: a supersampled frame of n_samples = n_max samples, of which every pixel takes the first n_base
struct AdaptiveReq { SamplesReq s; uint32_t n_base; float threshold; };

// what both variants of rr_render_adaptive refuse before they look at device memory or allocate anything; fills the offsets
int check_adaptive(rr_context* ctx, const AdaptiveReq& q, bool have_colour, SampleOffsets& off)
{
    if (int r = check_samples(ctx, q.s, have_colour, off)) return r;
    const std::string w(q.s.who);
    if (q.n_base == 0 || q.n_base > q.s.n_samples) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need 1 <= n_base <= n_max").c_str());
    if (!(q.threshold >= 0.0f) || std::isinf(q.threshold))      // (NaN fails the comparison)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": threshold must be finite and >= 0").c_str());
    return RR_OK;
}

// launches a checked adaptive frame: device pointers, a workspace of at least rr_host_adaptive_workspace_bytes.  Allocates,
// copies and synchronises nothing.
int adaptive_impl(rr_context* ctx, const AdaptiveReq& q, const SampleOffsets& off, const ShadeOut& out, uint32_t* n_taken, const AdaptiveWorkspace& ws)
{
    const FrameArgs f = frame_args(ctx, q.s);
    if (hipError_t e = launch_render_adaptive(f.sc, f.a, f.cam, off, q.n_base, q.s.n_samples, q.threshold, ws, n_taken,
                                              (uint32_t)ctx->dbg_refine_groups, out, f.v, ctx->stream))
        return fail(ctx, RR_ERR_DEVICE, q.s.who, e);
    return RR_OK;
}

// Both variants of rr_render_adaptive, through the frame shell: what the pair has beyond the three outputs sits in the launch
// step, where it stood between the shell's steps before.  _device (o.n_taken, workspace: device pointers): the workspace refusal
// behind the shell's alignment refusal, then the launch.  Host (o.n_taken, n_refined: the caller's): between the staging and the
// fetch, the growth of the context's n_taken and workspace buffers, the launch and the copies the fetch then waits for.
int adaptive_pair(rr_context* ctx, const AdaptiveReq& q, const CallerOut& o, void* d_workspace, uint64_t workspace_bytes, uint64_t* n_refined)
{
    const uint32_t width = q.s.width, height = q.s.height;
    uint32_t* const n_taken = static_cast<uint32_t*>(o.n_taken);
    SampleOffsets off;
    uint32_t total = 0;
    const int rc = frame_shell(ctx, q.s.who, width, height, o, false,
        [&](bool have_colour) { return check_adaptive(ctx, q, have_colour, off); },
        [&](const ShadeOut& out) {
            if (o.device) {
                if (!d_workspace || ((uintptr_t)d_workspace & 15u) != 0 || workspace_bytes < rr_host_adaptive_workspace_bytes(width, height))
                    return refuse(ctx, RR_ERR_INVALID_ARGUMENT, q.s.who, ": need a 16-byte aligned workspace of at least rr_host_adaptive_workspace_bytes(width, height) bytes");
                return adaptive_impl(ctx, q, off, out, n_taken, AdaptiveWorkspace(d_workspace, width, height));
            }
            const size_t n = (size_t)width * height;
            const size_t ws_units = (size_t)(rr_host_adaptive_workspace_bytes(width, height) / 16u);
            if (n_taken && n > ctx->d_adaptive_taken.size()) if (int r = ctx->d_adaptive_taken.grow(ctx, n)) return r;
            if (ws_units > ctx->d_adaptive_ws.size()) if (int r = ctx->d_adaptive_ws.grow(ctx, ws_units)) return r;
            const AdaptiveWorkspace ws(ctx->d_adaptive_ws.get(), width, height);
            if (int r = adaptive_impl(ctx, q, off, out, n_taken ? ctx->d_adaptive_taken.get() : nullptr, ws)) return r;
            if (n_taken) RR_HIP(hipMemcpyAsync(n_taken, ctx->d_adaptive_taken.get(), n * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (n_refined) RR_HIP(hipMemcpyAsync(&total, ws.total, 4, hipMemcpyDeviceToHost, ctx->stream));
            return (int)RR_OK;
        });
    if (rc == RR_OK && n_refined) *n_refined = total;
    return rc;
}

// a thin-lens frame: a supersampled frame with a lens and one lens offset per sample
struct LensReq { SamplesReq s; const float* lens_offsets; const rr_lens* lens; };

// what both variants of rr_render_lens refuse before they look at their outputs' memory or allocate anything: what
// rr_render_samples refuses, then the lens and its offsets; fills both tables and the lens
int check_lens(rr_context* ctx, const LensReq& q, bool have_colour, SampleOffsets& off, SampleOffsets& loff, LensDev& lens)
{
    if (int r = check_samples(ctx, q.s, have_colour, off)) return r;
    const std::string w(q.s.who);
    if (!q.lens) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": null lens").c_str());
    if (lens_setup(q.s.constants, q.lens, &lens))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need a finite radius >= 0, a finite focus_distance > 0 and proj_inv columns of finite non-zero length").c_str());
    memset(&loff, 0, sizeof loff);
    if (!q.lens_offsets) {
        (void)rr_host_lens_pattern(q.s.n_samples, loff.v);      // (1 <= n_samples <= 64: check_samples)
        return RR_OK;
    }
    for (uint32_t i = 0; i < 2 * q.s.n_samples; ++i) {
        if (!(q.lens_offsets[i] >= -1.0f && q.lens_offsets[i] <= 1.0f))     // (NaN fails both comparisons)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": lens offsets must lie in [-1, 1]").c_str());
        loff.v[i] = q.lens_offsets[i];
    }
    return RR_OK;
}

// launches a checked thin-lens frame: out holds device pointers.  As samples_pair's launch: nothing of the context but its error text,
// nothing allocated or copied.
int lens_impl(rr_context* ctx, const LensReq& q, const SampleOffsets& off, const SampleOffsets& loff, const LensDev& lens, const ShadeOut& out)
{
    const FrameArgs f = frame_args(ctx, q.s, q.lens);
    if (hipError_t e = launch_render_lens(f.sc, f.a, f.cam, off, loff, lens, q.s.n_samples, out, f.v, ctx->stream))
        return fail(ctx, RR_ERR_DEVICE, q.s.who, e);
    return RR_OK;
}

// both variants of rr_render_lens, through the frame shell
int lens_pair(rr_context* ctx, const LensReq& q, const CallerOut& o)
{
    SampleOffsets off, loff;
    LensDev ld;
    return frame_shell(ctx, q.s.who, q.s.width, q.s.height, o, false,
                       [&](bool have_colour) { return check_lens(ctx, q, have_colour, off, loff, ld); },
                       [&](const ShadeOut& out) { return lens_impl(ctx, q, off, loff, ld, out); });
}

// a spectral frame: a supersampled frame with one band (index of refraction, channel weights) per sample
struct SpectralReq { SamplesReq s; const rr_band* bands; };

// what both variants of rr_render_spectral refuse before they look at their outputs' memory or allocate anything: what
// rr_render_samples refuses (params->ior included, although the bands replace it), then the bands; fills both tables.
// bands == NULL: every row is { params->ior, 1, 1, 1 }, the frame of rr_render_samples
int check_spectral(rr_context* ctx, const SpectralReq& q, bool have_colour, SampleOffsets& off, BandTable& bands)
{
    if (int r = check_samples(ctx, q.s, have_colour, off)) return r;
    const std::string w(q.s.who);
    const float ior = params_or_default(q.s.params).ior;
    memset(&bands, 0, sizeof bands);
    for (uint32_t k = 0; k < q.s.n_samples; ++k) {              // (1 <= n_samples <= 64: check_samples)
        const rr_band b = q.bands ? q.bands[k] : rr_band{ ior, { 1.0f, 1.0f, 1.0f } };
        if (!std::isfinite(b.ior) || !(b.ior > 0.0f)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": every band's ior must be finite and > 0").c_str());
        for (int ch = 0; ch < 3; ++ch) {
            if (!std::isfinite(b.weight[ch])) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": every band's weights must be finite").c_str());
            bands.weight[k][ch] = b.weight[ch];
        }
        bands.ior[k] = b.ior; bands.inv_ior[k] = inv_ior_of(b.ior);
    }
    return RR_OK;
}

// launches a checked spectral frame: out holds device pointers.  As samples_pair's launch: nothing of the context but its error text,
// nothing allocated or copied.
int spectral_impl(rr_context* ctx, const SpectralReq& q, const SampleOffsets& off, const BandTable& bands, const ShadeOut& out)
{
    const FrameArgs f = frame_args(ctx, q.s);
    if (hipError_t e = launch_render_spectral(f.sc, f.a, f.cam, off, bands, q.s.n_samples, out, f.v, ctx->stream))
        return fail(ctx, RR_ERR_DEVICE, q.s.who, e);
    return RR_OK;
}

// both variants of rr_render_spectral, through the frame shell
int spectral_pair(rr_context* ctx, const SpectralReq& q, const CallerOut& o)
{
    SampleOffsets off;
    BandTable bt;
    return frame_shell(ctx, q.s.who, q.s.width, q.s.height, o, false,
                       [&](bool have_colour) { return check_spectral(ctx, q, have_colour, off, bt); },
                       [&](const ShadeOut& out) { return spectral_impl(ctx, q, off, bt, out); });
}

// What both material calls need beside their scalar twins' checks: a table, and every instance of the scene inside it.  The index
// of refraction comes from the table, so the one in params is not looked at: the checks and shading_args see a valid one instead.
int check_materials(rr_context* ctx, const char* who, rr_dispatch_params& p)
{
    const std::string w(who);
    if (!ctx->n_mats) return fail(ctx, RR_ERR_STATE, (w + ": set a material table first (rr_set_materials)").c_str());
    if (ctx->max_material >= ctx->n_mats)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": an instance's hit-group index is not below the material table's length").c_str());
    p.ior = 1.0f;
    return RR_OK;
}

// the hit-group index of instance 0, which the kernels take as an argument where the scene skips the top level
uint32_t inst0_material(const rr_context* ctx) { return ctx->inst_host.empty() ? 0u : ctx->inst_host[0].hitgroup_flags & 0xffffffu; }

// the ray tree with the material table (p: after check_materials), on caller rays and as a frame
hipError_t shade_mat(rr_context* ctx, const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* d_rays, uint32_t n, const ShadeOut& out, const FusedVariant& v)
{
    return launch_shade_rays_mat(sc, a, ctx->d_mats.get(), inst0_material(ctx), d_rays, n, out, v, ctx->stream);
}
hipError_t frame_mat(rr_context* ctx, const FrameArgs& f, const SampleOffsets& off, uint32_t n_samples, const ShadeOut& out)
{
    return launch_render_materials(f.sc, f.a, f.cam, off, ctx->d_mats.get(), inst0_material(ctx), n_samples, out, f.v, ctx->stream);
}
const RayTree kShadeMaterials = { "shade_rays_materials", check_materials, shade_mat };
const FrameTree kMaterials = { check_materials, frame_mat };

// What the nested calls need beside check_materials: a list entry is one byte holding row + 1, so no instance's row above 254
int check_nested(rr_context* ctx, const char* who, rr_dispatch_params& p)
{
    if (int r = check_materials(ctx, who, p)) return r;
    if (ctx->max_material > RR_NESTED_MAX_MATERIAL)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (std::string(who) + ": an instance's hit-group index is above RR_NESTED_MAX_MATERIAL (254)").c_str());
    return RR_OK;
}

// the material trees with the nested tree (p: after check_nested)
hipError_t shade_nested(rr_context* ctx, const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* d_rays, uint32_t n, const ShadeOut& out, const FusedVariant& v)
{
    return launch_shade_rays_nested(sc, a, ctx->d_mats.get(), inst0_material(ctx), d_rays, n, out, v, ctx->stream);
}
hipError_t frame_nested(rr_context* ctx, const FrameArgs& f, const SampleOffsets& off, uint32_t n_samples, const ShadeOut& out)
{
    return launch_render_nested(f.sc, f.a, f.cam, off, ctx->d_mats.get(), inst0_material(ctx), n_samples, out, f.v, ctx->stream);
}
const RayTree kShadeNested = { "shade_rays_nested", check_nested, shade_nested };
const FrameTree kNested = { check_nested, frame_nested };

// the nested trees with the surface table and the lights (p: after check_nested).  On caller rays check_shading_params refuses
// under the entry point's own name, unlike its three siblings.  surface_launch: the context's table, lights and shadow_steps as the
// launchers take them -- the cap picks the kernel there (0: the first-hit shadow ray, else the walk)
SurfaceLaunch surface_launch(const rr_context* ctx) { return { ctx->d_surfs.get(), ctx->n_surfs, &ctx->lights, ctx->shadow_steps }; }
hipError_t shade_surfaces(rr_context* ctx, const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* d_rays, uint32_t n, const ShadeOut& out, const FusedVariant& v)
{
    return launch_shade_rays_surfaces(sc, a, ctx->d_mats.get(), surface_launch(ctx), inst0_material(ctx), d_rays, n, out, v, ctx->stream);
}
hipError_t frame_surfaces(rr_context* ctx, const FrameArgs& f, const SampleOffsets& off, uint32_t n_samples, const ShadeOut& out)
{
    return launch_render_surfaces(f.sc, f.a, f.cam, off, ctx->d_mats.get(), surface_launch(ctx), inst0_material(ctx), n_samples, out, f.v, ctx->stream);
}
const RayTree kShadeSurfaces = { nullptr, check_nested, shade_surfaces };
const FrameTree kSurfaces = { check_nested, frame_surfaces };

// a composed frame: a nested frame whose samples each have a lens offset and a band of the context's band set; lens may be null
// (a pinhole).  s.offsets is not the caller's: check_composed points it at the sub-pixel positions it takes from the samples
struct ComposedReq { SamplesReq s; const rr_composed_sample* samples; const rr_lens* lens; };
struct ComposedTables { SampleOffsets off, loff; LensDev lens; SampleBands band; float pos[2 * RR_MAX_SAMPLES]; };

// what both variants of rr_render_composed refuse before they look at their outputs' memory or allocate anything: what
// rr_render_nested refuses (p: its check_nested result, which q.s.params points at), then the lens and its offsets as
// rr_render_lens (a pinhole looks at no lens offset), then the bands; fills the tables
// check_composed behind the scene's state: the samples, the lens and the bands (live: as check_samples)
int check_composed_args(rr_context* ctx, ComposedReq& q, bool have_colour, ComposedTables& t, bool live)
{
    const std::string w(q.s.who);
    if (!q.samples) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": null samples").c_str());
    if (q.s.n_samples == 0 || q.s.n_samples > RR_MAX_SAMPLES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need 1 <= n_samples <= 64").c_str());
    for (uint32_t k = 0; k < q.s.n_samples; ++k) { t.pos[2 * k] = q.samples[k].offset[0]; t.pos[2 * k + 1] = q.samples[k].offset[1]; }
    q.s.offsets = t.pos;
    if (int r = check_samples(ctx, q.s, have_colour, t.off, live)) return r;
    memset(&t.loff, 0, sizeof t.loff);
    memset(&t.lens, 0, sizeof t.lens);
    t.lens.pinhole = 1u;
    if (q.lens && lens_setup(q.s.constants, q.lens, &t.lens))
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need a finite radius >= 0, a finite focus_distance > 0 and proj_inv columns of finite non-zero length").c_str());
    const uint32_t n_bands = ctx->n_bands ? ctx->n_bands : 1u;
    memset(&t.band, 0, sizeof t.band);
    for (uint32_t k = 0; k < q.s.n_samples; ++k) {
        const rr_composed_sample& c = q.samples[k];
        if (!t.lens.pinhole) for (int i = 0; i < 2; ++i) {
            if (!(c.lens_offset[i] >= -1.0f && c.lens_offset[i] <= 1.0f))       // (NaN fails both comparisons)
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": lens offsets must lie in [-1, 1]").c_str());
            t.loff.v[2 * k + i] = c.lens_offset[i];
        }
        if (c.band >= n_bands) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a sample's band is not below the number of bands in force (1 without rr_set_material_bands)").c_str());
        t.band.set(k, c.band);                                  // (n_bands <= 64: a byte)
    }
    return RR_OK;
}
int check_composed(rr_context* ctx, ComposedReq& q, rr_dispatch_params& p, bool have_colour, ComposedTables& t)
{
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, (std::string(q.s.who) + ": build the BLAS and TLAS first").c_str());
    if (int r = check_nested(ctx, q.s.who, p)) return r;
    return check_composed_args(ctx, q, have_colour, t, true);
}

// the band set in force on the device, or the material table and the weights 1 in its place
struct BandSet { const MatDev* mats; const float* weights; };
BandSet band_set(const rr_context* ctx)
{
    return ctx->n_bands ? BandSet{ ctx->d_band_mats.get(), ctx->d_band_w.get() } : BandSet{ ctx->d_mats.get(), ctx->d_band_one.get() };
}

// launches a checked composed frame: out holds device pointers.  As a nested frame: nothing of the context but its error text,
// nothing allocated, copied or waited for -- the band set, or the table in force and the weights 1 in its place, is on the device
int composed_impl(rr_context* ctx, const ComposedReq& q, const ComposedTables& t, const ShadeOut& out)
{
    const FrameArgs f = frame_args(ctx, q.s, q.lens);
    const BandSet b = band_set(ctx);
    if (hipError_t e = launch_render_composed(f.sc, f.a, f.cam, t.off, t.loff, t.lens, t.band, b.mats, ctx->n_mats, b.weights, inst0_material(ctx),
                                              q.s.n_samples, out, f.v, ctx->stream))
        return fail(ctx, RR_ERR_DEVICE, q.s.who, e);
    return RR_OK;
}

// both variants of rr_render_composed, through the frame shell (q.s.params: the caller's; the checks see their own copy)
int composed_pair(rr_context* ctx, ComposedReq q, const CallerOut& o)
{
    rr_dispatch_params p = params_or_default(q.s.params);
    q.s.params = &p;
    ComposedTables t;
    return frame_shell(ctx, q.s.who, q.s.width, q.s.height, o, false,
                       [&](bool have_colour) { return check_composed(ctx, q, p, have_colour, t); },
                       [&](const ShadeOut& out) { return composed_impl(ctx, q, t, out); });
}

// a shutter frame: a composed frame whose samples each name a captured scene key.  c: the samples as composed records (what
// check_composed_args reads), used: which keys the frame traces in
struct ShutterReq { ComposedReq c; const rr_shutter_sample* samples; };
struct ShutterTables { ComposedTables c; SampleKeys key; rr_composed_sample rec[RR_MAX_SAMPLES]; bool used[RR_MAX_SCENE_KEYS]; };

// what both variants of rr_render_shutter refuse before they look at their outputs' memory: a missing table, what rr_render_composed
// refuses of its arguments (the live scene's state is not looked at: the frame traces keys), then the keys; fills the tables
int check_shutter(rr_context* ctx, ShutterReq& q, rr_dispatch_params& p, bool have_colour, ShutterTables& t)
{
    const std::string w(q.c.s.who);
    if (!ctx->n_mats) return fail(ctx, RR_ERR_STATE, (w + ": set a material table first (rr_set_materials)").c_str());
    p.ior = 1.0f;                                               // (not looked at, as check_materials has it)
    if (!q.samples) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": null samples").c_str());
    if (q.c.s.n_samples == 0 || q.c.s.n_samples > RR_MAX_SAMPLES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": need 1 <= n_samples <= 64").c_str());
    for (uint32_t k = 0; k < q.c.s.n_samples; ++k) {
        const rr_shutter_sample& s = q.samples[k];
        t.rec[k] = rr_composed_sample{ { s.offset[0], s.offset[1] }, { s.lens_offset[0], s.lens_offset[1] }, s.band, { 0u, 0u, 0u } };
    }
    q.c.samples = t.rec;
    if (int r = check_composed_args(ctx, q.c, have_colour, t.c, false)) return r;
    memset(&t.key, 0, sizeof t.key);
    memset(t.used, 0, sizeof t.used);
    const SceneKey* first = nullptr;
    for (uint32_t k = 0; k < q.c.s.n_samples; ++k) {
        const rr_shutter_sample& s = q.samples[k];
        if (s.pad[0] || s.pad[1]) return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a sample's pad must be zero").c_str());
        if (s.key >= RR_MAX_SCENE_KEYS || !ctx->keys[s.key].captured)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a sample's key is not a captured scene key (rr_capture_scene_key)").c_str());
        const SceneKey& sk = ctx->keys[s.key];
        if (!first) first = &sk;
        if (sk.facts.single_identity != first->facts.single_identity)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": the keys of one frame must all have a top level or all be without one").c_str());
        if (sk.max_material >= ctx->n_mats)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a key's hit-group index is not below the material table's length").c_str());
        if (sk.max_material > RR_NESTED_MAX_MATERIAL)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a key's hit-group index is above RR_NESTED_MAX_MATERIAL (254)").c_str());
        t.used[s.key] = true;
        t.key.set(k, s.key);
    }
    return RR_OK;
}

// what a shutter frame's launch takes from the keys it uses.  The rectangle is that of the union of the used keys' boxes; the
// kernel variant comes from fused_variant over the used keys' facts merged: the deepest stack need, the largest mesh and pools
// (16-bit stack entries only where every key's references fit them)
struct ShutterFrame { FrameArgs f; bool single_identity; };
ShutterFrame shutter_frame(rr_context* ctx, const ShutterReq& q, const ShutterTables& t)
{
    float box[6] = { 3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f };
    SceneFacts sf = { false, 0, 0, 0, 0, false };
    for (uint32_t k = 0; k < RR_MAX_SCENE_KEYS; ++k) {
        if (!t.used[k]) continue;
        const SceneKey& sk = ctx->keys[k];
        for (int i = 0; i < 3; ++i) { box[i] = std::min(box[i], sk.bounds[i]); box[3 + i] = std::max(box[3 + i], sk.bounds[3 + i]); }
        sf.single_identity = sk.facts.single_identity;          // (the same in every used key: check_shutter)
        sf.need = std::max(sf.need, sk.facts.need);
        sf.blas_tris = std::max(sf.blas_tris, sk.facts.blas_tris);
        sf.pool_nodes = std::max(sf.pool_nodes, sk.facts.pool_nodes);
        sf.pool_refs = std::max(sf.pool_refs, sk.facts.pool_refs);
    }
    return { frame_args_of(ctx, q.c.s, q.c.lens, box, sf), sf.single_identity };
}

// launches a checked shutter frame: out holds device pointers.  As composed_impl: nothing allocated, copied or waited for -- the
// key records are on the device since their capture
int shutter_impl(rr_context* ctx, const ShutterReq& q, const ShutterTables& t, const ShadeOut& out)
{
    const ShutterFrame m = shutter_frame(ctx, q, t);
    const FrameArgs& f = m.f;
    const BandSet b = band_set(ctx);
    if (hipError_t e = launch_render_shutter(ctx->d_key_scenes.get(), m.single_identity, f.a, f.cam, t.c.off, t.c.loff, t.c.lens, t.c.band, t.key, b.mats,
                                             ctx->n_mats, b.weights, ctx->d_env.get(), ctx->env_w, ctx->env_h, q.c.s.n_samples, out, f.v, ctx->stream))
        return fail(ctx, RR_ERR_DEVICE, q.c.s.who, e);
    return RR_OK;
}

// both variants of rr_render_shutter, through the frame shell (params as composed_pair)
int shutter_pair(rr_context* ctx, ShutterReq q, const CallerOut& o)
{
    rr_dispatch_params p = params_or_default(q.c.s.params);
    q.c.s.params = &p;
    ShutterTables t;
    return frame_shell(ctx, q.c.s.who, q.c.s.width, q.c.s.height, o, false,
                       [&](bool have_colour) { return check_shutter(ctx, q, p, have_colour, t); },
                       [&](const ShadeOut& out) { return shutter_impl(ctx, q, t, out); });
}

// a light's v, one component, moved by a sample's light offset (lu, lv) over its shape: the arithmetic rr_host_moved_lights states
// and k_render_lit does (rr_render_lit.h), each fmaf rounded once
inline float moved_v(float v, float ex, float ey, float lu, float lv) { return std::fmaf(lv, ey, std::fmaf(lu, ex, v)); }

// a lit frame: a shutter frame over the surface tree whose samples each carry a light offset.  rec: the samples as shutter records
// (what check_shutter reads), lgt: the light offsets as the kernel takes them
struct LitReq { ShutterReq s; const rr_lit_sample* samples; };
struct LitTables { ShutterTables s; SampleOffsets lgt; rr_shutter_sample rec[RR_MAX_SAMPLES]; };

// what both variants of rr_render_lit refuse before they look at their outputs' memory: what rr_render_shutter refuses, then the
// light offsets (whether or not a shape table is set), then per sample the lights as rr_host_moved_lights moves them; fills the tables
int check_lit(rr_context* ctx, LitReq& q, rr_dispatch_params& p, bool have_colour, LitTables& t)
{
    const std::string w(q.s.c.s.who);
    const uint32_t n = q.s.c.s.n_samples;
    if (q.samples && n >= 1 && n <= RR_MAX_SAMPLES) {           // (otherwise check_shutter refuses, in its own order)
        for (uint32_t k = 0; k < n; ++k) {
            const rr_lit_sample& s = q.samples[k];
            t.rec[k] = rr_shutter_sample{ { s.offset[0], s.offset[1] }, { s.lens_offset[0], s.lens_offset[1] }, s.band, s.key, { 0u, 0u } };
        }
        q.s.samples = t.rec;
    }
    if (int r = check_shutter(ctx, q.s, p, have_colour, t.s)) return r;
    memset(&t.lgt, 0, sizeof t.lgt);
    const LightsDev& L = ctx->lights;
    const LightShapesDev& S = ctx->light_shapes;
    for (uint32_t k = 0; k < n; ++k) {
        const rr_lit_sample& s = q.samples[k];
        for (int i = 0; i < 2; ++i) {
            if (!(s.light_offset[i] >= -1.0f && s.light_offset[i] <= 1.0f))     // (NaN fails both comparisons)
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": light offsets must lie in [-1, 1]").c_str());
            t.lgt.v[2 * k + i] = s.light_offset[i];
        }
        for (uint32_t i = 0; i < L.n; ++i) {
            float v[3];                                         // (rr_host_moved_lights' arithmetic, moved_v)
            for (int ch = 0; ch < 3; ++ch) v[ch] = S.on ? moved_v(L.l[i].v[ch], S.s[i].ex[ch], S.s[i].ey[ch], s.light_offset[0], s.light_offset[1]) : L.l[i].v[ch];
            if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2]))
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a light moved by a sample's offset has a position or direction that is not finite").c_str());
            if (L.l[i].kind == RR_LIGHT_DIRECTIONAL && v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f)
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, (w + ": a directional light moved by a sample's offset has the direction zero").c_str());
        }
    }
    return RR_OK;
}

// launches a checked lit frame: out holds device pointers.  As shutter_impl, whose merge of the used keys' facts this is: nothing
// allocated, copied or waited for -- the surface table is on the device, the lights and their shapes travel by value
int lit_impl(rr_context* ctx, const LitReq& q, const LitTables& t, const ShadeOut& out)
{
    const ShutterFrame m = shutter_frame(ctx, q.s, t.s);
    const BandSet b = band_set(ctx);
    const hipError_t e = launch_render_lit(ctx->d_key_scenes.get(), m.single_identity, m.f.a, m.f.cam, t.s.c.off, t.s.c.loff, t.lgt, t.s.c.lens, t.s.c.band,
                                           t.s.key, b.mats, ctx->n_mats, b.weights, surface_launch(ctx), ctx->light_shapes, ctx->d_env.get(), ctx->env_w,
                                           ctx->env_h, q.s.c.s.n_samples, out, m.f.v, ctx->stream);
    if (e) return fail(ctx, RR_ERR_DEVICE, q.s.c.s.who, e);
    return RR_OK;
}

// both variants of rr_render_lit, through the frame shell (params as composed_pair)
int lit_pair(rr_context* ctx, LitReq q, const CallerOut& o)
{
    SamplesReq& s = q.s.c.s;
    rr_dispatch_params p = params_or_default(s.params);
    s.params = &p;
    LitTables t;
    return frame_shell(ctx, s.who, s.width, s.height, o, false,
                       [&](bool have_colour) { return check_lit(ctx, q, p, have_colour, t); },
                       [&](const ShadeOut& out) { return lit_impl(ctx, q, t, out); });
}
} // namespace

extern "C" {
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
    RR_HIP(launch_trace_rays(sc, ctx->d_rays.get(), n, ctx->d_hits.get(), &ctx->d_cnt.get()->error, query_stack(ctx), ctx->stream));
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
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    if (int r = query_impl(ctx, ctx->d_rays.get(), n, ctx->d_hits.get())) return r;
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
    return query_impl(ctx, static_cast<const rr_ray_dev*>(d_rays), n, static_cast<rr_hit_dev*>(d_hits));
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
    RR_HIP(hipMemcpyAsync(ctx->d_rays.get(), rays, (size_t)n * sizeof(rr_ray_dev), hipMemcpyHostToDevice, ctx->stream));
    if (int r = query_multi_impl(ctx, ctx->d_rays.get(), n, k, ctx->d_hits.get(), counts ? ctx->d_counts.get() : nullptr)) return r;
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
    return query_multi_impl(ctx, static_cast<const rr_ray_dev*>(d_rays), n, k, static_cast<rr_hit_dev*>(d_hits), static_cast<uint32_t*>(d_counts));
}

int rr_shade_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f, uint8_t* rgba8,
                  uint32_t* n_rays)
{
    return rays_shell(ctx, "rr_shade_rays", kShadeRays, rays, n, params, { rgba32f, rgba8, n_rays, false });
}

int rr_shade_rays_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f, void* d_rgba8,
                         void* d_n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_device", kShadeRays, d_rays, n, params, { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_samples(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                      const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return samples_pair(ctx, { "rr_render_samples", width, height, constants, params, offsets, n_samples }, kSamples, { rgba32f, rgba8, n_rays, false });
}

int rr_render_samples_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                             const float* offsets, uint32_t n_samples, void* d_rgba32f, void* d_rgba8, void* d_n_rays)
{
    return samples_pair(ctx, { "rr_render_samples_device", width, height, constants, params, offsets, n_samples }, kSamples,
                        { d_rgba32f, d_rgba8, d_n_rays, true });
}

uint64_t rr_host_adaptive_workspace_bytes(uint32_t width, uint32_t height)
{
    if (width == 0 || height == 0 || width > 32768u || height > 32768u) return 0;
    return AdaptiveWorkspace(nullptr, width, height).bytes;
}

int rr_render_adaptive(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                       const float* offsets, uint32_t n_base, uint32_t n_max, float threshold, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays,
                       uint32_t* n_taken, uint64_t* n_refined)
{
    return adaptive_pair(ctx, { { "rr_render_adaptive", width, height, constants, params, offsets, n_max }, n_base, threshold },
                         { rgba32f, rgba8, n_rays, false, n_taken }, nullptr, 0, n_refined);
}

int rr_render_adaptive_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                              const float* offsets, uint32_t n_base, uint32_t n_max, float threshold, void* d_rgba32f, void* d_rgba8, void* d_n_rays,
                              void* d_n_taken, void* d_workspace, uint64_t workspace_bytes)
{
    return adaptive_pair(ctx, { { "rr_render_adaptive_device", width, height, constants, params, offsets, n_max }, n_base, threshold },
                         { d_rgba32f, d_rgba8, d_n_rays, true, d_n_taken }, d_workspace, workspace_bytes, nullptr);
}

int rr_render_lens(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                   const float* offsets, const float* lens_offsets, uint32_t n_samples, const rr_lens* lens, float* rgba32f, uint8_t* rgba8,
                   uint32_t* n_rays)
{
    return lens_pair(ctx, { { "rr_render_lens", width, height, constants, params, offsets, n_samples }, lens_offsets, lens },
                     { rgba32f, rgba8, n_rays, false });
}

int rr_render_lens_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                          const float* offsets, const float* lens_offsets, uint32_t n_samples, const rr_lens* lens, void* d_rgba32f, void* d_rgba8,
                          void* d_n_rays)
{
    return lens_pair(ctx, { { "rr_render_lens_device", width, height, constants, params, offsets, n_samples }, lens_offsets, lens },
                     { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_spectral(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                       const float* offsets, const rr_band* bands, uint32_t n_samples, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return spectral_pair(ctx, { { "rr_render_spectral", width, height, constants, params, offsets, n_samples }, bands }, { rgba32f, rgba8, n_rays, false });
}

int rr_render_spectral_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                              const float* offsets, const rr_band* bands, uint32_t n_samples, void* d_rgba32f, void* d_rgba8, void* d_n_rays)
{
    return spectral_pair(ctx, { { "rr_render_spectral_device", width, height, constants, params, offsets, n_samples }, bands },
                         { d_rgba32f, d_rgba8, d_n_rays, true });
}

float rr_host_expf_neg(float x) { return rr_expf_neg(x); }

int rr_set_materials(rr_context* ctx, const rr_material* mats, uint32_t n)
{
    if (int r = use_device(ctx)) return r;
    if (n == 0) { ctx->n_mats = 0; ctx->n_bands = 0; return RR_OK; }
    if (!mats) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_materials: null table");
    if (n > 0x1000000u) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_materials: a hit-group index has 24 bits, so at most 16 777 216 materials");
    std::vector<MatDev> rows(n);
    for (uint32_t i = 0; i < n; ++i) {
        const rr_material& m = mats[i];
        if (!std::isfinite(m.ior) || !(m.ior > 0.0f)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_materials: every ior must be finite and > 0");
        MatDev& o = rows[i];
        memset(&o, 0, sizeof o);
        o.ior = m.ior; o.inv_ior = inv_ior_of(m.ior);
        for (int ch = 0; ch < 3; ++ch) {
            if (!std::isfinite(m.sigma_a[ch]) || !(m.sigma_a[ch] >= 0.0f))
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_materials: every sigma_a must be finite and >= 0");
            o.sigma[ch] = m.sigma_a[ch];
        }
    }
    // the old table stays in force until the new one is whole: launches in flight on the stream read it, and the copy is ordered
    // behind them (grow waits for the stream before it lets the old buffer go)
    // a band set (rr_set_material_bands) was made from the old table, whose row count may differ: it goes with it.  What
    // rr_render_composed weights its one band with while no set is in force is made here, with the first table: its launch
    // allocates nothing
    ctx->n_bands = 0;
    if (n > ctx->d_mats.size()) {
        ctx->n_mats = 0;
        if (int r = ctx->d_mats.grow(ctx, n)) return r;
    }
    if (!ctx->d_band_one.size()) {
        static const float one[3] = { 1.0f, 1.0f, 1.0f };
        RR_HIP(ctx->d_band_one.alloc(3));
        RR_HIP(hipMemcpyAsync(ctx->d_band_one.get(), one, sizeof one, hipMemcpyHostToDevice, ctx->stream));
    }
    RR_HIP(hipMemcpyAsync(ctx->d_mats.get(), rows.data(), (size_t)n * sizeof(MatDev), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));   // (rows goes away with this call)
    ctx->mats_host.swap(rows);
    ctx->n_mats = n;
    return RR_OK;
}

int rr_set_material_bands(rr_context* ctx, const float* iors, const float* weights, uint32_t n_bands)
{
    if (int r = use_device(ctx)) return r;
    if (n_bands == 0) { ctx->n_bands = 0; return RR_OK; }
    if (!ctx->n_mats) return fail(ctx, RR_ERR_STATE, "rr_set_material_bands: set a material table first (rr_set_materials)");
    if (!iors) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_material_bands: null iors");
    if (n_bands > RR_MAX_SAMPLES) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_material_bands: need n_bands <= 64");
    const uint32_t n_rows = ctx->n_mats;
    const size_t n = (size_t)n_bands * n_rows;
    std::vector<MatDev> rows(n);
    std::vector<float> w((size_t)n_bands * 3, 1.0f);
    for (size_t i = 0; i < n; ++i) {                            // band i / n_rows, row i % n_rows: the table's row with the band's index
        if (!std::isfinite(iors[i]) || !(iors[i] > 0.0f)) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_material_bands: every ior must be finite and > 0");
        rows[i] = ctx->mats_host[i % n_rows];
        rows[i].ior = iors[i]; rows[i].inv_ior = inv_ior_of(iors[i]);
    }
    if (weights) for (size_t i = 0; i < w.size(); ++i) {
        if (!std::isfinite(weights[i])) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_material_bands: every weight must be finite");
        w[i] = weights[i];
    }
    // as rr_set_materials: the set in force stays until the new one is whole, and the copies are ordered behind what is in flight
    if (n > ctx->d_band_mats.size()) {
        ctx->n_bands = 0;
        if (int r = ctx->d_band_mats.grow(ctx, n)) return r;
    }
    if (w.size() > ctx->d_band_w.size()) {
        ctx->n_bands = 0;
        if (int r = ctx->d_band_w.grow(ctx, w.size())) return r;
    }
    RR_HIP(hipMemcpyAsync(ctx->d_band_mats.get(), rows.data(), n * sizeof(MatDev), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(hipMemcpyAsync(ctx->d_band_w.get(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));   // (rows and w go away with this call)
    ctx->n_bands = n_bands;
    return RR_OK;
}

int rr_shade_rays_materials(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f, uint8_t* rgba8,
                            uint32_t* n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_materials", kShadeMaterials, rays, n, params, { rgba32f, rgba8, n_rays, false });
}

int rr_shade_rays_materials_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f, void* d_rgba8,
                                   void* d_n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_materials_device", kShadeMaterials, d_rays, n, params, { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_materials(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                        const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return samples_pair(ctx, { "rr_render_materials", width, height, constants, params, offsets, n_samples }, kMaterials, { rgba32f, rgba8, n_rays, false });
}

int rr_render_materials_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                               const float* offsets, uint32_t n_samples, void* d_rgba32f, void* d_rgba8, void* d_n_rays)
{
    return samples_pair(ctx, { "rr_render_materials_device", width, height, constants, params, offsets, n_samples }, kMaterials,
                        { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_shade_rays_nested(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f, uint8_t* rgba8,
                         uint32_t* n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_nested", kShadeNested, rays, n, params, { rgba32f, rgba8, n_rays, false });
}

int rr_shade_rays_nested_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f, void* d_rgba8,
                                void* d_n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_nested_device", kShadeNested, d_rays, n, params, { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_nested(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                     const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return samples_pair(ctx, { "rr_render_nested", width, height, constants, params, offsets, n_samples }, kNested, { rgba32f, rgba8, n_rays, false });
}

int rr_render_nested_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                            const float* offsets, uint32_t n_samples, void* d_rgba32f, void* d_rgba8, void* d_n_rays)
{
    return samples_pair(ctx, { "rr_render_nested_device", width, height, constants, params, offsets, n_samples }, kNested,
                        { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_set_surfaces(rr_context* ctx, const rr_surface* rows, uint32_t n)
{
    if (int r = use_device(ctx)) return r;
    if (n == 0) { ctx->n_surfs = 0; return RR_OK; }
    if (!rows) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_surfaces: null table");
    if (n > 0x1000000u) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_surfaces: a hit-group index has 24 bits, so at most 16 777 216 rows");
    std::vector<SurfDev> dev(n);
    for (uint32_t i = 0; i < n; ++i) {
        const rr_surface& s = rows[i];
        if (s.kind != RR_SURFACE_GLASS && s.kind != RR_SURFACE_OPAQUE) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_surfaces: unknown surface kind");
        SurfDev& o = dev[i];
        memset(&o, 0, sizeof o);
        o.kind = s.kind;
        for (int ch = 0; ch < 3; ++ch) {
            if (!std::isfinite(s.albedo[ch]) || !(s.albedo[ch] >= 0.0f) || !std::isfinite(s.specular[ch]) || !(s.specular[ch] >= 0.0f))
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_surfaces: every albedo and specular must be finite and >= 0");
            if (!std::isfinite(s.emission[ch])) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_surfaces: every emission must be finite");
            o.albedo[ch] = s.albedo[ch]; o.emission[ch] = s.emission[ch]; o.specular[ch] = s.specular[ch];
        }
    }
    // as rr_set_materials: the table in force stays until the new one is whole, and the copy is ordered behind what is in flight
    if (n > ctx->d_surfs.size()) {
        ctx->n_surfs = 0;
        if (int r = ctx->d_surfs.grow(ctx, n)) return r;
    }
    RR_HIP(hipMemcpyAsync(ctx->d_surfs.get(), dev.data(), (size_t)n * sizeof(SurfDev), hipMemcpyHostToDevice, ctx->stream));
    RR_HIP(hipStreamSynchronize(ctx->stream));   // (dev goes away with this call)
    ctx->n_surfs = n;
    return RR_OK;
}

int rr_set_lights(rr_context* ctx, const rr_light* lights, uint32_t n, const float ambient[3])
{
    if (int r = use_device(ctx)) return r;
    if (n > RR_MAX_LIGHTS) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: need n <= RR_MAX_LIGHTS (8)");
    if (n && !lights) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: null lights");
    LightsDev t;
    memset(&t, 0, sizeof t);
    for (uint32_t i = 0; i < n; ++i) {
        const rr_light& l = lights[i];
        if (l.kind != RR_LIGHT_DIRECTIONAL && l.kind != RR_LIGHT_POINT) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: unknown light kind");
        if (l.shadow_mask > 0xffu) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: an instance mask has 8 bits, so shadow_mask <= 0xff");
        for (int ch = 0; ch < 3; ++ch) {
            if (!std::isfinite(l.v[ch]) || !std::isfinite(l.radiance[ch]))
                return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: every direction, position and radiance must be finite");
            t.l[i].v[ch] = l.v[ch]; t.l[i].radiance[ch] = l.radiance[ch];
        }
        if (l.kind == RR_LIGHT_DIRECTIONAL && l.v[0] == 0.0f && l.v[1] == 0.0f && l.v[2] == 0.0f)
            return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: a directional light needs a direction that is not zero");
        t.l[i].kind = l.kind; t.l[i].shadow_mask = l.shadow_mask;
    }
    for (int ch = 0; ch < 3; ++ch) {
        if (ambient && !std::isfinite(ambient[ch])) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_lights: the ambient term must be finite");
        t.ambient[ch] = ambient ? ambient[ch] : 0.0f;
    }
    t.n = n;
    // the set travels by value with every launch: those in flight hold their own copy.  Waiting keeps the setters alike
    RR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->lights = t;
    ctx->light_shapes = LightShapesDev{};                       // (row i belonged with the old light i)
    return RR_OK;
}

static_assert(SHADOW_MAX_STEPS == RR_SHADOW_MAX_STEPS, "the launchers' cap is the header's");
int rr_set_shadow_steps(rr_context* ctx, uint32_t k)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    if (k > RR_SHADOW_MAX_STEPS) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_shadow_steps: need k <= RR_SHADOW_MAX_STEPS (16)");
    // the cap travels by value with every launch, so nothing is waited for: a launch in flight keeps the one it was given
    ctx->shadow_steps = k;
    return RR_OK;
}

int rr_get_shadow_steps(rr_context* ctx, uint32_t* k)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    if (!k) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_get_shadow_steps: null k");
    *k = ctx->shadow_steps;
    return RR_OK;
}

int rr_shade_rays_surfaces(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f, uint8_t* rgba8,
                           uint32_t* n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_surfaces", kShadeSurfaces, rays, n, params, { rgba32f, rgba8, n_rays, false });
}

int rr_shade_rays_surfaces_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f, void* d_rgba8,
                                  void* d_n_rays)
{
    return rays_shell(ctx, "rr_shade_rays_surfaces_device", kShadeSurfaces, d_rays, n, params, { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_surfaces(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                       const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return samples_pair(ctx, { "rr_render_surfaces", width, height, constants, params, offsets, n_samples }, kSurfaces, { rgba32f, rgba8, n_rays, false });
}

int rr_render_surfaces_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                              const float* offsets, uint32_t n_samples, void* d_rgba32f, void* d_rgba8, void* d_n_rays)
{
    return samples_pair(ctx, { "rr_render_surfaces_device", width, height, constants, params, offsets, n_samples }, kSurfaces,
                        { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_composed(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                       const rr_composed_sample* samples, uint32_t n_samples, const rr_lens* lens, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return composed_pair(ctx, { { "rr_render_composed", width, height, constants, params, nullptr, n_samples }, samples, lens },
                         { rgba32f, rgba8, n_rays, false });
}

int rr_render_composed_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                              const rr_composed_sample* samples, uint32_t n_samples, const rr_lens* lens, void* d_rgba32f, void* d_rgba8,
                              void* d_n_rays)
{
    return composed_pair(ctx, { { "rr_render_composed_device", width, height, constants, params, nullptr, n_samples }, samples, lens },
                         { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_render_shutter(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                      const rr_shutter_sample* samples, uint32_t n_samples, const rr_lens* lens, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return shutter_pair(ctx, { { { "rr_render_shutter", width, height, constants, params, nullptr, n_samples }, nullptr, lens }, samples },
                        { rgba32f, rgba8, n_rays, false });
}

int rr_render_shutter_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                             const rr_shutter_sample* samples, uint32_t n_samples, const rr_lens* lens, void* d_rgba32f, void* d_rgba8,
                             void* d_n_rays)
{
    return shutter_pair(ctx, { { { "rr_render_shutter_device", width, height, constants, params, nullptr, n_samples }, nullptr, lens }, samples },
                        { d_rgba32f, d_rgba8, d_n_rays, true });
}

int rr_set_light_shapes(rr_context* ctx, const rr_light_shape* shapes, uint32_t n)
{
    if (int r = use_device(ctx)) return r;
    LightShapesDev t;
    memset(&t, 0, sizeof t);
    if (n) {
        if (!shapes) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_light_shapes: null shapes");
        if (n != ctx->lights.n) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_light_shapes: need one shape per light in force (rr_set_lights), or n == 0");
        for (uint32_t i = 0; i < n; ++i) {
            const rr_light_shape& s = shapes[i];
            if (s.pad[0] || s.pad[1]) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_light_shapes: a shape's pad must be zero");
            for (int ch = 0; ch < 3; ++ch) {
                if (!std::isfinite(s.ex[ch]) || !std::isfinite(s.ey[ch])) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_set_light_shapes: every ex and ey must be finite");
                t.s[i].ex[ch] = s.ex[ch]; t.s[i].ey[ch] = s.ey[ch];
            }
        }
        t.on = 1u;
    }
    // as the lights: the table travels by value with every launch, and waiting keeps the setters alike
    RR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->light_shapes = t;
    return RR_OK;
}

int rr_host_moved_lights(const rr_light* lights, const rr_light_shape* shapes, uint32_t n, float lu, float lv, rr_light* out)
{
    if (n && (!lights || !out)) return RR_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n; ++i) {
        rr_light m = lights[i];
        if (shapes) for (int ch = 0; ch < 3; ++ch) m.v[ch] = moved_v(m.v[ch], shapes[i].ex[ch], shapes[i].ey[ch], lu, lv);
        out[i] = m;
    }
    return RR_OK;
}

int rr_render_lit(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                  const rr_lit_sample* samples, uint32_t n_samples, const rr_lens* lens, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays)
{
    return lit_pair(ctx, { { { { "rr_render_lit", width, height, constants, params, nullptr, n_samples }, nullptr, lens }, nullptr }, samples },
                    { rgba32f, rgba8, n_rays, false });
}

int rr_render_lit_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants, const rr_dispatch_params* params,
                         const rr_lit_sample* samples, uint32_t n_samples, const rr_lens* lens, void* d_rgba32f, void* d_rgba8, void* d_n_rays)
{
    return lit_pair(ctx, { { { { "rr_render_lit_device", width, height, constants, params, nullptr, n_samples }, nullptr, lens }, nullptr }, samples },
                    { d_rgba32f, d_rgba8, d_n_rays, true });
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
} // extern "C"
