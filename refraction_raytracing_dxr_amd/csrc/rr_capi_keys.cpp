// rr_capi_keys.cpp -- the scene keys of shutter frames: rr_capture_scene_key, rr_release_scene_key, rr_scene_key_info.  A key is a
// frozen copy of the scene a render call would trace (rr_context.h SceneKey); rr_render_shutter (rr_capi_query.cpp) traces in them.
#include "rr_context.h"

namespace {
// grows a key's buffer to n elements where it holds fewer (grow waits for the context's stream: a frame in flight may read the
// old one); n == 0 keeps what is there
template <class T> int fit(rr_context* ctx, DevBuf<T>& b, size_t n) { return n > b.size() ? b.grow(ctx, n) : RR_OK; }

template <class T> hipError_t copy_d2d(rr_context* ctx, DevBuf<T>& dst, const T* src, size_t n)
{
    return n ? hipMemcpyAsync(dst.get(), src, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
}
} // namespace

extern "C" {
int rr_capture_scene_key(rr_context* ctx, uint32_t key)
{
    if (int r = use_device(ctx)) return r;
    if (key >= RR_MAX_SCENE_KEYS) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_capture_scene_key: key must be below RR_MAX_SCENE_KEYS (16)");
    if (!ctx->tlas_built) return fail(ctx, RR_ERR_STATE, "rr_capture_scene_key: build the BLAS and TLAS first");
    SceneKey& k = ctx->keys[key];
    const bool single = ctx->single_identity;
    const MeshRes* const m0 = single ? &ctx->meshes[(size_t)ctx->inst_host[0].blas] : nullptr;
    const size_t n_insts = ctx->n_insts, n_nodes = ctx->n_pool_nodes, n_tris = ctx->n_pool_tris;
    const size_t n_nodes0 = m0 ? m0->n_nodes() : 0, n_tris0 = m0 ? m0->n_tris : 0;
    // the key is empty from here until it is whole again: a failure below leaves it released
    k.captured = false;
    int r = RR_OK;
    if (!ctx->d_key_scenes.size()) {
        if ((r = ctx->d_key_scenes.grow(ctx, RR_MAX_SCENE_KEYS)) == RR_OK)
            if (hipMemsetAsync(ctx->d_key_scenes.get(), 0, RR_MAX_SCENE_KEYS * sizeof(KeyDev), ctx->stream) != hipSuccess) r = RR_ERR_DEVICE;
    }
    if (!r) r = fit(ctx, k.insts, n_insts);
    if (!r) r = fit(ctx, k.pool_qnodes, n_nodes);
    if (!r) r = fit(ctx, k.pool_tris, n_tris);
    if (!r) r = fit(ctx, k.pool_nrms, n_tris);
    if (!r) r = fit(ctx, k.qnodes0, n_nodes0);
    if (!r) r = fit(ctx, k.tris0, n_tris0);
    if (!r) r = fit(ctx, k.nrms0, n_tris0);
    if (r) { k.release(); return r; }
    // device to device on the context's stream: behind every build, refit and vertex update issued so far, in front of every
    // frame issued from now on
    hipError_t e = copy_d2d(ctx, k.insts, ctx->d_insts.get(), n_insts);
    if (e == hipSuccess) e = copy_d2d(ctx, k.pool_qnodes, ctx->d_pool_qnodes.get(), n_nodes);
    if (e == hipSuccess) e = copy_d2d(ctx, k.pool_tris, ctx->d_pool_tris.get(), n_tris);
    if (e == hipSuccess) e = copy_d2d(ctx, k.pool_nrms, ctx->d_pool_nrms.get(), n_tris);
    if (e == hipSuccess && m0) e = copy_d2d(ctx, k.qnodes0, m0->qnodes.get(), n_nodes0);
    if (e == hipSuccess && m0) e = copy_d2d(ctx, k.tris0, m0->tris.get(), n_tris0);
    if (e == hipSuccess && m0) e = copy_d2d(ctx, k.nrms0, m0->nrms.get(), n_tris0);
    // the record: the live scene's, pointed at the key's buffers; never an environment map (it is the context's at the launch)
    KeyDev& h = ctx->key_host[key];
    memset(&h, 0, sizeof h);
    fill_scene(ctx, h.sc);
    if (m0) { h.sc.blas0.nodes = k.qnodes0.get(); h.sc.blas0.tris = k.tris0.get(); h.sc.blas0.nrms = k.nrms0.get(); }
    h.sc.pool_nodes = k.pool_qnodes.get(); h.sc.pool_tris = k.pool_tris.get(); h.sc.pool_nrms = k.pool_nrms.get();
    h.sc.insts = k.insts.get();
    h.sc.env = nullptr; h.sc.env_w = 0; h.sc.env_h = 0;
    h.mat0 = ctx->inst_host.empty() ? 0u : ctx->inst_host[0].hitgroup_flags & 0xffffffu;
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_key_scenes.get() + key, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { k.release(); return fail(ctx, RR_ERR_DEVICE, "rr_capture_scene_key", e); }
    k.facts = scene_facts(ctx);
    k.facts.lds_fits = false;
    memcpy(k.bounds, ctx->scene_bounds, sizeof k.bounds);
    k.n_insts = ctx->n_insts;
    k.n_tris = single ? m0->n_tris : ctx->n_pool_tris;
    k.max_material = ctx->max_material;
    k.mat0 = h.mat0;
    k.captured = true;
    return RR_OK;
}

int rr_release_scene_key(rr_context* ctx, uint32_t key)
{
    if (int r = use_device(ctx)) return r;
    if (key >= RR_MAX_SCENE_KEYS && key != RR_ALL_SCENE_KEYS)
        return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_release_scene_key: key must be below RR_MAX_SCENE_KEYS (16) or RR_ALL_SCENE_KEYS");
    RR_HIP(hipStreamSynchronize(ctx->stream));                  // a frame in flight may read the key
    for (uint32_t k = 0; k < RR_MAX_SCENE_KEYS; ++k)
        if (key == RR_ALL_SCENE_KEYS || key == k) ctx->keys[k].release();
    return RR_OK;
}

int rr_scene_key_info(rr_context* ctx, uint32_t key, struct rr_scene_key_info* out)
{
    if (!ctx) return RR_ERR_INVALID_ARGUMENT;
    if (key >= RR_MAX_SCENE_KEYS || !out) return fail(ctx, RR_ERR_INVALID_ARGUMENT, "rr_scene_key_info: key must be below RR_MAX_SCENE_KEYS (16), out not null");
    memset(out, 0, sizeof *out);
    const SceneKey& k = ctx->keys[key];
    if (!k.captured) return RR_OK;
    out->captured = 1u;
    out->top_level = k.facts.single_identity ? 0u : 1u;
    out->n_instances = k.n_insts;
    out->n_triangles = k.n_tris;
    memcpy(out->bounds, k.bounds, sizeof out->bounds);
    out->stack_need = k.facts.need;
    out->max_material = k.max_material;
    out->bytes = k.bytes();
    return RR_OK;
}
} // extern "C"
