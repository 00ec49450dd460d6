// rr_capi_build.cpp -- acceleration structures: BLAS build and refit, vertex updates, TLAS build and refit, the scene pools
// (the two BuildRaytracingAccelerationStructure calls, RefractionDemo.cpp:277-356).
#include "rr_context.h"

namespace {
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
    RR_HIP(launch_quantize_nodes(m.qnodes.get(), m.nodes.get(), m.n_nodes(), m.grid, 0, 0, ctx->stream));
    m.stale = false;
    ++m.version;
    return RR_OK;
}

// ALLOW_UPDATE builds over n primitives keep what a refit needs: the links of the nodes and their arrival counters, zeroed
int alloc_refit_state(rr_context* ctx, uint32_t n, DevBuf<int32_t>& links, DevBuf<uint32_t>& visit)
{
    if (n <= 1) return RR_OK;
    RR_HIP(links.alloc(2 * (size_t)n - 1));
    RR_HIP(visit.alloc(n - 1));
    RR_HIP(hipMemsetAsync(visit.get(), 0, (size_t)(n - 1) * sizeof(uint32_t), ctx->stream));
    return RR_OK;
}

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
        o.material = d.hitgroup_flags & 0xffffffu;
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
        RR_HIP_MSG(launch_quantize_nodes(ctx->d_pool_qnodes.get() + no, m.nodes.get(), m.n_nodes(), m.grid, no, to, ctx->stream), what);
        RR_HIP_MSG(hipMemcpyAsync(ctx->d_pool_tris.get() + to, m.tris.get(), (size_t)m.n_tris * sizeof(TriRec), hipMemcpyDeviceToDevice, ctx->stream), what);
        RR_HIP_MSG(hipMemcpyAsync(ctx->d_pool_nrms.get() + to, m.nrms.get(), (size_t)m.n_tris * sizeof(NrmRec), hipMemcpyDeviceToDevice, ctx->stream), what);
        ctx->pool_version[mi] = m.version;
    }
    return RR_OK;
}

// The shared run of a TLAS build and update (`what` names the step in a failure): the scene grid from the root the builder or
// the refit left, the top level quantized, the BLASes pooled
int pool_tlas(rr_context* ctx, const char* what, uint32_t n)
{
    BvhNode root;
    RR_HIP_MSG(hipMemcpyAsync(&root, ctx->d_pool_nodes.get(), sizeof root, hipMemcpyDeviceToHost, ctx->stream), what);
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), what);
    scene_from_root(ctx, root);
    RR_HIP_MSG(launch_quantize_nodes(ctx->d_pool_qnodes.get(), ctx->d_pool_nodes.get(), n > 1 ? n - 1 : 1, ctx->scene_grid, 0, 0, ctx->stream), what);
    if (int r = repool(ctx, what)) return r;
    RR_HIP_MSG(hipStreamSynchronize(ctx->stream), what);
    return RR_OK;
}

// what a successful TLAS build or update leaves in the context
int finish_tlas(rr_context* ctx, const rr_instance_desc* instances, uint32_t n, const InstDev& inst0, float scene_scale)
{
    ctx->inst_host.assign(instances, instances + n);
    ctx->n_insts = n;
    ctx->scene_scale = scene_scale;
    ctx->max_material = 0;
    for (uint32_t i = 0; i < n; ++i) ctx->max_material = std::max(ctx->max_material, instances[i].hitgroup_flags & 0xffffffu);
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
    RR_HIP_MSG(hipMemcpyAsync(ctx->d_insts.get(), host.data(), (size_t)n * sizeof(InstDev), hipMemcpyHostToDevice, ctx->stream), "TLAS update");
    RR_HIP_MSG(hipMemcpyAsync(d_xb.get(), xb.data(), xb.size() * 4, hipMemcpyHostToDevice, ctx->stream), "TLAS update");
    RR_HIP_MSG(launch_refit_tlas(ctx->d_insts.get(), d_xb.get(), n, ctx->d_pool_nodes.get(), ctx->d_tlas_links.get(), ctx->d_tlas_visit.get(), ctx->stream),
               "TLAS update");
    if (int r = pool_tlas(ctx, "TLAS update", n)) return r;
    return finish_tlas(ctx, instances, n, host[0], scene_scale);
}
} // namespace

extern "C" {
int rr_build_blas(rr_context* ctx, uint32_t mesh_id) { return rr_build_blas_ex(ctx, mesh_id, RR_BUILD_PREFER_FAST_TRACE); }

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
    RR_HIP(m.nodes.alloc(m.n_nodes()));
    RR_HIP(m.qnodes.alloc(m.n_nodes()));
    RR_HIP(m.tris.alloc(n));
    RR_HIP(m.nrms.alloc(n));
    if (keep) {
        if (int r = ensure_upd(ctx, m)) return r;
        if (int r = alloc_refit_state(ctx, n, m.links, m.visit)) return r;
    }
    s.b.nodes = m.nodes.get();
    bool clustered = (flags & RR_BUILD_PREFER_FAST_TRACE) && !(flags & RR_BUILD_PREFER_FAST_BUILD) && n > 1 && n <= PLOC_MAX_PRIMS;
    uint32_t sb[6], depth = 0;
    for (;;) {
        // (the setup again in front of a second pass: k_ploc used visit[] as scratch, k_refit needs it zero, and depth is a maximum)
        RR_HIP(launch_tri_setup(m.d_verts.get(), m.d_idx.get(), n, s.b, ctx->stream));
        if (clustered)
            RR_HIP(launch_ploc(s.b, ctx->stream));          // clustered hierarchy (fewer node visits)
        else
            RR_HIP(launch_lbvh(s.b, ctx->stream));          // Karras radix tree (fastest build, any size)
        if (keep) RR_HIP(launch_keep_links(s.b, m.links.get(), ctx->stream));
        RR_HIP(launch_pack_tris(m.d_verts.get(), m.d_idx.get(), s.b, m.tris.get(), m.nrms.get(), ctx->stream));
        RR_HIP(hipMemcpyAsync(sb, s.b.scene_box, sizeof sb, hipMemcpyDeviceToHost, ctx->stream));
        RR_HIP(hipMemcpyAsync(&depth, s.b.depth, 4, hipMemcpyDeviceToHost, ctx->stream));
        RR_HIP(hipStreamSynchronize(ctx->stream));
        // Where every merged-box area ties (coincident or same-box triangles) the clustered builder merges one pair a round
        // and its tree is a chain as deep as the mesh is large: past the 64-entry stack the radix tree, whose depth the key
        // length bounds, is built instead -- nodes, links and leaf records are all written again, so nothing of the chain stays
        if (!clustered || depth <= 64) break;
        clustered = false;
    }
    set_bounds(m, sb);
    m.depth = depth;
    RR_HIP(launch_quantize_nodes(m.qnodes.get(), m.nodes.get(), m.n_nodes(), m.grid, 0, 0, ctx->stream));
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
        n_pool_nodes += m.n_nodes();
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
    if (keep) if (int r = alloc_refit_state(ctx, n, ctx->d_tlas_links, ctx->d_tlas_visit)) return r;
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
    RR_HIP_MSG(hipMemcpyAsync(&depth, s.b.depth, 4, hipMemcpyDeviceToHost, ctx->stream), "TLAS build");
    if (int r = pool_tlas(ctx, "TLAS build", n)) return r;
    ctx->n_pool_tris = n_pool_tris; ctx->n_pool_nodes = n_pool_nodes;
    ctx->tlas_depth = depth;
    ctx->tlas_refittable = keep;
    return finish_tlas(ctx, instances, n, host[0], scene_scale);
}
} // extern "C"
