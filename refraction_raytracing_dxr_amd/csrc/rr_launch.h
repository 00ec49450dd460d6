// rr_launch.h -- host-callable launchers of the gfx950 kernels (implemented in the .hip files)
#pragma once
#include <hip/hip_runtime.h>
#include "rr_types.h"
#include "rr_choice.h"
#include "host/rr_host_lens.h"

namespace rr {

// device twins of rr_ray / rr_hit (include/rrdxr.h), same layout
struct alignas(16) rr_ray_dev { float origin[3]; float tmin; float dir[3]; float tmax; uint32_t flags; uint32_t instance_mask; uint32_t pad[2]; };
struct rr_hit_dev { float t, u, v; uint32_t prim, inst, hit; };
static_assert(sizeof(rr_ray_dev) == 48 && sizeof(rr_hit_dev) == 24, "ABI layout");

// ---- rr_render_fused.hip
hipError_t launch_render_fused(const SceneDev& sc, const DispatchDev& a, int stack, int pend, bool stats, hipStream_t s,
                               bool stack16 = false);
// the instantiation the calling thread's last launch_render_* call launched, e.g. "k_render_fused<19, 2, false, false, false, unsigned int, 0>"
// (a launch without blocks launches nothing and leaves the name as it was); every render launcher sets it
const char* last_render_kernel_name();
void set_render_kernel_name(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// ---- rr_render_paths.hip
// launches of one or two slices: four lanes per pixel inside the scene's screen rectangle (k_render_paths)
hipError_t launch_render_paths(const SceneDev& sc, const DispatchDev& a, int stack, bool stats, hipStream_t s);
// ---- rr_render_lds.hip
// BLAS nodes in LDS, persistent workgroups (single identity instance whose node array fits: lds_kernel_shape() >= 0)
// shapes (waves per workgroup x workgroups per CU): 0 = 12x2 (the product shape), 1 = 16x2, 2 = 16x1 (experiments:
// RR_DEBUG_SHAPE = first shape to consider); -1: the node array does not fit
int lds_kernel_shape(uint32_t node_bytes, uint32_t stack_entries, size_t* lds_bytes, int min_shape = 0);
hipError_t launch_render_lds(const SceneDev& sc, const DispatchDev& a, LdsDispatch q, int n_cus, bool stats, hipStream_t s, int min_shape = 0);
// ---- rr_render_stream.hip: one kernel per ray generation, rays in HBM queues, lanes refilled as their rays end (two-level scenes)
hipError_t launch_render_stream(const SceneDev& sc, const DispatchDev& a, const StreamDev& s, int stack, uint32_t n_wg, bool stats, hipStream_t st);
// ---- rr_query.hip: one stage on caller input
hipError_t launch_env_lookup(const SceneDev& sc, const float* dirs, uint32_t n, float* rgb, hipStream_t s);
hipError_t launch_trace_rays(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t* err,
                             int stack, hipStream_t s);
// the query kernels (rr_query_rays[_device]): instance masks and per-lane first-hit termination; inst0_mask: the InstanceMask of
// a single-identity scene's instance
hipError_t launch_query_rays(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, rr_hit_dev* hits, uint32_t inst0_mask, int stack,
                             hipStream_t s);
// ---- rr_query_multi.hip: multi-hit queries (rr_query_rays_multi[_device]): the first k accepted triangles per ray, k slots of
// hits per ray; counts (may be null) receives the number of accepted triangles.  0 <= k <= RR_QUERY_MULTI_MAX_K, k == 0 only with counts
constexpr uint32_t RR_QUERY_MULTI_MAX_K = 16;
hipError_t launch_query_multi(const SceneDev& sc, const rr_ray_dev* rays, uint32_t n, uint32_t k, rr_hit_dev* hits, uint32_t* counts,
                              uint32_t inst0_mask, int stack, hipStream_t s);
// ---- the ray-tree launchers (rr_shade_rays.hip ... rr_render_adaptive.hip below) end in the same three parameters: out, the
// rasters (or, for caller rays, arrays of n entries) to write, any of them null; v, the scene's FusedVariant (rr_choice.h), which
// for_tree_variant (there) maps to the instantiation launched -- v.stack > 64 or v.pend > 8 is hipErrorInvalidValue; the stream
struct ShadeOut { float4* f32; uint32_t* rgba8; uint32_t* n_rays; };
// One launch of a ray-tree kernel template <STACK, PEND, TLAS, E>: the instantiation of FusedVariant v through the ladder, `groups`
// workgroups of 256 lanes with that instantiation's LDS on stream s; the value is the launch's hipError_t.  (A function template
// cannot be handed to a function, hence a macro.)
#define RR_LAUNCH_TREE_KERNEL(kernel, single_identity, v, groups, s, ...)                                                                      \
    for_tree_variant((single_identity), (v), [&](auto t_) {                                                                                    \
        using T_ = decltype(t_);                                                                                                               \
        hipLaunchKernelGGL((kernel<T_::stack, T_::pend, T_::tlas, typename T_::entry>), dim3(groups), dim3(256), T_::lds_bytes, (s), __VA_ARGS__); \
        return hipGetLastError();                                                                                                              \
    })
// ---- rr_shade_rays.hip: radiance queries (rr_shade_rays[_device]): the render kernels' ray tree on caller rays.  a: the fields
// shade_ray and store_pixel read
hipError_t launch_shade_rays(const SceneDev& sc, const DispatchDev& a, const rr_ray_dev* rays, uint32_t n, const ShadeOut& out, FusedVariant v,
                             hipStream_t s);
// ---- rr_render_samples.hip: supersampled frames (rr_render_samples[_device]): n_samples primary rays per pixel of an a.W x a.H
// frame through the sub-pixel positions off (pixel units), each with the ray tree of a radiance query, averaged in the kernel.
// a: the fields shade_ray and store_pixel read, W, H, tmin_p, tmax_p and the scene's screen rectangle hx0..hy1; f32 / rgba8 /
// n_rays: W * H rasters.  The offsets travel as a kernel argument: 512 bytes
struct SampleOffsets { static constexpr uint32_t MAX = 64; float v[2 * MAX]; };     // x0, y0, x1, y1, ...
// What every frame launcher checks -- W, H in 1..32768, n_samples in 1..SampleOffsets::MAX, v as above: false is
// hipErrorInvalidValue -- and the frame's raster of 8x8 blocks, four of them to a workgroup
struct FrameBlocks { uint32_t blocks_x, n_blocks, groups; };
inline bool frame_blocks(const DispatchDev& a, uint32_t n_samples, FusedVariant v, FrameBlocks& fb)
{
    if (a.W == 0 || a.H == 0 || a.W > 32768u || a.H > 32768u || n_samples == 0 || n_samples > SampleOffsets::MAX || v.stack > 64 || v.pend > 8) return false;
    fb.blocks_x = (a.W + 7u) / 8u; fb.n_blocks = fb.blocks_x * ((a.H + 7u) / 8u);           // <= 4096 * 4096
    fb.groups = (fb.n_blocks + 3u) / 4u;
    return true;
}
hipError_t launch_render_samples(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, uint32_t n_samples,
                                 const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_lens.hip: thin-lens frames (rr_render_lens[_device]): launch_render_samples with every sample's ray starting on
// the lens (LensDev, host/rr_host_lens.h) at lens offset loff[s], in units of the radius, towards the focal-plane point of pixel
// offset off[s]; lens.pinhole: the rays of launch_render_samples.  a.hx0..hy1: the scene's rectangle for the lens
// (rr_host_lens_screen_rect).  Both tables and the lens travel as kernel arguments: 1056 bytes
hipError_t launch_render_lens(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const SampleOffsets& loff,
                              const LensDev& lens, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_spectral.hip: spectral frames (rr_render_spectral[_device]): launch_render_samples with sample k shaded with the
// index of refraction of band k instead of a.ior / a.inv_ior, and its colour weighted per channel before the resolve's sum:
// sum = w_0 * c_0, then sum + w_k * c_k in sample order, / n_samples.  inv_ior[k] = inv_ior_of(ior[k]) (rr_types.h), filled by the
// host.  The band table travels as a kernel argument beside the offsets: 1280 bytes
struct BandTable { static constexpr uint32_t MAX = SampleOffsets::MAX; float ior[MAX]; float inv_ior[MAX]; float weight[MAX][3]; };
hipError_t launch_render_spectral(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const BandTable& bands,
                                  uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_materials.hip: per-instance glass (rr_shade_rays_materials[_device], rr_render_materials[_device]):
// launch_shade_rays and launch_render_samples with the ray tree of rr_render_materials.h -- an RGB path weight, the index of
// refraction of the hit instance's material instead of a.ior / a.inv_ior, and Beer-Lambert absorption over the path inside the
// glass.  mats: the context's table in device memory (rows of 32 bytes), which every InstDev::material of the scene indexes; mat0:
// the index of instance 0, used where the scene skips the top level.  mats == nullptr is hipErrorInvalidValue
hipError_t launch_shade_rays_mat(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, uint32_t mat0, const rr_ray_dev* rays, uint32_t n,
                                 const ShadeOut& out, FusedVariant v, hipStream_t s);
hipError_t launch_render_materials(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                   uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_nested.hip: nested media (rr_shade_rays_nested[_device], rr_render_nested[_device]): launch_shade_rays_mat and
// launch_render_materials with the ray tree of rr_render_nested.h -- every ray carries the list of the media it is in, TraceRay sees
// both faces, an interface refracts with n_from / n_to and absorption is the crossed medium's.  mats, mat0: as above, every row of
// the scene <= NESTED_MAX_MATERIAL (the host checks)
hipError_t launch_shade_rays_nested(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, uint32_t mat0, const rr_ray_dev* rays, uint32_t n,
                                    const ShadeOut& out, FusedVariant v, hipStream_t s);
hipError_t launch_render_nested(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_surfaces.hip: opaque hit groups (rr_shade_rays_surfaces[_device], rr_render_surfaces[_device]): launch_shade_rays_nested
// and launch_render_nested with the ray tree of rr_render_surfaces.h -- an instance whose row of the surface table is opaque is lit
// by `lights` through shadow rays, emits and may continue as a mirror.  What they add to a nested launch travels in SurfaceLaunch.
// surfs: the context's table in device memory, n_surfs rows (0: every row is glass, surfs may be null); rows at or beyond n_surfs
// are glass.  lights travels by value to the kernel.  shadow_k is the cap of transparent shadows (rr_set_shadow_steps) on this
// launcher, launch_render_surfaces and launch_render_lit: 0 launches the first-hit kernel, 1 .. SHADOW_MAX_STEPS its _shadows twin,
// whose shadow rays walk through glass (rr_render_shadows.h); above that is hipErrorInvalidValue
constexpr uint32_t SHADOW_MAX_STEPS = 16;
struct SurfaceLaunch {
    const SurfDev* surfs; uint32_t n_surfs;
    const LightsDev* lights;
    uint32_t shadow_k;
    // false is hipErrorInvalidValue.  mats: the launch's material table (the band tables, for the lit frames)
    bool ok(const MatDev* mats) const { return mats && (!n_surfs || surfs) && lights->n <= MAX_LIGHTS && shadow_k <= SHADOW_MAX_STEPS; }
};
hipError_t launch_shade_rays_surfaces(const SceneDev& sc, const DispatchDev& a, const MatDev* mats, const SurfaceLaunch& su, uint32_t mat0,
                                      const rr_ray_dev* rays, uint32_t n, const ShadeOut& out, FusedVariant v, hipStream_t s);
hipError_t launch_render_surfaces(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const MatDev* mats,
                                  const SurfaceLaunch& su, uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_composed.hip: composed frames (rr_render_composed[_device]): launch_render_nested with launch_render_lens' primary
// rays (off, loff, lens; a.hx0..hy1 the lens rectangle, or the pinhole's when lens.pinhole) and launch_render_spectral's resolve.
// Sample k is shaded under the table band_mats + b_k * n_rows (the context's band set: the bands' tables one behind the other,
// every b_k below their number -- the host checks) and weighted with band_w[3 * b_k + channel]; band_mats and band_w are device
// memory.  The band indices travel as a kernel argument beside the two offset tables, a byte each: b_k is byte k & 3 of
// w[k >> 2], least significant first, so that a scalar load fetches it; 64 bytes
struct SampleBands {
    uint32_t w[SampleOffsets::MAX / 4];
    void set(uint32_t k, uint32_t band) { w[k >> 2] = (w[k >> 2] & ~(0xffu << ((k & 3u) * 8u))) | ((band & 0xffu) << ((k & 3u) * 8u)); }
};
hipError_t launch_render_composed(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, const SampleOffsets& loff,
                                  const LensDev& lens, const SampleBands& band, const MatDev* band_mats, uint32_t n_rows, const float* band_w,
                                  uint32_t mat0, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_shutter.hip: shutter frames (rr_render_shutter[_device]): launch_render_composed with the scene as one more
// per-sample table entry.  keys: the context's RR_MAX_SCENE_KEYS records in device memory, written at rr_capture_scene_key; sample k
// is traced in keys[key_k].sc with keys[key_k].mat0 -- every key_k captured and of the same kind (single_identity: all without a
// top level, else all with one), and stack, pend, stack16 valid for every key used: the host checks.  A record's env fields are
// never read: the environment map is the context's at the launch and travels as env, env_w, env_h.  The key indices travel like
// the band indices, a byte each, four to a word; 64 bytes
struct KeyDev { SceneDev sc; uint32_t mat0; uint32_t pad; };
static_assert(sizeof(KeyDev) % 16 == 0, "KeyDev: a multiple of 16 bytes");
struct SampleKeys {
    uint32_t w[SampleOffsets::MAX / 4];
    void set(uint32_t k, uint32_t key) { w[k >> 2] = (w[k >> 2] & ~(0xffu << ((k & 3u) * 8u))) | ((key & 0xffu) << ((k & 3u) * 8u)); }
};
hipError_t launch_render_shutter(const KeyDev* keys, bool single_identity, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off,
                                 const SampleOffsets& loff, const LensDev& lens, const SampleBands& band, const SampleKeys& key,
                                 const MatDev* band_mats, uint32_t n_rows, const float* band_w, const float4* env, int32_t env_w, int32_t env_h,
                                 uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_lit.hip: lit shutter frames (rr_render_lit[_device]): launch_render_shutter over the ray tree of
// launch_render_surfaces, with the lights per sample.  su: as launch_render_surfaces, the cap included.  shapes: per light the two
// edges its position (or direction) moves along, by value; lgt: per sample the light offset (lu, lv), laid out as off -- sample k is
// lit by light i at fmaf(lv_k, ey_i, fmaf(lu_k, ex_i, v_i)) per component, or at v_i where shapes.on == 0 (rr_render_lit.h).  That
// every moved v is finite and no moved direction is zero the host checks
hipError_t launch_render_lit(const KeyDev* keys, bool single_identity, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off,
                             const SampleOffsets& loff, const SampleOffsets& lgt, const LensDev& lens, const SampleBands& band, const SampleKeys& key,
                             const MatDev* band_mats, uint32_t n_rows, const float* band_w, const SurfaceLaunch& su, const LightShapesDev& shapes,
                             const float4* env, int32_t env_w, int32_t env_h, uint32_t n_samples, const ShadeOut& out, FusedVariant v, hipStream_t s);
// ---- rr_render_adaptive.hip: adaptive supersampling (rr_render_adaptive[_device]): the first n_base samples for every pixel, the
// rest up to n_max where the base samples show contrast above threshold.  Arguments as launch_render_samples; n_taken (may be null):
// n_base or n_max per pixel; refine_groups: workgroups of the refine pass, 0 = one lane per pixel of the frame (the worst case).
// The stages' state lives in a caller's workspace of AdaptiveWorkspace(nullptr, W, H).bytes bytes, 16-byte aligned, laid out as:
//   rec    W * H float4     sum of the base samples (r, g, b) and the pixel's own contrast
//   cnt    W * H uint32     TraceRay calls of the base samples
//   list   W * H uint32     the refined pixels' indices, the first base[n_blocks] entries
//   masks  n_blocks uint64  per 8x8 block (raster order): bit l = the block's pixel l in Morton order is refined
//   base   n_blocks + 1     exclusive scan of the masks' popcounts; base[n_blocks] (total) = refined pixels of the frame
struct AdaptiveWorkspace {
    float4* rec; uint32_t* cnt; uint32_t* list; unsigned long long* masks; uint32_t* base; uint32_t* total;
    uint64_t bytes;
    // p may be null (sizes only); W, H: 1..32768
    AdaptiveWorkspace(void* p, uint32_t W, uint32_t H)
    {
        const uint64_t n = (uint64_t)W * H, nb = (uint64_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
        const uint64_t o_cnt = 16u * n, o_list = o_cnt + 4u * n, o_masks = (o_list + 4u * n + 15u) & ~(uint64_t)15u, o_base = o_masks + 8u * nb;
        const uintptr_t c = reinterpret_cast<uintptr_t>(p);
        rec = static_cast<float4*>(p); cnt = reinterpret_cast<uint32_t*>(c + o_cnt); list = reinterpret_cast<uint32_t*>(c + o_list);
        masks = reinterpret_cast<unsigned long long*>(c + o_masks); base = reinterpret_cast<uint32_t*>(c + o_base); total = base + nb;
        bytes = (o_base + 4u * (nb + 1u) + 15u) & ~(uint64_t)15u;
    }
};
hipError_t launch_render_adaptive(const SceneDev& sc, const DispatchDev& a, const CamDev& cam, const SampleOffsets& off, uint32_t n_base,
                                  uint32_t n_max, float threshold, const AdaptiveWorkspace& ws, uint32_t* n_taken, uint32_t refine_groups, const ShadeOut& out,
                                  FusedVariant v, hipStream_t s);
// ---- rr_frame.hip: the screen-coordinate tables of a frame, and gathered tiles -> rasters
hipError_t launch_screen_tables(float* out, uint32_t W, uint32_t H, hipStream_t s);
hipError_t launch_assemble_tiles(const uint32_t* gathered, uint32_t* frame, uint32_t W, uint32_t H, uint32_t tiles_x,
                                 uint32_t n_tiles, uint32_t world, uint32_t max_tiles, hipStream_t s);
// batched: strides in 32-bit words
hipError_t launch_assemble_frames(const uint32_t* gathered, uint32_t* frames, uint32_t W, uint32_t H, uint32_t tiles_x,
                                  uint32_t n_tiles, uint32_t world, size_t rank_stride, size_t frame_stride,
                                  size_t out_stride, uint32_t n_frames, hipStream_t s);
hipError_t launch_assemble_frames_rgb8(const uint8_t* gathered, uint32_t* frames, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles,
                                       uint32_t world, size_t rank_stride_b, size_t frame_stride_b, size_t out_stride, uint32_t n_frames,
                                       hipStream_t s);
hipError_t launch_assemble_frames_mesh_rgb8(const uint8_t* gathered, const uint8_t* bg, uint32_t* frames, uint32_t W, uint32_t H, const MeshPartDev& mp,
                                            size_t rank_stride_b, size_t frame_stride_b, size_t bg_stride_b, size_t out_stride, uint32_t n_frames, hipStream_t s);

// ---- rr_bvh_build.hip
// Scratch + outputs of one LBVH build over n primitives (triangles of a mesh, or instances).
struct BuildBuffers {
    uint32_t n;                     // primitives
    uint32_t n_pad;                 // next power of two >= n (sort width)
    float*   prim_box;              // n * 6 (lo.xyz, hi.xyz) in primitive order
    unsigned long long* keys;       // n_pad  (morton30 << 32 | prim)
    int32_t* parent;                // (2n-1): [0,n-1) internal, [n-1, 2n-1) leaves (sorted order)
    int32_t* child;                 // (n-1)*2 child refs
    float*   node_box;              // (2n-1)*6 boxes, same indexing as parent
    uint32_t* visit;                // (n-1) arrival counters
    uint32_t* scene_box;            // 6 ordered-uint encodings of the scene bounds
    uint32_t* depth;                // 1
    uint32_t* ploc;                 // 2*n cluster arrays of the PLOC builder
    BvhNode* nodes;                 // out: max(n-1,1)
    uint32_t leaf_ref_prim;         // 0: leaf ref = ~sorted position (BLAS); 1: ~(leaf_base + primitive index) (TLAS)
    uint32_t leaf_base;
};

hipError_t launch_tri_setup(const void* verts, const uint32_t* idx, uint32_t n_tris, const BuildBuffers& b, hipStream_t s);
hipError_t launch_lbvh(const BuildBuffers& b, hipStream_t s);
// PREFER_FAST_TRACE hierarchy: Morton order + parallel locally-ordered clustering (n <= PLOC_MAX_PRIMS)
constexpr uint32_t PLOC_MAX_PRIMS = 32768;
hipError_t launch_ploc(const BuildBuffers& b, hipStream_t s);
// after launch_lbvh: keys[i] & 0xffffffff is the primitive of sorted leaf i
hipError_t launch_pack_tris(const void* verts, const uint32_t* idx, const BuildBuffers& b, TriRec* tris, NrmRec* nrms,
                            hipStream_t s);
hipError_t launch_inst_setup(const InstDev* insts, const float* blas_bounds, uint32_t n, const BuildBuffers& b, hipStream_t s);
// copy a BLAS into the scene pool: internal refs += node_off, leaf refs ~l -> ~(l + tri_off)
hipError_t launch_quantize_nodes(QNode* dst, const BvhNode* src, uint32_t n_nodes, const QGrid& g, uint32_t node_off, uint32_t tri_off,
                                 hipStream_t s);
// update builds (DXR ALLOW_UPDATE / PERFORM_UPDATE): after launch_lbvh / launch_ploc, links[2n-1] = (parent << 1 | child slot) of
// every node, -1 at the root (leaves of a TLAS, leaf_ref_prim = 1, by instance); then a refit rewrites the boxes of `nodes` in
// place over new primitives (visit: n-1 arrival counters, zero after the build, never reset)
hipError_t launch_keep_links(const BuildBuffers& b, int32_t* links, hipStream_t s);
hipError_t launch_refit_blas(const void* verts, const uint32_t* idx, uint32_t n_tris, TriRec* tris, NrmRec* nrms, BvhNode* nodes,
                             const int32_t* links, uint32_t* visit, uint32_t* scene_box, hipStream_t s);
hipError_t launch_refit_tlas(const InstDev* insts, const float* xforms_and_bounds, uint32_t n, BvhNode* nodes, const int32_t* links,
                             uint32_t* visit, hipStream_t s);
// device-side vertex update: copies n_verts 32-byte vertices d_src -> d_dst unless a position is non-finite or > 1e18, in which
// case nothing is copied and st[1] becomes 1 (st[0] is scratch)
hipError_t launch_update_verts(const void* d_src, void* d_dst, uint32_t n_verts, uint32_t* st, hipStream_t s);
hipError_t launch_env_pad(const float* rgb, float4* out, uint32_t n_texels, hipStream_t s);

} // namespace rr
