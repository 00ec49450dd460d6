/*
 * rrdxr.h -- C ABI of the MI355X-native refraction ray tracer.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (bottledspace/refraction-raytracing-dxr) has no FFI of its own: the path sits
 * behind D3D12 command-list calls issued by RefractionDemo.cpp.  Every entry
 * point below cites the reference call it replaces (file:line relative to the
 * reference tree).  Plain C types only; every function returns an rr_status
 * (never aborts, never throws); one caller thread per context, exactly like the
 * reference's single-threaded frame loop (RefractionDemo.cpp:557-612).
 *
 * The library needs a gfx950 device for every rr_* call that takes a context;
 * there is no CPU fallback.  The rr_host_* helpers (OBJ loader, camera math,
 * image decode) are pure host code.
 */
#ifndef RRDXR_H
#define RRDXR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRDXR_ABI_VERSION 3

typedef enum rr_status {
    RR_OK = 0,
    RR_ERR_INVALID_ARGUMENT = 1,
    RR_ERR_NO_DEVICE = 2,        /* no gfx950 device / HIP runtime failure at create */
    RR_ERR_DEVICE = 3,           /* a HIP call failed; rr_last_error has the text */
    RR_ERR_OUT_OF_MEMORY = 4,
    RR_ERR_STATE = 5,            /* call order violated (e.g. dispatch before build) */
    RR_ERR_IO = 6,
    RR_ERR_UNSUPPORTED = 7,      /* parameter outside what the kernels are built for */
    RR_ERR_TRAVERSAL_OVERFLOW = 8/* sticky device error flag of a dispatch (reserved: the kernels size the traversal
                                  * stack from the built tree and deeper trees are refused at build time) */
} rr_status;

/* Vertex record: Mesh.hpp:6-11 == RayTracing.hlsl:5-9.  32 bytes, stride of t2. */
typedef struct rr_vertex {
    float position[3];
    float norm[3];
    float uv[2];
} rr_vertex;

/* SceneConstants: RayTracing.hlsl:1-4, CPU twin RefractionDemo.cpp:12-15.
 * proj_inv holds the 64 bytes exactly as the CPU writes them (DirectXMath row-major);
 * the shader reads them column-major, which the kernels reproduce. */
typedef struct rr_scene_constants {
    float proj_inv[16];
    float camera_loc[4];
} rr_scene_constants;

/* Mirrors the 64-byte D3D12_RAYTRACING_INSTANCE_DESC filled at RefractionDemo.cpp:324-334. */
typedef struct rr_instance_desc {
    float    transform[12];       /* 3x4 row-major object->world */
    uint32_t instance_id_mask;    /* InstanceID:24 | InstanceMask:8  */
    uint32_t hitgroup_flags;      /* InstanceContributionToHitGroupIndex:24 | Flags:8 */
    uint64_t blas;                /* mesh id from rr_upload_mesh (stands for the BLAS GPU VA) */
} rr_instance_desc;

#define RR_INSTANCE_FLAG_TRIANGLE_CULL_DISABLE            0x1u
#define RR_INSTANCE_FLAG_TRIANGLE_FRONT_COUNTERCLOCKWISE  0x2u

/* The literals of the shader become parameters whose defaults are those literals. */
typedef struct rr_dispatch_params {
    int32_t max_refract;          /* 5      RayTracing.hlsl:82  (payload.count < 5) */
    int32_t max_reflect;          /* 2      RayTracing.hlsl:110 (payload.count < 2); <= 8 */
    float   ior;                  /* 1.3    RayTracing.hlsl:95 */
    float   tmin_primary;         /* 1e-4   RayTracing.hlsl:52 */
    float   tmax_primary;         /* 100    RayTracing.hlsl:53 */
    float   tmin_secondary;       /* 1e-3   RayTracing.hlsl:99,114 */
    float   tmax_secondary;       /* 1000   RayTracing.hlsl:100,115 */
    uint32_t flags;               /* RR_DISPATCH_* */
} rr_dispatch_params;

#define RR_DISPATCH_FLOAT_OUTPUT  0x1u  /* also keep the un-quantised float4 colour per pixel */
#define RR_DISPATCH_COLLECT_STATS 0x2u  /* instrumented kernel: node/triangle/hit/miss counters */
#define RR_DISPATCH_TIME_KERNEL   0x4u  /* bracket the render kernel with a HIP event pair (rr_kernel_time) */
#define RR_DISPATCH_KEEP_COUNTERS 0x8u  /* do not zero the rr_get_stats counters first: keep accumulating */
#define RR_DISPATCH_TILES_RGB8    0x10u /* rr_render_orbit_sharded only: tiles are written as 3 bytes per pixel (alpha is
                                         * always 255): a quarter less to gather; rr_assemble_frames_rgb8 restores RGBA8 */
#define RR_DISPATCH_TONEMAP_REINHARD 0x20u /* SURVEY 8f.2, additive: the R8G8B8A8_UNORM store takes c / (1 + c) per channel (NaN and
                                              negative -> 0, +inf -> 1) instead of the reference's saturating c; the float frame
                                              (RR_DISPATCH_FLOAT_OUTPUT) stays linear.  Off by default = RayTracing.hlsl:62 */
#define RR_DISPATCH_DEBUG_NO_CULL 0x40u /* verification switch: treat the whole frame as the scene's screen rectangle, i.e. trace the
                                           primary ray of EVERY pixel (RayTracing.hlsl:60) instead of shading the blocks the host
                                           projection of the scene bounds rules out as one Miss.  Frames are identical by
                                           contract (tests/test_gpu_parity.py::test_background_culling_...); only slower */

typedef struct rr_stats {
    uint64_t rays;                /* every TraceRay: primary + secondary */
    uint64_t primary;
    uint64_t secondary;
    uint64_t hits;
    uint64_t misses;
    uint64_t terminal_hits;       /* ClosestHit with count >= max_refract */
    uint64_t tir;                 /* RefractRay returned false */
    uint64_t node_visits;         /* internal BVH nodes fetched (32 B each)  */
    uint64_t tri_tests;           /* triangle records fetched (48 B each)    */
    uint64_t pixels;              /* pixels this context rendered (last dispatch, or all frames of rr_render_orbit) */
    uint32_t stats_valid;         /* 1 if the last dispatch ran with RR_DISPATCH_COLLECT_STATS */
    uint32_t traversal_overflow;  /* sticky device error flag of the last dispatch (0 unless a kernel raised it) */
    uint32_t bvh_depth;           /* deepest BLAS / TLAS leaf */
    uint32_t render_kernel;       /* which kernel rendered the last dispatch: 0 k_render_fused (one lane per pixel, nodes through
                                     the L1), 1 k_render_lds (the same with persistent workgroups and the nodes in LDS),
                                     2 k_render_paths (four lanes per pixel), 7 k_stream_* (two-level scenes: one kernel per ray
                                     generation, rays in HBM queues); all of them produce the same bits */
    /* wave-level loop trips of the RR_DISPATCH_COLLECT_STATS kernels: a 64-lane wave issues one internal-node step, one
     * triangle test or one shading pass per trip however many of its lanes take part, so these are what vector-issue
     * time is made of; node_visits / (64 * node_trips) is the lane utilisation of the internal-node phase, and so on */
    uint64_t node_trips;
    uint64_t leaf_trips;
    uint64_t shade_passes;
    uint64_t waves;               /* waves that rendered (one 8x8 pixel block each in the block-per-wave kernels) */
    uint64_t background_waves;    /* of those, the waves of blocks outside the scene's screen rectangle: RayGen + one Miss
                                     (counted in shade_passes too), on a branch of their own in k_render_fused */
    /* ABI 3: the clock the RR_DISPATCH_COLLECT_STATS launches ran at = clock_ticks / clock_ref_ticks * 100 MHz (sums over the
     * waves of their lifetime on the shader clock, s_memtime, and on the constant 100 MHz reference, s_memrealtime) */
    uint64_t clock_ticks;
    uint64_t clock_ref_ticks;
    char     render_kernel_name[96]; /* the instantiation that rendered the last dispatch, as rocprofv3 --kernel-trace names it
                                        (less the argument list), e.g. "k_render_fused<19, 2, false, false, false, unsigned int, 0>" */
} rr_stats;

typedef struct rr_ray {
    float origin[3]; float tmin;
    float dir[3];    float tmax;
    uint32_t flags;               /* RR_RAY_FLAG_* */
    uint32_t instance_mask;       /* DXR InstanceInclusionMask (low 8 bits): an instance is visited only if
                                     (instance_mask & InstanceMask) != 0, so 0 hits nothing.  rr_query_rays[_device] only;
                                     rr_trace_rays treats every ray as 0xff */
    uint32_t pad[2];
} rr_ray;

/* DXR RAY_FLAG values.  Every other bit is ignored.  With both cull bits set CULL_BACK wins. */
#define RR_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH 0x4u  /* rr_query_rays[_device] only: return SOME accepted intersection in
                                                             (tmin, tmax) under the ray's cull flags and stop there.  Which one is
                                                             unspecified (as in DXR) but the same for the same inputs and build;
                                                             hit is always the closest-hit query's hit, and t, u, v, prim, inst
                                                             describe the returned triangle as for a closest hit */
#define RR_RAY_FLAG_SKIP_CLOSEST_HIT_SHADER         0x8u  /* accepted, no effect: the attributes are still returned */
#define RR_RAY_FLAG_CULL_BACK_FACING_TRIANGLES  0x10u
#define RR_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES 0x20u

typedef struct rr_hit {
    float    t, u, v;             /* u weights vertex 1, v weights vertex 2 (RayTracing.hlsl:86) */
    uint32_t prim;                /* PrimitiveIndex() */
    uint32_t inst;                /* index into the rr_build_tlas array */
    uint32_t hit;                 /* 0 = miss; rr_query_rays_multi: the DXR HitKind of the triangle */
} rr_hit;

typedef struct rr_context rr_context;

/* ---- device / lifetime: createDevice, RefractionDemo.cpp:142-172 ------------------------- */
int  rr_create(int device_ordinal, rr_context** out);
int  rr_destroy(rr_context* ctx);
const char* rr_last_error(const rr_context* ctx);
/* Use a caller-owned hipStream_t (e.g. torch's current stream) instead of the context's own, so that
 * the caller's work on that stream (RCCL collectives, copies) is ordered with the render kernels.
 * NULL means HIP's default stream.  rr_reset_stream returns to the context's own stream.
 * Stands where the command queue of :161-166 stood. */
int  rr_set_stream(rr_context* ctx, void* hip_stream);
int  rr_reset_stream(rr_context* ctx);
/* wait_until_finished, RefractionDemo.cpp:65-71 */
int  rr_wait(rr_context* ctx);

/* ---- assets -> device -------------------------------------------------------------------- */
/* Mesh::upload, Mesh.cpp:55-94 (+ geometry desc Mesh.cpp:39-53): copies; caller keeps ownership.
 * Positions must be finite and no larger than 1e18 in magnitude (rr_host_validate_positions): the BLAS builder works
 * with box areas in fp32 -- a D3D12 driver is free to produce garbage for such input, this library returns
 * RR_ERR_INVALID_ARGUMENT instead.  (Mesh::load itself accepts "v 1e39 0 0": strtof turns it into +inf.) */
int  rr_upload_mesh(rr_context* ctx, const rr_vertex* verts, uint32_t n_verts,
                    const uint32_t* indices, uint32_t n_indices, uint32_t* mesh_id);
/* load_texture, RefractionDemo.cpp:108-140: tightly packed RGB32F, row pitch w*12 (:128). */
int  rr_upload_envmap(rr_context* ctx, const float* rgb, int32_t w, int32_t h);

/* ---- acceleration structures: RefractionDemo.cpp:272-361 ----------------------------------- */
/* BuildRaytracingAccelerationStructure (bottom level), :277-322 */
int  rr_build_blas(rr_context* ctx, uint32_t mesh_id);       /* = PREFER_FAST_TRACE, the flag the reference passes (:286) */
/* D3D12_RAYTRACING_ACCELERATION_STRUCTURE_BUILD_FLAG_PREFER_FAST_TRACE / _FAST_BUILD (same bit values):
 * FAST_TRACE builds a clustered (PLOC) hierarchy for meshes up to 32768 triangles, the Morton LBVH above
 * that; FAST_BUILD always builds the LBVH. */
#define RR_BUILD_PREFER_FAST_TRACE 0x4u
#define RR_BUILD_PREFER_FAST_BUILD 0x8u
int  rr_build_blas_ex(rr_context* ctx, uint32_t mesh_id, uint32_t flags);
/* BuildRaytracingAccelerationStructure (top level), :324-356.  n == 0 is invalid; the
 * reference's scene is one identity instance with mask 1 and flags 0. */
int  rr_build_tlas(rr_context* ctx, const rr_instance_desc* instances, uint32_t n);

/* ---- update builds (present from this version of the library, ABI version 3) ---------------
 * D3D12_RAYTRACING_ACCELERATION_STRUCTURE_BUILD_FLAG_ALLOW_UPDATE / _PERFORM_UPDATE (same bit values).
 * rr_build_blas_ex(ALLOW_UPDATE) builds the same nodes as without the flag and also keeps what a refit needs (a parent link
 * per node and an arrival counter per internal node, 12 bytes per triangle).  rr_build_blas_ex(PERFORM_UPDATE) refits that
 * hierarchy over the mesh's current vertices: boxes, triangle and normal records, bounds and the fp16 grid are recomputed, child
 * refs and depth stay; RR_ERR_STATE if the BLAS was not built with ALLOW_UPDATE.  Either kind of BLAS build leaves the scene
 * unbuilt: dispatches return RR_ERR_STATE until rr_build_tlas_ex builds or updates it.
 * rr_build_tlas_ex(ALLOW_UPDATE) keeps the top level refittable; rr_build_tlas_ex(PERFORM_UPDATE) takes the same n and the
 * same blas in every slot as that build (RR_ERR_INVALID_ARGUMENT otherwise; RR_ERR_STATE without an ALLOW_UPDATE build):
 * transforms, masks and flags may change.  It refits the top level over the new instance boxes and re-pools only the BLASes
 * built or updated since the scene was last built or updated.  rr_build_tlas == rr_build_tlas_ex(flags = 0). */
#define RR_BUILD_ALLOW_UPDATE   0x1u
#define RR_BUILD_PERFORM_UPDATE 0x20u
int  rr_build_tlas_ex(rr_context* ctx, const rr_instance_desc* instances, uint32_t n, uint32_t flags);
/* Overwrite a mesh's vertex buffer in place (the index buffer, the topology, never changes).  n_verts must be the uploaded
 * count; positions are validated as in rr_upload_mesh, and on failure the mesh is left untouched.  The mesh's BLAS is then out
 * of date: rr_build_tlas_ex refuses it (RR_ERR_STATE) until rr_build_blas_ex rebuilds or updates it.  The mesh id and its
 * device buffers stay the same.  The host array is copied before the call returns. */
int  rr_update_mesh_vertices(rr_context* ctx, uint32_t mesh_id, const rr_vertex* verts, uint32_t n_verts);
/* The same from device memory (n_verts 32-byte vertices at a 4-byte aligned device pointer), stream-ordered on the context's
 * stream (rr_set_stream): the copy runs after the work queued on that stream before the call, and nothing is synchronised.
 * A kernel checks the positions; if one is non-finite or huge nothing is copied, and the next rr_build_blas_ex of the mesh
 * returns RR_ERR_INVALID_ARGUMENT with the mesh and its BLAS as they were. */
int  rr_update_mesh_vertices_device(rr_context* ctx, uint32_t mesh_id, const void* d_verts, uint32_t n_verts);

/* ---- per frame ----------------------------------------------------------------------------- */
/* copy_to_buffer(cameraConstantBuffer, ...), RefractionDemo.cpp:566 */
int  rr_set_camera(rr_context* ctx, const rr_scene_constants* constants);
/* Multi-GPU sharding (new; the reference is single-adapter): this context renders only the
 * 32x32-pixel tiles t with t % world == rank.  world == 1 (default) renders the whole frame. */
int  rr_set_tile_partition(rr_context* ctx, uint32_t rank, uint32_t world);
/* DispatchRays(desc{W,H,1}), RefractionDemo.cpp:580-594.  Asynchronous on the stream. */
int  rr_dispatch_rays(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params);
/* DispatchRays(desc{W,H,Depth}): the reference always passes Depth = 1 (RefractionDemo.cpp:591); here
 * depth slice f is a whole frame rendered with constants[f] (the constant buffer becomes an array).
 * One launch renders all slices, so the long-running waves of one frame overlap the next frame's work.
 * Slice f is read back with rr_read_frame_slice(ctx, f, ...). */
int  rr_dispatch_rays_batch(rr_context* ctx, uint32_t width, uint32_t height, uint32_t depth,
                            const rr_scene_constants* constants, const rr_dispatch_params* params);
/* CopyResource(backbuffer <- rtTexture) + Present, RefractionDemo.cpp:596-609: blocks, copies the
 * R8G8B8A8_UNORM frame (and the float4 frame if RR_DISPATCH_FLOAT_OUTPUT was set) to host memory.
 * Either pointer may be NULL.  Only valid with world == 1. */
int  rr_read_frame(rr_context* ctx, uint8_t* rgba8, float* rgba32f);
int  rr_read_frame_slice(rr_context* ctx, uint32_t slice, uint8_t* rgba8, float* rgba32f);

/* Sharded output.  A context with world > 1 renders into a compact tile buffer:
 * rr_local_tile_count tiles of 32*32 RGBA8 pixels (4096 B each), tile-major. */
int  rr_local_tile_count(rr_context* ctx, uint32_t width, uint32_t height, uint32_t* n_tiles,
                         uint32_t* max_tiles_any_rank);
/* device -> device copy of this rank's tiles into caller memory (e.g. a torch tensor that RCCL
 * will gather); dst must hold max_tiles_any_rank*4096 bytes, the tail is zero-filled. */
int  rr_export_tiles(rr_context* ctx, void* d_dst);
/* rank 0: de-interleave the gathered [world][max_tiles][4096 B] buffer into a W*H RGBA8 frame.
 * d_frame may be NULL (an internal frame is used; fetch it with rr_read_frame). */
int  rr_assemble_tiles(rr_context* ctx, const void* d_gathered, uint32_t world, void* d_frame);

/* drawFrame loop in C (RefractionDemo.cpp:557-567 + WinMain.cpp:49-59): n_frames times
 * { camera constants for `angle`; rr_set_camera; rr_dispatch_rays; angle += angle_step }, issued
 * as ceil(n_frames / frames_per_dispatch) launches of frames_per_dispatch depth slices each
 * (1 = the reference's one DispatchRays per frame).  The last frames_per_dispatch frames stay
 * readable through rr_read_frame_slice.
 * Asynchronous; *angle is advanced like the reference's `static float angle`.  The counters
 * of rr_get_stats accumulate over the n_frames (they are zeroed once, before the first). */
int  rr_render_orbit(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params,
                     float* angle, float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch,
                     float fov_y, float aspect, float zn, float zf);

/* The same loop with every frame delivered to host memory: frame k lands at host_rgba8 + k*W*H*4.  Launches
 * alternate between two (or rr_set_frames_in_flight) device regions and each finished region is copied out on
 * its own stream while the next launch renders -- the CPU-GPU overlap the reference notes it lacks
 * (RefractionDemo.cpp:519-521).  Blocking: all n_frames are in host memory on return.  Page-lock the buffer
 * (rr_host_register) for full PCIe speed. */
int  rr_render_orbit_to_host(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params,
                             float* angle, float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch,
                             float fov_y, float aspect, float zn, float zf, uint8_t* host_rgba8);

/* How many launches of rr_render_orbit / rr_render_orbit_sharded may be in flight at once (1..4, default 2;
 * 1 = strictly one after the other, like the reference's fence wait per frame, RefractionDemo.cpp:611).  With 2,
 * consecutive launches go to two internal streams and write to two output regions, so the few long-running
 * waves that end one launch overlap the start of the next: monkey.obj 1080p, 137 -> 88 us per frame at
 * frames_per_dispatch = 4, 87 -> 83 at 16, nothing at 64 (ott.obj: 311 -> 172, 124 -> 107).  The call still returns
 * with everything ordered on the context's stream.  Dispatches with RR_DISPATCH_TIME_KERNEL always run one at a
 * time (their durations must be exclusive), and so do launches the persistent k_render_lds was chosen for (its
 * workgroups hold every CU until the launch ends).  rr_dispatch_rays[_batch] are not affected. */
int  rr_set_frames_in_flight(rr_context* ctx, uint32_t n);

/* The same loop for a sharded context (rr_set_tile_partition; world == 1 is allowed): frame f renders this rank's tiles straight into
 * caller device memory at d_tiles + f*frame_stride_bytes (max_tiles_any_rank*4096 B each, tail
 * zero-filled), i.e. into the send buffer of the RCCL gather, with no intermediate copy. */
int  rr_render_orbit_sharded(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params,
                             float* angle, float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch,
                             float fov_y, float aspect, float zn, float zf,
                             void* d_tiles, uint64_t frame_stride_bytes);
/* The same, submitted to internal stream `lane` (0..3) instead of the context's stream.  The lane starts
 * after everything submitted to the context's stream so far; the context's stream does NOT wait for the
 * lane until rr_lane_join (rr_wait / rr_get_stats join every lane).  Keeping two lanes in flight lets the
 * tail of one batch (a few long-running waves) overlap the head of the next, and lets the gather of batch b
 * run while batch b+1 renders.  Lanes own their constant buffers; counters are shared (atomic). */
int  rr_render_orbit_sharded_lane(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params,
                                  float* angle, float angle_step, uint32_t n_frames, uint32_t frames_per_dispatch,
                                  float fov_y, float aspect, float zn, float zf,
                                  void* d_tiles, uint64_t frame_stride_bytes, uint32_t lane);
int  rr_lane_join(rr_context* ctx, uint32_t lane);
/* Multi-GPU tile partition that only moves what has to move (see rr_host_mesh_partition below) */
typedef struct rr_mesh_partition {
    uint32_t tiles_x, n_tiles;
    uint32_t rect_x0, rect_y0, rect_w, rect_h;      /* in tiles */
    uint32_t n_mesh_tiles, n_bg_tiles, max_mesh_tiles_per_rank, world;
    uint32_t rank0_rounds;      /* how the mesh tiles are dealt: rank 0 also renders every background tile, so it takes fewer of them --
                                   ranks 1 .. world-1 take one tile each for rank0_rounds rounds, then rank 0 takes one
                                   (cycle of rank0_rounds * (world - 1) + 1 tiles); 0: plain round robin over all ranks (world == 1,
                                   or no background); 0xffffffff: rank 0 takes none (the background alone is its share) */
    uint32_t pad;
} rr_mesh_partition;
/* The mesh-tile partition for a sharded context, one DispatchRays(W, H, n_frames) per call:
 * rr_mesh_partition_for_orbit says how the n_frames frames starting at `angle` will be dealt (the rectangle is the union over
 * their cameras; the same on every rank), so that the caller can size its buffers: frame f's mesh tiles of this rank go to
 * d_mesh_tiles + f * mesh_stride_bytes (slot s at s * 3072: RGB8, max_mesh_tiles_per_rank slots, unused ones zeroed) -- the send
 * buffer of the gather --, and on rank 0 its background tiles to d_bg_tiles + f * bg_stride_bytes (n_bg_tiles slots; other
 * ranks pass NULL).  rr_assemble_frames_mesh_rgb8 puts gathered mesh tiles and rank 0's background tiles back into rasters.
 * RR_DISPATCH_DEBUG_NO_CULL is honoured here too: the launch then renders the whole-frame partition, the one
 * rr_host_mesh_partition(bounds, NULL, ...) returns (rect_w == 0, no background tiles, every tile a mesh tile), so the caller
 * sizes its buffers from that partition and passes it to rr_assemble_frames_mesh_rgb8.  The buffers are checked against the
 * partition the launch renders: ones sized from rr_mesh_partition_for_orbit are refused (RR_ERR_INVALID_ARGUMENT) wherever the
 * two differ, before anything is launched. */
int  rr_mesh_partition_for_orbit(rr_context* ctx, uint32_t width, uint32_t height, float angle, float angle_step, uint32_t n_frames,
                                 float fov_y, float aspect, float zn, float zf, rr_mesh_partition* out);
int  rr_render_orbit_mesh_sharded_lane(rr_context* ctx, uint32_t width, uint32_t height, const rr_dispatch_params* params,
                                       float* angle, float angle_step, uint32_t n_frames, float fov_y, float aspect, float zn, float zf,
                                       void* d_mesh_tiles, uint64_t mesh_stride_bytes, void* d_bg_tiles, uint64_t bg_stride_bytes,
                                       uint32_t lane);
int  rr_assemble_frames_mesh_rgb8(rr_context* ctx, const void* d_gathered, uint64_t rank_stride_bytes, uint64_t frame_stride_bytes,
                                  const void* d_bg_tiles, uint64_t bg_stride_bytes, const rr_mesh_partition* part, uint32_t n_frames,
                                  uint32_t width, uint32_t height, void* d_frames, uint64_t out_stride_bytes);
/* ---- the final image gather, natively (north star: "host stays C++ ... final RCCL gather over xGMI") --------------------
 * The reference has one adapter and no collective (RefractionDemo.cpp:163 NodeMask 0); here every rank renders its
 * tiles and ONE gather per batch of frames brings them to the root.  RCCL is looked up at run time (dlopen of
 * librccl.so; nothing links against it), one process per GPU:
 *   rr_comm_unique_id   rank 0 makes the 128-byte id and hands it to the other processes (file, pipe, MPI ...)
 *   rr_comm_init        ncclCommInitRank on the context's device; *comm is the communicator (opaque)
 *   rr_gather_frames    every rank contributes bytes_per_rank bytes at d_send; the root receives rank r's block at
 *                       d_recv + r * bytes_per_rank (d_recv may be NULL elsewhere).  Grouped ncclSend / ncclRecv, so the
 *                       root's seven incoming transfers use its seven xGMI links side by side; enqueued on the context's
 *                       stream (ordered after the renders before it, before the rr_assemble_frames after it).
 *   rr_comm_destroy
 * rr_device_alloc / rr_device_free / rr_device_read give a host without HIP headers the buffers these calls work on. */
int  rr_comm_unique_id(void* id128);
int  rr_comm_init(rr_context* ctx, const void* id128, int rank, int world, void** comm);
int  rr_comm_destroy(void* comm);
int  rr_gather_frames(rr_context* ctx, void* comm, int rank, int world, const void* d_send, void* d_recv,
                      uint64_t bytes_per_rank, int root);
int  rr_device_alloc(rr_context* ctx, uint64_t bytes, void** d_ptr);
int  rr_device_free(rr_context* ctx, void* d_ptr);
int  rr_device_read(rr_context* ctx, const void* d_src, void* host_dst, uint64_t bytes);   /* blocking */

/* rank 0, after gathering n_frames at once: frame f of rank r lies at
 * d_gathered + r*rank_stride_bytes + f*frame_stride_bytes; writes n_frames W*H RGBA8 rasters to
 * d_frames + f*out_stride_bytes.  One launch for all frames. */
int  rr_assemble_frames(rr_context* ctx, const void* d_gathered, uint32_t world, uint64_t rank_stride_bytes,
                        uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t width, uint32_t height,
                        void* d_frames, uint64_t out_stride_bytes);
/* The same for tiles rendered with RR_DISPATCH_TILES_RGB8 (max_tiles_any_rank*3072 B per frame and rank); output RGBA8. */
int  rr_assemble_frames_rgb8(rr_context* ctx, const void* d_gathered, uint32_t world, uint64_t rank_stride_bytes,
                             uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t width, uint32_t height,
                             void* d_frames, uint64_t out_stride_bytes);

/* HIP-event timing on the stream the kernels run on.  rr_timing_begin records an event,
 * rr_timing_end records another, waits for it and returns the elapsed milliseconds. */
int  rr_timing_begin(rr_context* ctx);
int  rr_timing_end(rr_context* ctx, float* elapsed_ms);
/* sum and count of the render-kernel durations of all dispatches issued with
 * RR_DISPATCH_TIME_KERNEL since the last call (blocks until they finished; at most 4096). */
int  rr_kernel_time(rr_context* ctx, float* sum_ms, uint32_t* n_launches);

/* exact counters of the last dispatch (blocks until it finished) */
int  rr_get_stats(rr_context* ctx, rr_stats* out);

/* Page-lock a caller-owned host buffer (e.g. the back buffer rr_read_frame copies into) so that read-backs run at
 * PCIe speed instead of through the runtime's staging copies; unregister before freeing it.  The reference's
 * readback heap plays this role (a CPU-visible committed resource, RefractionDemo.cpp:596-609 present path). */
int  rr_host_register(rr_context* ctx, void* p, size_t bytes);
int  rr_host_unregister(rr_context* ctx, void* p);

/* TraceRay on caller-supplied rays (host arrays), same traversal code as the render path.
 * Stands for RayTracing.hlsl:60,106,121 in isolation; used by the parity tests. */
int  rr_trace_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, rr_hit* hits);

/* ---- ray queries (present from this version of the library, ABI version 3) -------------------
 * TraceRay(Scene, flags, instance_mask, 0, 0, 0, ray, payload) on caller rays: the traversal of the render path with the ray's
 * InstanceInclusionMask (rr_ray.instance_mask) and RR_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH; rays of one batch may mix
 * first-hit and closest-hit.  A closest-hit query with instance_mask 0xff gives what rr_trace_rays gives.  Both return
 * RR_ERR_STATE until the scene is built, and after a BLAS build or update until rr_build_tlas_ex follows it.
 * rr_query_rays: host arrays, blocking (like rr_trace_rays). */
int  rr_query_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, rr_hit* hits);
/* The same from device memory: n rays at a 16-byte aligned device pointer, n hits to a 4-byte aligned one
 * (RR_ERR_INVALID_ARGUMENT otherwise; n == 0 is RR_OK).  Stream-ordered on the context's stream (rr_set_stream): the kernel
 * reads the rays after the work queued on that stream before the call, nothing is synchronised and nothing allocated.  The
 * rays must stay valid, and the hits must not be read, until that stream has run the query. */
int  rr_query_rays_device(rr_context* ctx, const void* d_rays, uint32_t n, void* d_hits);
/* Multi-hit queries (DXR's any-hit idiom that records each candidate and calls IgnoreHit), in one walk per ray.  For ray i the
 * hits are every triangle the closest-hit query's test accepts with t in (tmin, tmax), under the ray's cull flags and instance
 * mask (instance flags applied as for a closest hit), sorted ascending by (t, inst, prim); each (inst, prim) appears at most
 * once.  The first min(k, total) of them go to hits[i*k + j]: t, u, v, prim and inst have the bits a closest-hit query reports
 * for that triangle, and `hit` holds the DXR HitKind -- RR_HIT_KIND_TRIANGLE_FRONT_FACE if det > 0 in object space (swapped by
 * RR_INSTANCE_FLAG_TRIANGLE_FRONT_COUNTERCLOCKWISE, the rule the cull flags follow), else _BACK_FACE.  The remaining slots are
 * miss records (hit 0, t = the ray's tmax, u = v = prim = inst = 0).  counts may be NULL; if given, counts[i] is the total
 * number of accepted triangles (the walk is then not pruned by the k-th hit; the slots are the same either way).
 * 0 <= k <= RR_QUERY_MAX_HITS, and k == 0 only with counts (an occupancy query); anything else is RR_ERR_INVALID_ARGUMENT.
 * RR_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH and _SKIP_CLOSEST_HIT_SHADER are ignored (an any-hit shader that ignores every
 * hit commits none, so there is nothing to end the search on).  Errors, state and stream order as rr_query_rays[_device]; the
 * device variant takes 16-byte aligned rays and 4-byte aligned hits (n*k records) and counts (n words), allocates nothing.
 * NOT a crossing count: the triangle test is Moller-Trumbore, not watertight, so a ray through an edge shared by two
 * triangles may report both of them or neither. */
#define RR_QUERY_MAX_HITS 16
#define RR_HIT_KIND_TRIANGLE_FRONT_FACE 0xFEu   /* DXR HIT_KIND_* values */
#define RR_HIT_KIND_TRIANGLE_BACK_FACE  0xFFu
int  rr_query_rays_multi(rr_context* ctx, const rr_ray* rays, uint32_t n, uint32_t k, rr_hit* hits, uint32_t* counts);
int  rr_query_rays_multi_device(rr_context* ctx, const void* d_rays, uint32_t n, uint32_t k, void* d_hits, void* d_counts);

/* ---- radiance queries: a RayGen shader of the caller's own --------------------------------------
 * The shader's whole ray tree (RayTracing.hlsl:42-137) on caller rays instead of GenerateCameraRay's: ray i starts as RayGen's
 * payload {colour 0, weight 1, outside = true, count 0} with origin, dir, tmin, tmax taken from rays[i] as they are (dir is
 * NOT normalised, exactly as TraceRay takes it), CULL_BACK; every secondary ray is the shader's (tmin/tmax_secondary,
 * max_refract, max_reflect, ior of *params; NULL = defaults).  rr_ray.flags, instance_mask and pad are ignored: the shader's
 * TraceRay calls fix them.  Outputs, each optional, but at least one of rgba32f / rgba8 must be given:
 *   rgba32f[i]   float4 (r, g, b, 1): the un-quantised colour, the bits RR_DISPATCH_FLOAT_OUTPUT gives for that ray
 *   rgba8[i]     the R8G8B8A8_UNORM store of it (honours RR_DISPATCH_TONEMAP_REINHARD in params->flags)
 *   n_rays[i]    uint32: TraceRay calls of ray i's tree, the primary included
 * Of params->flags only RR_DISPATCH_TONEMAP_REINHARD is honoured, the others are ignored.  max_reflect > 8 is
 * RR_ERR_UNSUPPORTED and bad bounce limits RR_ERR_INVALID_ARGUMENT, as for rr_dispatch_rays.  Errors and state as the ray
 * queries: RR_ERR_STATE until the scene is built and after a BLAS build or update until rr_build_tlas_ex follows it; n == 0
 * is RR_OK.  A radiance query is not a dispatch: the context's frame (rr_read_frame), the rr_get_stats counters and
 * render_kernel[_name] and the measured kernel choices stay as the last dispatch left them.  Rays with non-finite or zero
 * directions give an unspecified colour; the tree of every ray is bounded by max_refract and max_reflect whatever its
 * arithmetic yields.
 * rr_shade_rays: host arrays, blocking.  rr_shade_rays_device: rays and d_rgba32f 16-byte aligned, d_rgba8 and d_n_rays 4-byte
 * aligned device pointers (RR_ERR_INVALID_ARGUMENT otherwise); stream-ordered on the context's stream (rr_set_stream) like
 * rr_query_rays_device: nothing is synchronised and nothing allocated. */
int  rr_shade_rays(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params,
                   float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_shade_rays_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params,
                          void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- supersampled frames: n_samples primary rays per pixel, resolved in the kernel --------------
 * Each pixel of a width x height frame takes n_samples primary rays through n_samples sub-pixel positions, every one with the
 * shader's whole ray tree, and their colours are averaged into one per pixel.  offsets: host array of 2 * n_samples floats
 * (x0, y0, x1, y1, ...) in pixel units inside the pixel -- (0.5, 0.5) is the centre -- every value finite and in [0, 1], with
 * 1 <= n_samples <= RR_MAX_SAMPLES; NULL: the built-in pattern of rr_host_sample_pattern(n_samples).  Sample (ox, oy) of
 * pixel (x, y) is GenerateCameraRay (RayTracing.hlsl:27-40) with its literal 0.5 replaced:
 *   sx = ((float)x + ox) / (float)width * 2 - 1,  sy = -(((float)y + oy) / (float)height * 2 - 1)
 * from camera_loc over params' primary interval with RayGen's payload: the rays of rr_host_camera_rays.  With c_s the
 * colour rr_shade_rays gives sample s's ray, a channel resolves in fp32 as ((c_0 + c_1) + ... + c_(S-1)) / (float)S.
 * Outputs, row-major width * height, each optional, but at least one of rgba32f / rgba8 must be given:
 *   rgba32f[i]   float4 (resolved r, g, b, 1)
 *   rgba8[i]     the R8G8B8A8_UNORM store of it (honours RR_DISPATCH_TONEMAP_REINHARD)
 *   n_rays[i]    uint32: TraceRay calls of all the trees of pixel i
 * Of params->flags only RR_DISPATCH_TONEMAP_REINHARD and RR_DISPATCH_DEBUG_NO_CULL are read (blocks of 8 x 8 pixels outside
 * rr_host_screen_rect of the scene are shaded as one Miss per sample without TraceRay; the flag traces them, with the same
 * output).  constants, params and offsets are host pointers in both variants; width and height are 1..32768.  Like a radiance
 * query this is not a dispatch: the context's frame, the rr_get_stats counters, render_kernel[_name] and the measured kernel
 * choices stay as the last dispatch left them, and rr_set_tile_partition is ignored (the whole frame is rendered).  Errors and
 * state as rr_shade_rays[_device].
 * rr_render_samples: host arrays, blocking.  rr_render_samples_device: d_rgba32f 16-byte, d_rgba8 and d_n_rays 4-byte aligned
 * device pointers (RR_ERR_INVALID_ARGUMENT otherwise); stream-ordered on the context's stream, nothing is synchronised and
 * nothing allocated. */
#define RR_MAX_SAMPLES 64
int  rr_render_samples(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                       const rr_dispatch_params* params, const float* offsets, uint32_t n_samples,
                       float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_render_samples_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                              const rr_dispatch_params* params, const float* offsets, uint32_t n_samples,
                              void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- adaptive supersampling: n_base samples everywhere, n_max where the frame has contrast (present from ABI version 3) ------
 * A supersampled frame whose pixels take the first n_base samples of the pattern, and the remaining ones up to n_max only where
 * the base samples show contrast.  width, height, constants, params and offsets[n_max][2] as for rr_render_samples (offsets ==
 * NULL: rr_host_sample_pattern(n_max), so n_max is 1, 2, 4, 8 or 16); 1 <= n_base <= n_max <= RR_MAX_SAMPLES; threshold finite and
 * >= 0 (RR_ERR_INVALID_ARGUMENT otherwise).  The base samples are samples 0 .. n_base-1 of the one pattern.  With c_s(p) the
 * colour rr_shade_rays gives sample s of pixel p (the rays of rr_host_camera_rays with offset s), all in fp32 and per channel:
 *   1. sum_b(p) = ((c_0 + c_1) + ...) + c_(n_base-1), starting at c_0: the resolve rule of rr_render_samples.
 *   2. the display value of a channel value c: v(c) = fminf(fmaxf(c, 0), 1); with RR_DISPATCH_TONEMAP_REINHARD m = fmaxf(c, 0),
 *      v = fminf(m / (1 + m), 1).  fmaxf / fminf return the operand that is a number: NaN shows as 0, +inf as 1.
 *   3. own contrast: r_own(p) = max over channels of (max_s v(c_s) - min_s v(c_s)) over the base samples.
 *   4. neighbour contrast: b(p) = v(sum_b(p) / (float)n_base); r_nb(p) = max over the 4-neighbours q of p inside the frame and
 *      over channels of fabsf(b(p) - b(q)).
 *   5. p is refined iff r_own(p) > threshold || r_nb(p) > threshold.
 *   6. an unrefined pixel resolves to sum_b / (float)n_base; a refined one continues the fold, sum_b + c_(n_base) + ... +
 *      c_(n_max-1), and divides by (float)n_max.
 * No operation of 2 to 5 is fused with another.  So every pixel is, bit for bit, that pixel of rr_render_samples(offsets, n_base)
 * or of rr_render_samples(offsets, n_max); n_base == n_max is rr_render_samples(n_max), and a threshold >= 1 refines nothing.
 * Outputs, row-major width * height, each optional, but at least one of rgba32f / rgba8 must be given:
 *   rgba32f[i]   float4 (resolved r, g, b, 1)
 *   rgba8[i]     the R8G8B8A8_UNORM store of it (honours RR_DISPATCH_TONEMAP_REINHARD)
 *   n_rays[i]    uint32: TraceRay calls of all the trees pixel i ran
 *   n_taken[i]   uint32: n_base or n_max
 * Of params->flags only RR_DISPATCH_TONEMAP_REINHARD and RR_DISPATCH_DEBUG_NO_CULL are read; background blocks take part in
 * the rule like any other, and the flag changes no byte of any output.  Not a dispatch, exactly as rr_render_samples: frame,
 * rr_get_stats, render_kernel[_name] and the kernel choices stay, rr_set_tile_partition is ignored.  Errors and state as
 * rr_render_samples[_device].
 * rr_render_adaptive: host arrays, blocking; n_refined (may be NULL) receives the number of refined pixels.
 * rr_render_adaptive_device: device pointers aligned as for rr_render_samples_device, d_n_taken 4-byte aligned; stream-ordered
 * on the context's stream: nothing is synchronised, allocated or read back.  The intermediate state lives in d_workspace, 16-byte
 * aligned device memory of workspace_bytes >= rr_host_adaptive_workspace_bytes(width, height) (RR_ERR_INVALID_ARGUMENT
 * otherwise), which needs no clearing and may be reused by the next call on the same stream. */
int  rr_render_adaptive(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                        const rr_dispatch_params* params, const float* offsets, uint32_t n_base, uint32_t n_max, float threshold,
                        float* rgba32f, uint8_t* rgba8, uint32_t* n_rays, uint32_t* n_taken, uint64_t* n_refined);
int  rr_render_adaptive_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                               const rr_dispatch_params* params, const float* offsets, uint32_t n_base, uint32_t n_max,
                               float threshold, void* d_rgba32f, void* d_rgba8, void* d_n_rays, void* d_n_taken,
                               void* d_workspace, uint64_t workspace_bytes);

/* ---- thin-lens frames: depth of field in the supersampling kernel (present from ABI version 3) ---------------------------------
 * A supersampled frame whose primary rays start on a lens of finite aperture instead of at camera_loc: what lies at
 * focus_distance along the centre ray is sharp, everything else goes soft.  With M = constants->proj_inv, O = camera_loc and
 * R(sx, sy) the un-normalised vector GenerateCameraRay forms, ((sx*M[0] + sy*M[1]) + M[3], (sx*M[4] + sy*M[5]) + M[7],
 * (sx*M[8] + sy*M[9]) + M[11]), once per frame on the host in fp32 (normalize: v * (1 / sqrt(dot(v, v))), the ray generators'):
 *   A = radius * normalize(M[0], M[4], M[8]),  B = radius * normalize(M[1], M[5], M[9]),  s = focus_distance / |(M[3], M[7], M[11])|
 * so s * R spans the focal plane.  Sample k of pixel (x, y) has the pixel offset (ox, oy) of offsets and the lens offset (lx, ly)
 * of lens_offsets, in units of the radius; in fp32, one rounding per operation and nothing fused:
 *   sx, sy, R   as for rr_render_samples
 *   off    = (lx*A.x + ly*B.x, lx*A.y + ly*B.y, lx*A.z + ly*B.z)
 *   origin = O + off
 *   dir    = normalize(s*R.x - off.x, s*R.y - off.y, s*R.z - off.z)
 * over params' primary interval with RayGen's payload: the rays of rr_host_lens_rays.  The frame is the fold of rr_shade_rays on
 * those rays by the resolve rule of rr_render_samples.  radius == 0 takes the pinhole's rays as they are, origin O and dir
 * normalize(R): the frame is rr_render_samples byte for byte.
 * offsets as for rr_render_samples (NULL: the built-in pattern, n_samples 1, 2, 4, 8 or 16).  lens_offsets: host array of
 * 2 * n_samples floats, each finite and in [-1, 1]; NULL: rr_host_lens_pattern(n_samples).  lens: not NULL, radius finite and
 * >= 0, focus_distance finite and > 0; the centre column (M[3], M[7], M[11]) and, with radius > 0, both axis columns must have a
 * finite non-zero length (RR_ERR_INVALID_ARGUMENT otherwise, before any output memory is looked at).
 * Blocks of 8 x 8 pixels outside rr_host_lens_screen_rect of the scene are shaded as one Miss per sample on that sample's lens
 * direction; RR_DISPATCH_DEBUG_NO_CULL traces them, with the same output.  Outputs, resolve, tone mapping, errors and state
 * exactly as rr_render_samples[_device]: not a dispatch, rr_set_tile_partition is ignored, the _device variant is stream-ordered
 * and neither synchronises nor allocates. */
typedef struct rr_lens { float radius; float focus_distance; } rr_lens;
int  rr_render_lens(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                    const rr_dispatch_params* params, const float* offsets, const float* lens_offsets, uint32_t n_samples,
                    const rr_lens* lens, float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_render_lens_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                           const rr_dispatch_params* params, const float* offsets, const float* lens_offsets, uint32_t n_samples,
                           const rr_lens* lens, void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- spectral frames: dispersion with an index of refraction per sample (present from ABI version 3) -----------------------------
 * A supersampled frame in which every sample has its own index of refraction and its own weight per colour channel: distribution
 * ray tracing over the wavelength, which puts colour fringes on refracting glass.  Sample k of pixel (x, y) is sample k of
 * rr_render_samples, the ray of rr_host_camera_rays with offset k, shaded by the ray tree of rr_shade_rays with params->ior
 * replaced by bands[k].ior; the reciprocal the shader refracts with on the way in is 1.0f / ior in fp32, the expression every
 * launcher forms it with.  With c_k that colour, channel ch of the pixel resolves in fp32, one rounding per operation and nothing
 * fused:
 *   p_k = bands[k].weight[ch] * c_k[ch]
 *   sum = p_0, then sum = sum + p_k in sample order
 *   out = sum / (float)n_samples
 * n_rays[i] is the number of TraceRay calls of all the trees of pixel i.  bands == NULL: every band is { params->ior, 1, 1, 1 };
 * such a frame, and any table with those values, is rr_render_samples byte for byte.  params->ior is validated as usual even when
 * bands replaces it.
 * offsets as for rr_render_samples (NULL: the built-in pattern, n_samples 1, 2, 4, 8 or 16).  bands: host array of n_samples
 * records or NULL.  1 <= n_samples <= RR_MAX_SAMPLES; every band's ior finite and > 0; every weight finite -- negative weights
 * are allowed (tables derived from XYZ matching functions have them) (RR_ERR_INVALID_ARGUMENT otherwise, before any output memory
 * is looked at).
 * Blocks of 8 x 8 pixels outside rr_host_screen_rect of the scene are shaded as one Miss per sample, which does not depend on the
 * index of refraction, and weighted and resolved by the same rule; RR_DISPATCH_DEBUG_NO_CULL traces them, with the same output.
 * The pinhole's rectangle holds because the primary rays are rr_render_samples'.  Outputs, tone mapping, alignment rules, errors and
 * state exactly as rr_render_samples[_device]: not a dispatch, rr_set_tile_partition is ignored, the _device variant is
 * stream-ordered and neither synchronises nor allocates (the tables travel as kernel arguments). */
typedef struct rr_band { float ior; float weight[3]; } rr_band;      /* 16 bytes */
int  rr_render_spectral(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                        const rr_dispatch_params* params, const float* offsets, const rr_band* bands, uint32_t n_samples,
                        float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_render_spectral_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                               const rr_dispatch_params* params, const float* offsets, const rr_band* bands, uint32_t n_samples,
                               void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- hit groups: per-instance glass with its own index of refraction and tint (present from ABI version 3) ------------------------
 * The context holds a material table.  An instance selects a row with the low 24 bits of rr_instance_desc::hitgroup_flags (DXR's
 * InstanceContributionToHitGroupIndex), in rr_build_tlas and in its RR_BUILD_PERFORM_UPDATE alike.  A material is an index of
 * refraction and an absorption coefficient per unit length and colour channel (R, G, B).  Only the two calls below read the table:
 * the dispatches, rr_shade_rays and the other frames shade every instance with params->ior and absorb nothing.
 *
 * rr_set_materials copies n rows into a device buffer the context owns; n == 0 clears the table.  It may come before or after
 * rr_build_tlas and may be repeated: the new table takes effect on the next call, without a rebuild.  Every ior finite and > 0,
 * every sigma_a finite and >= 0, n <= 2^24 (RR_ERR_INVALID_ARGUMENT otherwise; the table in force stays).  Waits for the
 * context's stream.
 *
 * rr_shade_rays_materials[_device] is rr_shade_rays[_device] and rr_render_materials[_device] is rr_render_samples[_device] -- the
 * same arguments, rays, outputs, resolve, culling, alignment rules and state: not dispatches -- with this ray tree instead:
 *   1. the path weight is one float per channel.  RayGen sets (1, 1, 1); every w * (1 - R) and w * R is taken per channel; a Miss
 *      adds acc.c = fmaf(w.c, e.c, acc.c);
 *   2. ClosestHit on instance i refracts with material m = hitgroup_flags_i & 0xffffff: eta = outside ? 1.0f / ior_m : ior_m;
 *   3. a ray that reaches ClosestHit from inside the glass (it was refracted into instance i and now hits its inner side) is
 *      absorbed over the distance t it travelled, before anything else: w.c = w.c * E(-(sigma_a_m[c] * t)), each operation rounded
 *      once.  Secondary directions have unit length, so t is a length; a caller's primary ray always starts outside.  The medium
 *      is that of the surface being left, which for overlapping or nested instances is an approximation.  A Miss from inside (an
 *      open mesh) absorbs nothing.
 * E is rr_host_expf_neg, fp32 with explicit fused operations, the same on host and device: exactly 1 at +0 and -0, 0 from -87 down.
 * So a table whose rows are all { ior, 0, 0, 0 } makes both calls equal rr_shade_rays / rr_render_samples under params->ior = ior,
 * byte for byte.  params->ior is ignored (not even validated); the rest of params is used and checked as by the scalar calls.
 * RR_ERR_STATE without a built TLAS or without a table; RR_ERR_INVALID_ARGUMENT when an instance's index is >= the table's
 * length. */
typedef struct rr_material { float ior; float sigma_a[3]; } rr_material;      /* 16 bytes */
int  rr_set_materials(rr_context* ctx, const rr_material* mats, uint32_t n);
int  rr_shade_rays_materials(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f,
                             uint8_t* rgba8, uint32_t* n_rays);
int  rr_shade_rays_materials_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f,
                                    void* d_rgba8, void* d_n_rays);
int  rr_render_materials(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                         const rr_dispatch_params* params, const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8,
                         uint32_t* n_rays);
int  rr_render_materials_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                                const rr_dispatch_params* params, const float* offsets, uint32_t n_samples, void* d_rgba32f,
                                void* d_rgba8, void* d_n_rays);

/* ---- nested media: instances inside, or overlapping, other instances (present from ABI version 3) ---------------------------------
 * The material tree above traces with CULL_BACK outside and CULL_FRONT inside, so a ray inside one glass instance cannot see the
 * front faces of anything placed in it: an ice cube in water is invisible from inside the water, eta at the outer surface is always
 * taken against air and the outer glass absorbs over the whole chord.  The four calls below are their _materials twins -- the same
 * arguments, table (rr_set_materials, rr_material), rays, sample offsets, resolve, tone mapping, RGBA8, culling of background blocks,
 * alignment rules and state: not dispatches, on the context's stream, params->ior ignored -- with a ray tree in which every ray knows
 * the media it is in.  One rounding per written operation, fmaf only where written:
 *
 * A ray carries (O, D, w[3], count, L).  L is the list of the material rows of the media it is in, in the order it entered them,
 * RR_NESTED_MAX_MEDIA (4) at most; empty means air (ior 1, no absorption).  A caller's primary ray starts with L empty.
 * TraceRay is called with cull flags 0 (both faces), mask 0xff and [tmin, tmax] as before.  The face of the hit is the HitKind of
 * rr_query_rays_multi: front = (det > 0) != the instance's RR_INSTANCE_FLAG_TRIANGLE_FRONT_COUNTERCLOCKWISE, det in object space.
 *   Miss: acc.c = fmaf(w.c, e.c, acc.c).  Nothing is absorbed, whatever L holds (an open mesh).
 *   ClosestHit on an instance of row m at distance t with count < max_refract (a hit at the limit adds nothing):
 *     1. c = top(L), the medium entered last.  If c is not air: w.ch = w.ch * E(-(sigma_a[c].ch * t)), E = rr_host_expf_neg: the
 *        medium crossed, not the one hit.
 *     2. Front face: L' = push(L, m); a push onto a full list is dropped.  Back face: L' = L without its last occurrence of m;
 *        removing an absent row changes nothing.  c' = top(L').
 *     3. X = fmaf(t, D, O).  Children have count + 1 and [tmin_secondary, tmax_secondary].
 *     4. c' and c the same row: NOT AN INTERFACE.  (The ray leaves something whose surface lies inside a medium entered later, or
 *        enters a second body of the same row, or its push was dropped, or it meets a back face from outside.)  One child
 *        (X, D, w, L'): D and w keep their bits, no reflection, no Fresnel factor.  The pass still costs one count, which keeps the
 *        tree bounded as before: a branch ends at max_refract whatever it meets.
 *     5. Otherwise AN INTERFACE.  N is the shading normal, Nf = front ? N : -N, R the shader's expression (hlsl:92-93),
 *        eta = ior[c] * (1.0f / ior[c']) with air as 1.0f on either side (1.0f / ior is the value rr_set_materials stores), and
 *        RefractRay(D, Nf, eta).  The refracted child carries L' and w * (1 - R) per channel; the reflected child exists if
 *        count < max_reflect, stays where it was (L) and carries w * R; on total internal reflection only the reflected child
 *        exists (hlsl:118-122).  Depth-first, refracted child first, as before.
 *
 * Reduction: on a scene in which culled and unculled TraceRay find the same hit for every ray of every tree -- closed, consistently
 * wound, pairwise disjoint instances -- these calls equal rr_shade_rays_materials / rr_render_materials byte for byte, colours, RGBA8
 * and ray counts: 1.0f * inv_ior and ior * 1.0f are exact, top(L) is the instance being left, front is outside.  (An open mesh such
 * as the shipped monkey.obj does not qualify.)
 * Overlap is handled without priorities: where a liquid's mesh reaches slightly into its container's wall, the interface is taken at
 * the first of the two surfaces met and the second is "not an interface".
 * Not covered: more than RR_NESTED_MAX_MEDIA simultaneous media (the dropped push); rays that start inside a medium; R0 recomputed
 * from the two indices (it stays the shader's constant); lens, spectral and adaptive frames; the dispatch kernels.
 *
 * RR_ERR_STATE without a built TLAS or without a table; RR_ERR_INVALID_ARGUMENT when an instance's row is >= the table's length
 * or > RR_NESTED_MAX_MATERIAL (a list entry is one byte); the table itself may be longer. */
#define RR_NESTED_MAX_MEDIA 4
#define RR_NESTED_MAX_MATERIAL 254
int  rr_shade_rays_nested(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f,
                          uint8_t* rgba8, uint32_t* n_rays);
int  rr_shade_rays_nested_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f,
                                 void* d_rgba8, void* d_n_rays);
int  rr_render_nested(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                      const rr_dispatch_params* params, const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8,
                      uint32_t* n_rays);
int  rr_render_nested_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                             const rr_dispatch_params* params, const float* offsets, uint32_t n_samples, void* d_rgba32f,
                             void* d_rgba8, void* d_n_rays);

/* ---- opaque hit groups: lit, mirror and emissive instances with shadow rays (additive; the ABI version stays 3) -------------------
 * hitgroup_flags & 0xffffff selects a row per instance, as DXR's InstanceContributionToHitGroupIndex selects a ClosestHit shader.
 * The four calls below are their _nested twins -- the same arguments, rays, sample offsets, resolve, tone mapping, RGBA8, culling of
 * background blocks, alignment rules and state: not dispatches, on the context's stream, params->ior ignored -- with a second hit
 * group: an instance whose row of the SURFACE table is RR_SURFACE_OPAQUE is a surface lit by a small set of directional and point
 * lights through shadow rays, with an emission term and an optional mirror child.
 *
 * Tables.  Surface row r belongs with material row r.  Instance rows at or beyond the surface table's length are glass, and so are
 * all rows while no surface table is set.  rr_set_materials neither reads nor clears the surface table.  An opaque row still needs
 * a material row; its ior and sigma_a are never read.  The context owns a device copy of the surface table, next to the material
 * table, and a host copy of the lights, which travel by value with every launch (one in flight keeps the set it was launched with).
 * Both setters wait for the context's stream, as rr_set_materials does, and only the four calls below read what they set.
 *   rr_set_surfaces: n == 0 clears.  kind a known value; every float finite; albedo and specular >= 0 (emission may be negative).
 *   rr_set_lights:   n <= RR_MAX_LIGHTS; ambient NULL = (0, 0, 0), else three finite floats.  kind a known value; v and radiance
 *                    finite (a negative radiance is allowed); a directional v is not (0, 0, 0) and is used AS GIVEN -- normalise it;
 *                    shadow_mask <= 0xff.  It also clears the shape table of rr_set_light_shapes (below), whose rows belong with
 *                    the lights they were set for; none of the four calls here reads that table.
 * A refused table (RR_ERR_INVALID_ARGUMENT) leaves the one in force.
 *
 * The contract.  One rounding per written operation, fmaf only where written, dot is the shader's dot3.  Everything in the nested
 * calls' contract stands, step 1 included: absorption over t in the medium CROSSED happens before anything else, so an opaque olive
 * inside a tinted liquid is dimmed correctly.  After step 1, a hit with count < max_refract on row m whose surface kind is
 * RR_SURFACE_OPAQUE does this instead of steps 2-5:
 *   a. L is unchanged.  X = fmaf(t, D, O).  N is the shading normal, Nf = front ? N : -N, front the HitKind as before.
 *   b. E = ambient.  Then for each light in table order:
 *        directional: Ld = v, far = tmax_secondary, g = 1.
 *        point:       d = v - X per component, d2 = dot(d, d), far = sqrtf(d2), Ld = d / far per component, g = 1.0f / d2.
 *        cs = dot(Nf, Ld).  If !(cs > 0) the light adds nothing AND NO RAY IS TRACED.  Otherwise one shadow ray:
 *        TraceRay(X, Ld, [tmin_secondary, far], cull flags 0, ACCEPT_FIRST_HIT_AND_END_SEARCH, InstanceInclusionMask = shadow_mask).
 *        It counts as one ray in n_rays, whether or not any instance passes the mask.  Any accepted hit occludes, glass instances
 *        included; to let glass cast no shadow, give it an InstanceMask bit that the light's shadow_mask lacks.  If unoccluded:
 *        f = cs * g and E.ch = fmaf(radiance.ch, f, E.ch).
 *   c. col.ch = fmaf(albedo.ch, E.ch, emission.ch).  Then acc.ch = fmaf(w.ch, col.ch, acc.ch).
 *   d. If any specular.ch != 0: one child (X, normalize(ReflectRay(D, Nf)), w.ch * specular.ch, L, count + 1) on the secondary
 *      interval.  It is the continuing ray; nothing is parked.  It is NOT gated by max_reflect -- a mirror is the main path -- count
 *      alone bounds it, so the tree stays bounded as before.  Otherwise the branch ends and a parked ray is taken up, as after a Miss.
 * A scene without a top level shades its one instance (mask 1, row of instance 0) the same way; its shadow ray passes if
 * shadow_mask & 1.
 *
 * Reduction: with no surface table, or with every row glass, the four calls equal the _nested calls byte for byte in colours, RGBA8
 * and counts.  The lights are then never read.
 * Not covered: area lights or environment lighting of opaque surfaces in these four calls; textures; opaque rows in
 * rr_render_composed / rr_render_shutter, the dispatch kernels and the _materials calls (all of which ignore the surface table).
 * Opaque rows through a lens, over scene keys and under lights with an area are rr_render_lit's, below.  Shadow rays that pass
 * glass and take its tint are opt-in (rr_set_shadow_steps, further below); what they leave out: Fresnel loss and bending at the
 * interfaces a shadow ray crosses, absorption beyond its last hit, caustics.
 *
 * State and rows as the nested calls: RR_ERR_STATE without a built TLAS or without a material table; RR_ERR_INVALID_ARGUMENT when an
 * instance's row is >= the material table's length or > RR_NESTED_MAX_MATERIAL. */
#define RR_SURFACE_GLASS  0u      /* the row of rr_set_materials decides everything: rr_shade_rays_nested's ClosestHit */
#define RR_SURFACE_OPAQUE 1u
typedef struct rr_surface { uint32_t kind; float albedo[3]; float emission[3]; float specular[3]; uint32_t pad[2]; } rr_surface;  /* 48 bytes */
#define RR_LIGHT_DIRECTIONAL 0u   /* v: unit direction TOWARDS the light */
#define RR_LIGHT_POINT       1u   /* v: position */
#define RR_MAX_LIGHTS 8
typedef struct rr_light { float v[3]; uint32_t kind; float radiance[3]; uint32_t shadow_mask; } rr_light;                          /* 32 bytes */
int  rr_set_surfaces(rr_context* ctx, const rr_surface* rows, uint32_t n);
int  rr_set_lights(rr_context* ctx, const rr_light* lights, uint32_t n, const float ambient[3]);
int  rr_shade_rays_surfaces(rr_context* ctx, const rr_ray* rays, uint32_t n, const rr_dispatch_params* params, float* rgba32f,
                            uint8_t* rgba8, uint32_t* n_rays);
int  rr_shade_rays_surfaces_device(rr_context* ctx, const void* d_rays, uint32_t n, const rr_dispatch_params* params, void* d_rgba32f,
                                   void* d_rgba8, void* d_n_rays);
int  rr_render_surfaces(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                        const rr_dispatch_params* params, const float* offsets, uint32_t n_samples, float* rgba32f, uint8_t* rgba8,
                        uint32_t* n_rays);
int  rr_render_surfaces_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                               const rr_dispatch_params* params, const float* offsets, uint32_t n_samples, void* d_rgba32f,
                               void* d_rgba8, void* d_n_rays);

/* ---- composed frames: a lens and dispersion on the nested-media tree (present from ABI version 3) ---------------------------------
 * One frame call that takes the primary rays of rr_render_lens, the ray tree of rr_render_nested and the weighted resolve of
 * rr_render_spectral, with dispersion per material instead of per frame: the glass of water with an ice cube, photographed with
 * depth of field and colour fringes.
 *
 * The band set.  rr_set_material_bands gives the context n_bands variants T_0 .. T_(n_bands-1) of the material table in force, n_rows
 * rows each.  Row r of T_b is row r of the table with ior = iors[b * n_rows + r] (band-major) and the reciprocal 1.0f / ior that
 * rr_set_materials would store for it; sigma_a is unchanged.  weights: n_bands x 3 floats, the weight of band b's colour per channel;
 * NULL: all 1.  1 <= n_bands <= RR_MAX_SAMPLES, every ior finite and > 0, every weight finite (negative weights are allowed, as in
 * rr_band): RR_ERR_INVALID_ARGUMENT otherwise, and the set in force stays.  RR_ERR_STATE when no table is set.  n_bands == 0 clears
 * the set.  The context owns the copies; the call waits for the context's stream, like rr_set_materials.  rr_set_materials clears
 * the set, because the row count may have changed.  Without a set there is exactly one band, band 0: the table in force with
 * weights 1.  Only the two calls below read the set.
 *
 * The frame.  Sample k of a pixel has the sub-pixel position samples[k].offset (as rr_render_samples' offsets, each in [0, 1]), the
 * lens offset samples[k].lens_offset (as rr_render_lens' lens offsets, each in [-1, 1]) and the band samples[k].band, which must be
 * below the number of bands in force; pad is ignored.  Let c_k be what rr_shade_rays_nested returns for the rays of
 * rr_host_lens_rays(constants, width, height, offset_k, lens_offset_k, lens) with T_(band_k) as the table in force; with lens ==
 * NULL or radius == 0 the rays are those of rr_host_camera_rays(constants, width, height, offset_k) and the lens offsets are not
 * looked at.  Channel ch of the pixel resolves in fp32, one rounding per operation and nothing fused, by rr_render_spectral's rule:
 *   p_k = weights[band_k][ch] * c_k[ch]
 *   sum = p_0, then sum = sum + p_k in sample order
 *   out = sum / (float)n_samples
 * and n_rays[i] is the sum of the samples' TraceRay counts.  Consequences, all byte for byte in colours, RGBA8 and counts:
 *   - no lens, band 0 throughout and no band set (or a one-band set that repeats the table, weights 1): rr_render_nested with the
 *     same offsets;
 *   - one closed convex instance of row { ior, 0, 0, 0 }, no band set, a lens: rr_render_lens under params->ior = ior;
 *   - the same scene, no lens, a band set made from rr_host_spectral_bands(B, ior, abbe): rr_render_spectral with that band table
 *     in the same sample order.
 * The last two hold where culled and unculled TraceRay agree for every ray used, as the reduction of the nested calls does.
 *
 * samples: host array of n_samples records, not NULL; 1 <= n_samples <= RR_MAX_SAMPLES.  lens: NULL for a pinhole, else validated as
 * by rr_render_lens.  A lens disk must lie outside every instance: the rays start in air (the nested calls do not cover a start
 * inside a medium).  Blocks of 8 x 8 pixels outside rr_host_lens_screen_rect of the scene (lens == NULL: rr_host_screen_rect) are
 * shaded as one Miss per sample on that sample's own direction, counted as one ray and weighted like any other sample;
 * RR_DISPATCH_DEBUG_NO_CULL traces them, with the same output.  State and parameters as rr_render_nested[_device]: RR_ERR_STATE
 * without a built TLAS or without a table, the same checks of the instances' rows, params->ior ignored, not a dispatch,
 * rr_set_tile_partition ignored; outputs, tone mapping and alignment rules as rr_render_samples[_device].  The _device variant is
 * stream-ordered on the context's stream and neither synchronises nor allocates: the band set is already on the device.
 * Only the nested tree is offered: on closed, pairwise disjoint instances it is the material tree byte for byte. */
typedef struct rr_composed_sample { float offset[2]; float lens_offset[2]; uint32_t band; uint32_t pad[3]; } rr_composed_sample; /* 32 bytes */
int  rr_set_material_bands(rr_context* ctx, const float* iors, const float* weights, uint32_t n_bands);
int  rr_render_composed(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                        const rr_dispatch_params* params, const rr_composed_sample* samples, uint32_t n_samples, const rr_lens* lens,
                        float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_render_composed_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                               const rr_dispatch_params* params, const rr_composed_sample* samples, uint32_t n_samples,
                               const rr_lens* lens, void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- shutter frames: motion blur over captured scene keys (present from ABI version 3) --------------------------------------------
 * Time as one more sample dimension.  The context keeps up to RR_MAX_SCENE_KEYS frozen copies of the scene, "keys"; a shutter
 * frame is a composed frame whose every sample also names the key it is traced in.
 *
 * Keys.  rr_capture_scene_key(ctx, key) freezes the scene that a render call issued at that point would trace: it copies the
 * instance records, the flattened node pool and the triangle and normal pools (for a scene without a top level: the mesh's own
 * nodes, triangles and normals) into buffers the key owns, device to device on the context's stream, so a capture right after
 * rr_build_tlas_ex(.., RR_BUILD_PERFORM_UPDATE) sees that update; nothing is waited for unless a buffer of the key must grow.
 * RR_ERR_STATE where rr_render_nested would refuse the scene's state (no TLAS, or a BLAS rebuilt or updated since the TLAS);
 * RR_ERR_INVALID_ARGUMENT for key >= RR_MAX_SCENE_KEYS; after RR_ERR_OUT_OF_MEMORY the key is empty.  Capturing into a used key
 * replaces it and reuses its buffers where they are large enough.  The live scene is never touched, and no later build, refit,
 * vertex update or new scene changes a key.  A key holds geometry and the instances' material rows, nothing else: the environment
 * map, the material table and the band set are the context's at the time of the render call.
 * rr_release_scene_key frees one key (RR_ALL_SCENE_KEYS: every key; an empty key is fine) after waiting for the context's stream.
 * rr_scene_key_info: captured (0: everything else is 0), top_level (0: one identity instance, traced without a top level),
 * instance and triangle counts, the world-space bounds (lo.xyz, hi.xyz), the deepest traversal stack the key can need, the largest
 * material row among its instances, and the bytes of device memory it holds.
 *
 * The frame.  rr_render_shutter[_device] is rr_render_composed[_device] with one word added: sample k is shaded as
 * rr_shade_rays_nested shades the rays of rr_host_lens_rays (without a lens: rr_host_camera_rays) in the scene of key samples[k].key
 * under the band table samples[k].band, and the pixel resolves by the same rule, ((w_0 * c_0 + w_1 * c_1) + ...) / n_samples with
 * every operation rounded once.  Outputs, tone mapping, ray counts, device pointers and their alignment as rr_render_composed.
 * Refused as rr_render_composed refuses its arguments, and with RR_ERR_INVALID_ARGUMENT: a key >= RR_MAX_SCENE_KEYS or not
 * captured; non-zero pad; keys of one frame that disagree on top_level; a key whose max_material is not below the rows of the
 * table in force or is above RR_NESTED_MAX_MATERIAL.  The live scene need not be built: no key, no frame.  The camera and every
 * lens point must lie outside every instance of every key used.  Blocks of 8 x 8 pixels outside the screen rectangle of the union
 * of the used keys' bounds are one Miss per sample, as in rr_render_composed; RR_DISPATCH_DEBUG_NO_CULL traces them.  Nothing is
 * allocated, copied or waited for by the _device variant.
 * Not covered: a camera per key, interpolation between keys, more than RR_MAX_SAMPLES samples. */
#define RR_MAX_SCENE_KEYS 16
#define RR_ALL_SCENE_KEYS 0xffffffffu
struct rr_scene_key_info {              /* a tag only: the call below has the name, so write `struct rr_scene_key_info` */
    uint32_t captured, top_level, n_instances, n_triangles;
    float    bounds[6];
    uint32_t stack_need, max_material;
    uint64_t bytes;
};
typedef struct rr_shutter_sample { float offset[2]; float lens_offset[2]; uint32_t band; uint32_t key; uint32_t pad[2]; } rr_shutter_sample; /* 32 bytes */
int  rr_capture_scene_key(rr_context* ctx, uint32_t key);
int  rr_release_scene_key(rr_context* ctx, uint32_t key);
int  rr_scene_key_info(rr_context* ctx, uint32_t key, struct rr_scene_key_info* out);
int  rr_render_shutter(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                       const rr_dispatch_params* params, const rr_shutter_sample* samples, uint32_t n_samples, const rr_lens* lens,
                       float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_render_shutter_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                              const rr_dispatch_params* params, const rr_shutter_sample* samples, uint32_t n_samples,
                              const rr_lens* lens, void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- lit shutter frames: opaque surfaces, lights and soft shadows per sample (additive; the ABI version stays 3) -------------------
 * rr_render_shutter's frame over rr_shade_rays_surfaces' hit groups: the lit scene through the lens, with motion blur, dispersion
 * and -- one more per-sample entry -- a point on every light, so that the fold over the samples which integrates the aperture and
 * the shutter integrates the lights' areas too.  No random numbers: every sample is stated by its record.
 *
 * Shapes.  rr_set_light_shapes gives light i of the set in force (rr_set_lights) the two edge vectors ex, ey of row i.  n == 0
 * clears the table; any other n must equal the number of lights in force.  RR_ERR_INVALID_ARGUMENT: another n, a NULL table with
 * n > 0, an ex or ey that is not finite, a non-zero pad; a refused table leaves the one in force.  rr_set_lights clears the table.
 * The call waits for the context's stream, as rr_set_lights does; the table travels by value with every launch.  Only the two
 * render calls below read it.
 *
 * Moved lights.  rr_host_moved_lights(lights, shapes, n, lu, lv, out) states the only new arithmetic, in fp32:
 *   out[i].v[c] = fmaf(lv, shapes[i].ey[c], fmaf(lu, shapes[i].ex[c], lights[i].v[c]))        each fmaf rounded once
 * and copies everything else of row i.  With shapes == NULL the rows are copied unchanged (a -0 in v stays -0).  Both light kinds
 * are moved alike; a moved directional v is used AS GIVEN, as rr_set_lights has it.  Needs no context; out may be lights.
 * RR_ERR_INVALID_ARGUMENT for a NULL lights or out with n > 0.
 *
 * The frame.  rr_render_lit[_device] takes rr_render_shutter[_device]'s arguments with rr_lit_sample records: a shutter sample whose
 * pad has a meaning, the light offset (lu, lv), each in [-1, 1].  Sample k is shaded as rr_shade_rays_surfaces shades the rays of
 * rr_host_lens_rays for sample k (without a lens: rr_host_camera_rays) in the scene of key samples[k].key, under the band table
 * samples[k].band, the surface table and ambient term in force, and the lights
 *   rr_host_moved_lights(lights in force, shape table in force or NULL, n, light_offset_k[0], light_offset_k[1]).
 * The pixel resolves as rr_render_shutter's, ((w_0 * c_0 + w_1 * c_1) + ...) / n_samples with every operation rounded once; shadow
 * rays count in n_rays.  Outputs, tone mapping, device pointers, alignment, culling of background blocks (a culled block is one Miss
 * per sample and looks at no table and no light) and RR_DISPATCH_DEBUG_NO_CULL as rr_render_shutter.  Nothing is allocated, copied
 * or waited for by the _device variant.
 * Refused: everything rr_render_shutter refuses, with the same codes (its pad check has nothing left to look at); and with
 * RR_ERR_INVALID_ARGUMENT a light offset outside [-1, 1], NaN included, whether or not a shape table is set; a sample for which a
 * moved v is not finite, or for which a moved directional light has v == (0, 0, 0).
 * Reductions, byte for byte in colours, RGBA8 and counts: with no surface table, or with every row glass, rr_render_shutter on the
 * same records; with one key that is a capture of the live scene, no lens, no band set and no shape table (or one of zeros),
 * rr_render_surfaces on the samples' positions.
 * Stated limits: a shaped light is a rectangle of point emitters -- there is no cosine at the light and no normalisation by its
 * area; the caller's radiance is per sample, and the / n_samples of the resolve averages it.  Any accepted hit still occludes,
 * unless rr_set_shadow_steps (below) says otherwise.
 * Not covered: a camera per key, textures, environment lighting of opaque surfaces; and of a shadow ray that passes glass:
 * Fresnel loss and bending at the interfaces, absorption beyond its last hit, caustics. */
typedef struct rr_light_shape { float ex[3]; float ey[3]; uint32_t pad[2]; } rr_light_shape;                                        /* 32 bytes */
typedef struct rr_lit_sample { float offset[2]; float lens_offset[2]; uint32_t band; uint32_t key; float light_offset[2]; } rr_lit_sample; /* 32 bytes */
int  rr_set_light_shapes(rr_context* ctx, const rr_light_shape* shapes, uint32_t n);
int  rr_host_moved_lights(const rr_light* lights, const rr_light_shape* shapes, uint32_t n, float lu, float lv, rr_light* out);
int  rr_render_lit(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                   const rr_dispatch_params* params, const rr_lit_sample* samples, uint32_t n_samples, const rr_lens* lens,
                   float* rgba32f, uint8_t* rgba8, uint32_t* n_rays);
int  rr_render_lit_device(rr_context* ctx, uint32_t width, uint32_t height, const rr_scene_constants* constants,
                          const rr_dispatch_params* params, const rr_lit_sample* samples, uint32_t n_samples, const rr_lens* lens,
                          void* d_rgba32f, void* d_rgba8, void* d_n_rays);

/* ---- transparent shadows: shadow rays pass glass and take its tint (additive; the ABI version stays 3) ------------------------------
 * Opt-in.  rr_set_shadow_steps(ctx, K) sets shadow_steps, 0 <= K <= RR_SHADOW_MAX_STEPS.  K = 0, the setting after rr_create,
 * changes nothing anywhere: step b of the opaque hit group stands as written above.  With K >= 1 the shadow ray of step b is a
 * straight WALK through the glass between the opaque hit and the light, attenuated by what it crosses and stopped only by an opaque
 * surface -- a glass of tinted water casts a tinted shadow, not a black one and not none.  The setting is read by the four _surfaces
 * calls and by rr_render_lit[_device], at the call; nothing else reads it, and rr_set_lights / rr_set_surfaces / rr_set_materials
 * leave it alone.  It travels by value with every launch, so the setter waits for nothing.  K > RR_SHADOW_MAX_STEPS is
 * RR_ERR_INVALID_ARGUMENT and the setting in force stays.  rr_get_shadow_steps reads the setting in force.
 *
 * The contract, with K >= 1, for a light the hit faces (cs > 0; Ld, far, g as in step b).  One rounding per written operation,
 * fmaf only where written:
 *   Start.  T = (1, 1, 1), Ls = L (the media list of the radiance ray at the hit), Xs = X, fs = far.
 *   Each of up to K calls: TraceRay(Xs, Ld, [tmin_secondary, fs], cull flags 0, closest hit, InstanceInclusionMask = shadow_mask).
 *   Each call counts one ray in n_rays.
 *     Miss: the walk ends lit.
 *     Hit on a row whose surface kind is opaque: the walk ends occluded; the light adds nothing.
 *     Hit on a glass row m at t:
 *       1. c = top(Ls).  If c is not air, T.ch = T.ch * rr_expf_neg(-(sigma_c.ch * t)): the medium CROSSED, as in the nested calls.
 *       2. Ls = front ? push(Ls, m) : remove(Ls, m), with the nested calls' rules: a push onto a full list is dropped, removing an
 *          absent row is a no-op.
 *       3. Xs.ch = fmaf(t, Ld.ch, Xs.ch) and fs = fs - t.
 *       4. If !(fs > tmin_secondary), the walk ends lit.
 *       5. If this was the K-th call, the walk ends occluded: the cap is conservative.
 *   Lit.  f = cs * g and E.ch = fmaf(radiance.ch, f * T.ch, E.ch).
 * A scene without a top level walks its one instance (mask 1, row of instance 0) the same way if shadow_mask & 1; otherwise the
 * first call misses.  In rr_render_lit the walk goes towards the light as moved for the sample, so a shaped light's soft shadow
 * takes the glass's colour.
 *
 * Reductions, byte for byte in colours, RGBA8 and ray counts:
 *   - any K equals K = 0 wherever no shadow ray's first hit is glass, since f * 1.0f == f;
 *   - K = 1 equals K = 0 on every scene, but for a glass hit closer than tmin_secondary to the far end of its interval, which
 *     step 4 lets through.
 * Not modelled: Fresnel loss and bending at the interfaces -- no normal is fetched on the walk, which is straight and loses only
 * what the media absorb; absorption beyond the last hit, for a light inside a medium; caustics.  Before this setting existed the
 * lists above named "transparent shadows" among what is not covered; the advice given there, an InstanceMask bit the light's
 * shadow_mask lacks, still makes glass cast no shadow at all. */
#define RR_SHADOW_MAX_STEPS 16
int  rr_set_shadow_steps(rr_context* ctx, uint32_t k);
int  rr_get_shadow_steps(rr_context* ctx, uint32_t* k);

/* Miss on caller-supplied ray directions (host arrays of n x 3 floats in, n x 3 floats out): the equirectangular lookup
 * of RayTracing.hlsl:127-137 in isolation -- atan2 / acos, the division by the literal 3.14159, the float-to-uint texel
 * address and the zero returned outside the texture (reached at atan2 = pi and at r.y = -1); used by the parity tests. */
int  rr_env_lookup(rr_context* ctx, const float* dirs, uint32_t n, float* rgb);

/* Introspection for tests: copies the packed BLAS of a mesh to host.  nodes: n_nodes*64 B
 * (two child boxes + two child refs), tris: n_tris*48 B (v0,e1,e2 with prim id in v0.w). */
int  rr_download_blas(rr_context* ctx, uint32_t mesh_id, void* nodes, uint32_t* n_nodes,
                      void* tris, uint32_t* n_tris);

/* The same hierarchy as the traversal kernels read it: n_nodes*32 B, per node six words holding one slab plane
 * of both children as IEEE half-precision cell counts q on the BLAS's grid (child 0 in the low half, child 1 in the
 * high half; order lox,loy,loz,hix,hiy,hiz), then the two child refs (>= 0: byte offset of an internal node, < 0:
 * leaf ~index).  grid_org_cell: origin xyz (the centre of the bounds) then cell size xyz (plane = org + q*cell).
 * Every stored box contains its fp32 box. */
int  rr_download_qnodes(rr_context* ctx, uint32_t mesh_id, void* qnodes, uint32_t* n_nodes, float grid_org_cell[6]);

/* The top level of the scene, read only: nodes: n_nodes*64 B, the fp32 hierarchy over the instances' world boxes as
 * rr_download_blas gives a BLAS (n_nodes = instances - 1, or 1 for one instance; a leaf ref is ~(triangles of the scene's
 * distinct BLASes + instance index)); qnodes: n_nodes*32 B, the same nodes as the traversal kernels read them from the head
 * of the scene's pool, on the scene grid returned in grid_org_cell (layout and meaning as rr_download_qnodes; internal refs
 * are byte offsets into the pool).  Either pointer may be NULL.  Waits for the context's stream.  RR_ERR_STATE without a built
 * TLAS (none yet, or invalidated by a BLAS build). */
int  rr_download_tlas(rr_context* ctx, void* nodes, void* qnodes, uint32_t* n_nodes, float grid_org_cell[6]);

/* ---- pure host helpers (no device, no context) --------------------------------------------- */
void rr_default_dispatch_params(rr_dispatch_params* p);
/* Where the box {lo[3], hi[3]} can be seen at all with any of the n constants (GenerateCameraRay, RayTracing.hlsl:27-40):
 * rect = {x0, y0, x1, y1} in pixels, aligned outward to 8 with 8 pixels of margin; the whole frame whenever the projection
 * cannot be trusted (camera inside or beside the box, singular or badly conditioned proj_inv, constants == NULL).  The render
 * kernels shade blocks outside it as one Miss without TraceRay. */
int  rr_host_screen_rect(const float bounds[6], const rr_scene_constants* constants, uint32_t n, uint32_t width, uint32_t height,
                         uint32_t rect[4]);
/* Multi-GPU tile partition that only moves what has to move: the tiles that touch the rectangle ("mesh tiles", raster order
 * inside the rectangle, index i) are dealt to the ranks in turn (rank0_rounds: rank 0 takes fewer, see the struct), each rank's
 * tiles filling the slots of its tile buffer in order; all the other tiles
 * ("background tiles": one Miss per pixel, a tenth of the work and two thirds of the bytes of the reference's views) belong to
 * rank 0, in raster order, and never cross a link.  rect_w == 0: no usable rectangle, every tile is a mesh tile. */
int  rr_host_mesh_partition(const float bounds[6], const rr_scene_constants* constants, uint32_t n, uint32_t width, uint32_t height,
                            uint32_t world, rr_mesh_partition* out);
/* mesh tile `mesh_index` (raster order inside the rectangle) -> the rank it is dealt to and its slot in that rank's buffer;
 * the number of mesh tiles a rank holds */
int  rr_host_mesh_tile_home(const rr_mesh_partition* part, uint32_t mesh_index, uint32_t* rank, uint32_t* slot);
uint32_t rr_host_mesh_tiles_of_rank(const rr_mesh_partition* part, uint32_t rank);
/* RefractionDemo.cpp:559-566: camera constants for an orbit angle.  The reference's literals are
 * fov_y = float(52.0/180.0*3.1415), aspect = 1.333f, zn = 1, zf = 125; frame k uses angle 0.01*(k+1). */
int  rr_host_camera_orbit(float angle, float fov_y, float aspect, float zn, float zf,
                          rr_scene_constants* out);
/* D3D's standard multisample patterns for n_samples = 1, 2, 4, 8, 16 (RR_ERR_INVALID_ARGUMENT otherwise): 2 * n_samples floats
 * x0, y0, x1, y1, ..., sample i at 0.5 + k / 16 per axis, k in -8..7.  What rr_render_samples uses for offsets == NULL. */
int  rr_host_sample_pattern(uint32_t n_samples, float* offsets);
/* Bytes of the workspace rr_render_adaptive_device needs for a width x height frame; 0 for a width or height that is 0 or above
 * 32768.  Monotone in both. */
uint64_t rr_host_adaptive_workspace_bytes(uint32_t width, uint32_t height);
/* GenerateCameraRay for every pixel of a width x height frame (row-major) with its literal 0.5 replaced by (ox, oy), both in
 * [0, 1]: the primary rays rr_render_samples takes for that offset -- with (0.5, 0.5) those of a dispatch -- as rr_ray records
 * over [tmin, tmax] with flags 0 and instance_mask 0xff.  width, height: 1..32768. */
int  rr_host_camera_rays(const rr_scene_constants* c, uint32_t width, uint32_t height, float ox, float oy, float tmin, float tmax,
                         rr_ray* rays);
/* A band table for rr_render_spectral, 1 <= n <= RR_MAX_SAMPLES records.  n == 1: { ior_d, 1, 1, 1 }.  Otherwise band i has the
 * wavelength l_i = 400 + (i + 0.5) / n * 300 nm and, by Cauchy's law, ior = A + B / l^2 with
 *   B = (ior_d - 1) / (abbe * (1 / 486.1^2 - 1 / 656.3^2)),  A = ior_d - B / 587.6^2
 * (ior_d at the d line, abbe the Abbe number over the F and C lines), computed in double and rounded once.  The weights are three
 * tent functions of half-width 100 nm centred at 650 nm (R), 550 nm (G) and 450 nm (B), t_c(l) = max(0, 1 - |l - centre_c| / 100),
 * each channel normalised in double so that its n weights sum to n, weight = (float)(t_c(l_i) * n / sum_i t_c(l_i)): a white
 * environment stays white.  A stated convention, not colorimetry: bring a table of your own for that.  ior_d finite and > 0; abbe
 * > 0, +inf allowed (every ior is ior_d then); a table with an ior that is not finite and > 0 (abbe too small) is not handed out
 * (RR_ERR_INVALID_ARGUMENT, as n == 0, n > RR_MAX_SAMPLES or bands == NULL). */
int  rr_host_spectral_bands(uint32_t n, float ior_d, float abbe, rr_band* bands);
/* exp(x) for x <= 0 as the material kernels compute Beer-Lambert absorption: if (!(x > -87)) 0; k = floorf(fmaf(x, 1.44269504f,
 * 0.5f)); r = fmaf(k, -0.693359375f, x); r = fmaf(k, 2.12194440e-4f, r); p by Horner with fmaf over 1.9875691500e-4,
 * 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1; y = fmaf(p, r * r, r) + 1.0f; y times 2^k
 * built from the exponent bits.  Within 1 ulp of the correctly rounded value on [-87, 0]. */
float rr_host_expf_neg(float x);
/* The rays of rr_render_lens for one (pixel offset, lens offset) pair, every pixel of a width x height frame, row-major, as
 * rr_ray records shaped like those of rr_host_camera_rays: ox, oy in [0, 1], lx, ly finite and in [-1, 1], lens as rr_render_lens
 * takes it (RR_ERR_INVALID_ARGUMENT otherwise).  radius == 0: exactly rr_host_camera_rays. */
int  rr_host_lens_rays(const rr_scene_constants* c, uint32_t width, uint32_t height, float ox, float oy, float lx, float ly,
                       const rr_lens* lens, float tmin, float tmax, rr_ray* rays);
/* The built-in lens offsets of rr_render_lens, 1 <= n_samples <= RR_MAX_SAMPLES: 2 * n_samples floats, point i of a golden-angle
 * spiral inside the unit disk, r = sqrtf((i + 0.5f) / n), theta = i * 2.3999632f, (r * cosf(theta), r * sinf(theta)). */
int  rr_host_lens_pattern(uint32_t n_samples, float* lens_offsets);
/* rr_host_screen_rect for a lens: where the box can be seen from any point of the lens disk -- the union of the rectangles of five
 * pinhole cameras, the lens centre and the corners +-A +-B of the square round the disk, each at camera_loc + off with the centre
 * column of proj_inv reduced by off / s.  The whole frame whenever one of them cannot be trusted or constants == NULL; radius == 0
 * gives the pinhole's rectangle.  A lens rr_render_lens refuses is RR_ERR_INVALID_ARGUMENT. */
int  rr_host_lens_screen_rect(const float bounds[6], const rr_scene_constants* constants, const rr_lens* lens, uint32_t width,
                              uint32_t height, uint32_t rect[4]);
/* Mesh::load, Mesh.cpp:6-37.  Arrays are malloc'ed, release with rr_host_free.  A file that cannot
 * be opened returns RR_ERR_IO (Mesh::load returns false). */
int  rr_host_mesh_load_obj(const char* filename, rr_vertex** verts, uint32_t* n_verts,
                           uint32_t** indices, uint32_t* n_indices);
/* Additive hardening behind the same output format: with RR_OBJ_HARDENED faces may be
 * polygons (fan-triangulated), corners may be "v", "v/vt", "v//vn" or "v/vt/vn", indices may be
 * negative; a missing uv is (0,0), a face without normals gets its flat winding normal.
 * flags = 0 is exactly rr_host_mesh_load_obj. */
#define RR_OBJ_HARDENED 0x1u
int  rr_host_mesh_load_obj_ex(const char* filename, uint32_t flags, rr_vertex** verts, uint32_t* n_verts,
                              uint32_t** indices, uint32_t* n_indices);
/* stbi_loadf(file,&x,&y,&n,req_comp) as called at RefractionDemo.cpp:111, for the two formats the demo's
 * environment map exists in: Radiance .hdr (flat and RLE scanlines) and .png (1..16-bit gray / RGB / palette,
 * with or without alpha, plain or Adam7-interlaced), LDR expanded with pow(v/255, 2.2) as stb does.
 * NARROWER than stb_image (stb_image.h:1491): JPEG, BMP, TGA, PSD, GIF, PIC and PNM files are refused --
 * NULL, like any other failure (the reference ignores load failures; the C++ mirror reports them). */
float* rr_host_image_loadf(const char* filename, int* x, int* y, int* channels_in_file, int req_comp);
/* Radiance RLE .hdr writer (the reference's envmap.hdr is missing from the mount). */
int  rr_host_image_write_hdr(const char* filename, int w, int h, const float* rgb);
void rr_host_free(void* p);
/* RR_OK if every position of the n vertices is finite and |x|, |y|, |z| <= 1e18 (what rr_upload_mesh requires),
 * RR_ERR_INVALID_ARGUMENT otherwise; *first_bad (may be NULL) receives the index of the first offending vertex. */
int  rr_host_validate_positions(const rr_vertex* verts, uint32_t n_verts, uint32_t* first_bad);
uint32_t rr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RRDXR_H */
