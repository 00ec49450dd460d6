// rr_frame.hip -- the kernels around a frame that never touch a BVH: the screen-coordinate tables the render kernels read, and
// the assembly of gathered tiles into rasters (multi-GPU sharding).
#include <hip/hip_runtime.h>
#include "rr_launch.h"

namespace rr {

// screen coordinate of a pixel centre (GenerateCameraRay, RayTracing.hlsl:29-33), the same operations for every pixel of a column /
// row: k_screen_tables evaluates them once per column and row, the render kernels read the two tables
__device__ __forceinline__ float screen_coord(uint32_t i, uint32_t n, bool flip)
{
    const float p = (float)i + 0.5f;
    const float s = p / (float)n * 2.0f - 1.0f;
    return flip ? -s : s;
}

// GenerateCameraRay's per-column and per-row screen coordinates (RayTracing.hlsl:29-33): out[0..W) = sx, out[W..W+H) = sy
__global__ __launch_bounds__(256) void k_screen_tables(float* out, uint32_t W, uint32_t H)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < W) out[i] = screen_coord(i, W, false);
    else if (i < W + H) out[i] = screen_coord(i - W, H, true);
}

// rank 0 after the RCCL gather: [world][max_tiles][32*32] RGBA8 -> W*H raster
__global__ __launch_bounds__(256) void k_assemble_tiles(const uint32_t* __restrict__ gathered, uint32_t* __restrict__ frame,
                                                        uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles,
                                                        uint32_t world, uint32_t max_tiles)
{
    const uint32_t tile = blockIdx.x >> 2, strip = blockIdx.x & 3u;
    if (tile >= n_tiles) return;
    const uint32_t rank = tile % world, tile_local = tile / world;
    const uint32_t px = threadIdx.x & 31u, py = strip * 8u + (threadIdx.x >> 5);
    const uint32_t x = (tile % tiles_x) * TILE + px, y = (tile / tiles_x) * TILE + py;
    if (x < W && y < H)
        frame[(size_t)y * W + x] = gathered[((size_t)rank * max_tiles + tile_local) * (TILE * TILE) + py * TILE + px];
}

__global__ __launch_bounds__(256) void k_assemble_frames(const uint32_t* __restrict__ gathered, uint32_t* __restrict__ frames,
                                                         uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles,
                                                         uint32_t world, size_t rank_stride, size_t frame_stride,
                                                         size_t out_stride)
{
    const uint32_t tile = blockIdx.x >> 2, strip = blockIdx.x & 3u, f = blockIdx.y;
    if (tile >= n_tiles) return;
    const uint32_t rank = tile % world, tile_local = tile / world;
    const uint32_t px = threadIdx.x & 31u, py = strip * 8u + (threadIdx.x >> 5);
    const uint32_t x = (tile % tiles_x) * TILE + px, y = (tile / tiles_x) * TILE + py;
    if (x < W && y < H)
        frames[f * out_stride + (size_t)y * W + x] =
            gathered[rank * rank_stride + f * frame_stride + (size_t)tile_local * (TILE * TILE) + py * TILE + px];
}

// the same for RGB8 tiles (3 bytes per pixel in the gathered buffers); strides in bytes.  One workgroup per tile and
// frame, one thread per group of four pixels of a tile row: 12 contiguous bytes in, one 16-byte store out (rank 0 runs
// this for every gathered batch while it also renders its own share, so it is written for bandwidth).
// vec4: W % 4 == 0 (a group never straddles the right edge and its raster address is 16-byte aligned).
template <bool VEC4>
__global__ __launch_bounds__(256) void k_assemble_frames_rgb8(const uint8_t* __restrict__ gathered, uint32_t* __restrict__ frames,
                                                              uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles,
                                                              uint32_t world, size_t rank_stride_b, size_t frame_stride_b,
                                                              size_t out_stride)
{
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    if (tile >= n_tiles) return;
    const uint32_t rank = tile % world, tile_local = tile / world;
    const uint32_t py = threadIdx.x >> 3, px = (threadIdx.x & 7u) * 4u;
    const uint32_t x = (tile % tiles_x) * TILE + px, y = (tile / tiles_x) * TILE + py;
    if (y >= H || x >= W) return;
    const uint8_t* p = gathered + rank * rank_stride_b + f * frame_stride_b + ((size_t)tile_local * (TILE * TILE) + py * TILE + px) * 3;
    const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);                 // 12-byte group: 4-byte aligned
    const uint32_t w0 = p4[0], w1 = p4[1], w2 = p4[2];
    uint4 o;
    o.x = (w0 & 0x00ffffffu) | 0xff000000u;
    o.y = (((w0 >> 24) | (w1 << 8)) & 0x00ffffffu) | 0xff000000u;
    o.z = (((w1 >> 16) | (w2 << 16)) & 0x00ffffffu) | 0xff000000u;
    o.w = (w2 >> 8) | 0xff000000u;
    uint32_t* dst = frames + f * out_stride + (size_t)y * W + x;
    if (VEC4) {
        *reinterpret_cast<uint4*>(dst) = o;
    } else {
        dst[0] = o.x;
        if (x + 1 < W) dst[1] = o.y;
        if (x + 2 < W) dst[2] = o.z;
        if (x + 3 < W) dst[3] = o.w;
    }
}

// the mesh-tile partition's de-interleave (rr_mesh_partition): a tile inside the rectangle comes from the gathered buffer of the
// rank it was dealt to, any other tile from rank 0's own background tiles.  RGB8 in, RGBA8 rasters out; one workgroup per tile
// and frame, one thread per group of four pixels of a tile row.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_assemble_frames_mesh_rgb8(const uint8_t* __restrict__ gathered, const uint8_t* __restrict__ bg,
                                                                   uint32_t* __restrict__ frames, uint32_t W, uint32_t H, MeshPartDev mp,
                                                                   size_t rank_stride_b, size_t frame_stride_b, size_t bg_stride_b, size_t out_stride)
{
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    if (tile >= mp.n_tiles) return;
    const uint32_t tx = tile % mp.tiles_x, ty = tile / mp.tiles_x;
    const uint8_t* src;
    if (mp.rect_w == 0u || (tx >= mp.rect_x0 && tx < mp.rect_x0 + mp.rect_w && ty >= mp.rect_y0 && ty < mp.rect_y0 + mp.rect_h)) {
        const uint32_t i = mp.rect_w == 0u ? tile : (ty - mp.rect_y0) * mp.rect_w + (tx - mp.rect_x0);
        uint32_t rank, slot;
        mesh_deal_owner(i, mp.world, mp.rounds, rank, slot);
        src = gathered + (size_t)rank * rank_stride_b + f * frame_stride_b + (size_t)slot * (TILE * TILE * 3);
    } else {
        const uint32_t per_row = mp.tiles_x - mp.rect_w;
        uint32_t j;
        if (ty < mp.rect_y0) j = ty * mp.tiles_x + tx;
        else if (ty < mp.rect_y0 + mp.rect_h) j = mp.rect_y0 * mp.tiles_x + (ty - mp.rect_y0) * per_row + (tx < mp.rect_x0 ? tx : tx - mp.rect_w);
        else j = mp.rect_y0 * mp.tiles_x + mp.rect_h * per_row + (ty - mp.rect_y0 - mp.rect_h) * mp.tiles_x + tx;
        src = bg + f * bg_stride_b + (size_t)j * (TILE * TILE * 3);
    }
    const uint32_t py = threadIdx.x >> 3, px = (threadIdx.x & 7u) * 4u;
    const uint32_t x = tx * TILE + px, y = ty * TILE + py;
    if (y >= H || x >= W) return;
    const uint32_t* p4 = reinterpret_cast<const uint32_t*>(src + (py * TILE + px) * 3);
    const uint32_t w0 = p4[0], w1 = p4[1], w2 = p4[2];
    uint4 o;
    o.x = (w0 & 0x00ffffffu) | 0xff000000u;
    o.y = (((w0 >> 24) | (w1 << 8)) & 0x00ffffffu) | 0xff000000u;
    o.z = (((w1 >> 16) | (w2 << 16)) & 0x00ffffffu) | 0xff000000u;
    o.w = (w2 >> 8) | 0xff000000u;
    uint32_t* dst = frames + f * out_stride + (size_t)y * W + x;
    if (VEC4) *reinterpret_cast<uint4*>(dst) = o;
    else {
        dst[0] = o.x;
        if (x + 1 < W) dst[1] = o.y;
        if (x + 2 < W) dst[2] = o.z;
        if (x + 3 < W) dst[3] = o.w;
    }
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_screen_tables(float* out, uint32_t W, uint32_t H, hipStream_t s)
{
    hipLaunchKernelGGL(k_screen_tables, dim3((W + H + 255u) / 256u), dim3(256), 0, s, out, W, H);
    return hipGetLastError();
}

hipError_t launch_assemble_tiles(const uint32_t* gathered, uint32_t* frame, uint32_t W, uint32_t H, uint32_t tiles_x,
                                 uint32_t n_tiles, uint32_t world, uint32_t max_tiles, hipStream_t s)
{
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_assemble_tiles, dim3(n_tiles * 4u), dim3(256), 0, s, gathered, frame, W, H, tiles_x, n_tiles, world,
                       max_tiles);
    return hipGetLastError();
}

hipError_t launch_assemble_frames(const uint32_t* gathered, uint32_t* frames, uint32_t W, uint32_t H, uint32_t tiles_x,
                                  uint32_t n_tiles, uint32_t world, size_t rank_stride, size_t frame_stride,
                                  size_t out_stride, uint32_t n_frames, hipStream_t s)
{
    if (n_tiles == 0 || n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_assemble_frames, dim3(n_tiles * 4u, n_frames), dim3(256), 0, s, gathered, frames, W, H, tiles_x,
                       n_tiles, world, rank_stride, frame_stride, out_stride);
    return hipGetLastError();
}

hipError_t launch_assemble_frames_rgb8(const uint8_t* gathered, uint32_t* frames, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles,
                                       uint32_t world, size_t rank_stride_b, size_t frame_stride_b, size_t out_stride, uint32_t n_frames,
                                       hipStream_t s)
{
    if (n_tiles == 0 || n_frames == 0) return hipSuccess;
    const bool vec4 = (W % 4u) == 0u && (out_stride % 4u) == 0u && (reinterpret_cast<uintptr_t>(frames) % 16u) == 0u;
    if (vec4) hipLaunchKernelGGL(k_assemble_frames_rgb8<true>, dim3(n_tiles, n_frames), dim3(256), 0, s, gathered, frames, W, H, tiles_x,
                                 n_tiles, world, rank_stride_b, frame_stride_b, out_stride);
    else      hipLaunchKernelGGL(k_assemble_frames_rgb8<false>, dim3(n_tiles, n_frames), dim3(256), 0, s, gathered, frames, W, H, tiles_x,
                                 n_tiles, world, rank_stride_b, frame_stride_b, out_stride);
    return hipGetLastError();
}

hipError_t launch_assemble_frames_mesh_rgb8(const uint8_t* gathered, const uint8_t* bg, uint32_t* frames, uint32_t W, uint32_t H, const MeshPartDev& mp,
                                            size_t rank_stride_b, size_t frame_stride_b, size_t bg_stride_b, size_t out_stride, uint32_t n_frames, hipStream_t s)
{
    if (mp.n_tiles == 0 || n_frames == 0) return hipSuccess;
    const bool vec4 = (W % 4u) == 0u && (out_stride % 4u) == 0u && (reinterpret_cast<uintptr_t>(frames) % 16u) == 0u;
    if (vec4) hipLaunchKernelGGL(k_assemble_frames_mesh_rgb8<true>, dim3(mp.n_tiles, n_frames), dim3(256), 0, s, gathered, bg, frames, W, H, mp,
                                 rank_stride_b, frame_stride_b, bg_stride_b, out_stride);
    else      hipLaunchKernelGGL(k_assemble_frames_mesh_rgb8<false>, dim3(mp.n_tiles, n_frames), dim3(256), 0, s, gathered, bg, frames, W, H, mp,
                                 rank_stride_b, frame_stride_b, bg_stride_b, out_stride);
    return hipGetLastError();
}

} // namespace rr
