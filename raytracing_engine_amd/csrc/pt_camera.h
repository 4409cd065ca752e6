// pt_camera.h — path B, device side: from a path to its pixel and its camera ray.  The counter-based RNG of spec §6.2 (the camera
// ray's sub-pixel offset is its first use; pt_shade draws every later number from it), the Morton pixel slots and the camera ray.
// Used by the wavefront stages (path_b.hip: pt_generate, pt_shade, pt_resolve) and by the packet kernels (pt_packet.hip), which make
// their own camera rays.  Only __device__ __forceinline__ functions: every unit that includes this compiles its own copy into its kernels.
#pragma once
#include "rt_device_math.h"
#include "rt_internal.h"

namespace rt {
using namespace rtk;

// ---- spec §6.2: counter-based RNG -------------------------------------------------------------
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t path_key(uint32_t pixel, uint32_t sample, uint32_t seed) {
    return hash32(hash32(pixel + hash32(seed)) + sample);
}
__device__ __forceinline__ float rnd(uint32_t key, uint32_t depth, uint32_t dim) {
    const uint32_t h = hash32(key + (depth * 8u + dim + 1u) * 0x9e3779b9U);
    return (float)(h >> 8) * 0x1p-24f;
}

// ---- pixel slots ---------------------------------------------------------------------------------
// slot = owned_tile * 4096 + m, m = Morton code of (lx, ly) inside the 64x64 tile: 64 consecutive
// paths cover a compact pixel block, so camera rays of a wave stay coherent.
__device__ __forceinline__ uint32_t compact1by1(uint32_t x) {
    x &= 0x55555555u;
    x = (x ^ (x >> 1)) & 0x33333333u;
    x = (x ^ (x >> 2)) & 0x0f0f0f0fu;
    x = (x ^ (x >> 4)) & 0x00ff00ffu;
    x = (x ^ (x >> 8)) & 0x0000ffffu;
    return x;
}
__device__ __forceinline__ bool slot_pixel(const PtFrame& f, uint32_t slot, uint32_t& px, uint32_t& py, uint32_t& lx, uint32_t& ly, uint32_t& k) {
    k = slot >> 12;
    const uint32_t m = slot & 4095u;
    lx = compact1by1(m);
    ly = compact1by1(m >> 1);
    const uint32_t tile = f.part.rank + k * f.part.n_ranks;
    const uint32_t ty = tile / f.part.tiles_x, tx = tile - ty * f.part.tiles_x;
    px = tx * RT_TILE + lx;
    py = ty * RT_TILE + ly;
    return px < f.width && py < f.height;
}

// camera ray of sample s of pixel (px, py): fragment.glsl:129-133 with the pixel-centre 0.5 replaced by a random offset
__device__ __forceinline__ v3 camera_dir(const PtFrame& f, uint32_t px, uint32_t py, uint32_t s) {
    const uint32_t key = path_key(py * f.width + px, s, f.seed);
    const float nx = ((((float)px + rnd(key, 0, 0)) * 2.0f) / (float)f.width - 1.0f) * f.cam.ratio[0];
    const float ny = ((((float)py + rnd(key, 0, 1)) * 2.0f) / (float)f.height - 1.0f) * f.cam.ratio[1];
    return normalize(rotate_q(f.cam.rot[0], f.cam.rot[1], f.cam.rot[2], f.cam.rot[3], mk(nx, 1.0f, ny)));
}

}  // namespace rt
