// t360_mapgen.hip -- projection kernel: one thread per output pixel evaluates the reference's
// transformPos / transformInputPos chain and writes
//   (a) the float warp map   (reference VideoFrameTransform.cpp:534-554, warpMats_[idx])
//   (b) the packed sample LUT the gather kernels read (what cv::remap's RemapInvoker derives
//       from a CV_32FC2 map on every call; here it is derived once).
//
// The per-pixel projection itself (transformPos / transformInputPos, bit-exact, with its attribution) lives in
// t360_project.h, which the posed gather (t360_posed.hip) evaluates too.  All output layouts of the public header:
// CUBEMAP_32, CUBEMAP_23_OFFCENTER, FLAT_FIXED, EQUIRECT, BARREL, BARREL_SPLIT, EAC_32; inputs EQUIRECT and CUBEMAP_32;
// all stereo packings; rotation and off-centre projection.  One lane per pixel.
#include <hip/hip_runtime.h>

#include "t360_internal.h"
#include "t360_project.h"

#pragma clang fp contract(off)

namespace t360 {

__global__ __launch_bounds__(256) void mapgen_kernel(MapGenParams P, float2* __restrict__ map,
                                                     LutEntry* __restrict__ lut) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (j >= P.map_w || i >= P.map_h) return;

  const float2 mc = project_pixel(P, P.rot, P.yaw_deg, P.pitch_deg, i, j);
  const size_t o = (size_t)i * P.map_w + j;
  map[o] = mc;
  lut[o] = quantize_map_coord(P.interp, mc.x, mc.y);
}

// host-callable launcher (C++ linkage inside the library)
hipError_t launch_mapgen(const MapGenParams& P, float2* map, LutEntry* lut, hipStream_t stream) {
  dim3 block(256, 1, 1);
  dim3 grid((P.map_w + 255) / 256, P.map_h, 1);
  hipLaunchKernelGGL(mapgen_kernel, grid, block, 0, stream, P, map, lut);
  return hipGetLastError();
}

// ---- synthetic noise generator (bench / tests): byte i = splitmix64(seed + i) >> 56 ----
__device__ __host__ inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void fill_noise_kernel(uint8_t* __restrict__ dst, int64_t n, uint64_t seed) {
  // 16 bytes per thread per step, grid-stride
  const int64_t nvec = n >> 4;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
       v += (int64_t)gridDim.x * blockDim.x) {
    uint32_t w[4];
    for (int k = 0; k < 4; k++) {
      uint32_t acc = 0;
      for (int b = 0; b < 4; b++) {
        const uint64_t idx = (uint64_t)(v * 16 + k * 4 + b);
        acc |= (uint32_t)(splitmix64(seed + idx) >> 56) << (8 * b);
      }
      w[k] = acc;
    }
    reinterpret_cast<uint4*>(dst)[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  // tail
  const int64_t tail0 = nvec << 4;
  const int64_t t = tail0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = (uint8_t)(splitmix64(seed + (uint64_t)t) >> 56);
}

hipError_t launch_fill_noise(uint8_t* dst, int64_t n, uint64_t seed, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) != 0) return hipErrorInvalidValue;  // uint4 stores
  int blocks = (int)((((n >> 4) + 255) / 256) < 4096 ? (((n >> 4) + 255) / 256) : 4096);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(fill_noise_kernel, dim3(blocks), dim3(256), 0, stream, dst, n, seed);
  return hipGetLastError();
}

}  // namespace t360
