// t360_posed.hip -- remap_posed_kernel: the gather with the projection folded in, one pose per frame
// (T360_transformFramesPosed, include/Transform360/t360_device.h).
//
// Every lane evaluates, for each of its 4 horizontally adjacent output pixels, the reference's projection for its frame's
// pose (project_pixel, t360_project.h -- the code mapgen_kernel runs), quantises it as cv::remap does
// (quantize_map_coord: the LutEntry lives in registers, never in memory), gathers one OpenCV-exact sample
// (sample<KS, TRANSPARENT>, t360_sample.h) and writes the byte.  No warp map and no LUT in HBM: a stored LUT would be
// 8 B read per output pixel against 1 B written.  The cost is the projection's VALU work (a few hundred instructions
// per pixel, correctly rounded divides and square roots, fdlibm atan2f / asinf): DESIGN.md 9.
//
// Workgroups of 16 x 16 lanes cover 64 x 16 px, so a wave is 64 x 4 px and neighbouring lanes' stencils share cache
// lines.  The pose of frame blockIdx.y comes from the kernel arguments (a wave-uniform scalar load).
#include <hip/hip_runtime.h>

#include "t360_internal.h"
#include "t360_kernels.h"
#include "t360_project.h"
#include "t360_sample.h"

#pragma clang fp contract(off)

namespace t360 {

// the chunk of poses rides in the kernel arguments: stay inside the 4 KiB a HIP launch passes
static_assert(sizeof(PosedArgs) <= 4096, "PosedArgs must fit the kernel argument segment");

namespace {

template <int KS, bool TRANSPARENT>
__global__ __launch_bounds__(256) void remap_posed_kernel(PosedArgs a) {
  int k = 0;
#pragma unroll
  for (int q = 1; q < kPosedMaxPlanes; q++)
    if (q < a.nplanes && (int)blockIdx.x >= a.plane[q].tile0) k = q;
  const PosedPlane& P = a.plane[k];
  const int t = (int)blockIdx.x - P.tile0;
  const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
  const int i = ty * kPosedTileH + (int)threadIdx.y;
  const int x0 = tx * kPosedTileW + (int)threadIdx.x * 4;
  const int dw = P.gen.map_w;
  if (i >= P.gen.map_h || x0 >= dw) return;
  const int f = blockIdx.y;
  const PosePod& R = a.pose[f];
  const uint8_t* __restrict__ src = P.src + (size_t)f * P.src_frame_bytes;
  uint8_t* __restrict__ d = P.dst + (size_t)f * P.dst_frame_bytes + (size_t)i * P.dstride + x0;

  const int n = min(4, dw - x0);
  uint32_t word = 0, written = 0;
  // not unrolled: one copy of the projection's code per instantiation; the bytes are packed by shifts (no indexed
  // register array, no scratch)
#pragma unroll 1
  for (int c = 0; c < n; c++) {
    const float2 mc = project_pixel(P.gen, R.rot, R.yaw_deg, R.pitch_deg, i, x0 + c);
    const LutEntry e = quantize_map_coord(P.gen.interp, mc.x, mc.y);
    const int v = sample<KS, TRANSPARENT>(src, P.sw, P.sh, P.sstride, a.wtab, e);
    if (v >= 0) {
      word |= (uint32_t)v << (8 * c);
      written |= 1u << c;
    }
  }
  if (!TRANSPARENT && n == 4 && a.dst_dword_ok) {
    *reinterpret_cast<uint32_t*>(d) = word;
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (written & (1u << c)) d[c] = (uint8_t)(word >> (8 * c));
  }
}

template <int KS>
hipError_t launch_posed_ks(const PosedArgs& a, int nframes, int total_tiles, bool transparent, hipStream_t stream) {
  const dim3 block(kPosedTileW / 4, kPosedTileH, 1);
  const dim3 grid(total_tiles, nframes, 1);
  if (transparent)
    hipLaunchKernelGGL((remap_posed_kernel<KS, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((remap_posed_kernel<KS, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_remap_posed(const PosedArgs& a, int nframes, int total_tiles, int interp, bool transparent,
                              hipStream_t stream) {
  if (nframes <= 0 || nframes > kPosedChunk || total_tiles <= 0 || a.nplanes <= 0 || a.nplanes > kPosedMaxPlanes)
    return hipErrorInvalidValue;
  switch (interp) {
    case NEAREST: return launch_posed_ks<1>(a, nframes, total_tiles, transparent, stream);
    case LINEAR: return launch_posed_ks<2>(a, nframes, total_tiles, transparent, stream);
    case CUBIC: return launch_posed_ks<4>(a, nframes, total_tiles, transparent, stream);
    case LANCZOS4: return launch_posed_ks<8>(a, nframes, total_tiles, transparent, stream);
    default: return hipErrorInvalidValue;
  }
}

const char* remap_posed_kernel_name(int interp) {
  switch (interp) {
    case NEAREST: return "remap_posed_kernel<1>";
    case LINEAR: return "remap_posed_kernel<2>";
    case CUBIC: return "remap_posed_kernel<4>";
    default: return "remap_posed_kernel<8>";
  }
}

}  // namespace t360
