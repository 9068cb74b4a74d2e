// image.hip — what the reference's YOLO sample does to an image before the
// forward pass, on the device: TImageData.resize (ntypes.pas:837-883) and
// letterBox / letterBoxEx (899-947: resize, fill 0.5, Embed) from decoded
// bytes or a planar float image to the network's input planes, in one launch
// for the whole batch.
//
// The reference resizes in two passes through a `part` image (the source rows
// at the target width).  Here a thread owns one destination pixel and forms
// the one or two `part` values it needs itself; each is the same rounded
// single `part` would have held, so the result has the reference's bits:
//
//   P(y)  = src(w-1, y)                                    x = aW-1 or w = 1
//         = (1-dx)*src(ix, y) + dx*src(ix+1, y)            sx = x*w_scale, ix = trunc(sx)
//   val   = (1-dy)*P(iy)                                   sy = r*h_scale, iy = trunc(sy)
//   val  += dy*P(iy+1)                                     unless r = aH-1 or h = 1
//
// all in single, every product and sum rounded (no FMA: the intrinsics below
// are never contracted).  The last row is NOT special-cased the way the last
// column is: where single(aH-1)*h_scale rounds below h-1 it is
// (1-dy)*P(h-2) with dy just below 1, a near-black row, as in the reference.
// For x < aW-1 the exact x*(w-1)/(aW-1) lies at least (w-1)/(aW-1) below w-1,
// far more than the two roundings move it, so ix+1 <= w-1 there (and iy+1 <=
// h-1 for r < aH-1); the clamps below never bind and only keep a read inside
// the image whatever the arithmetic gives.
//
// Threads run x fastest, 64 x 4 a block, so the planar stores coalesce; the
// channel loop is inside the thread, so the four source pixels of an
// interleaved image are addressed once.  A byte becomes a float through a
// 256-entry table (the host computes it, so the conversion is exact by
// construction), staged in LDS.  The per-image geometry and the table arrive
// as kernel arguments: host arrays are thereby copied before the call
// returns, with no staging buffer and no synchronisation.
#include "tns_internal.hpp"

namespace tns {
namespace {

constexpr int kImgBlockX = 64, kImgBlockY = 4;

struct ImageBatch {
  ImageGeom g[kImagePerLaunch];
};
struct ByteTable {
  float v[256];
};

template <bool BYTES>
__device__ __forceinline__ float img_src(const void* __restrict__ src, const ImageGeom& g, int ps,
                                         const float* tab, int x, int y, int k) {
  if (BYTES) {
    const uint8_t* p = static_cast<const uint8_t*>(src);
    return tab[p[g.off + (int64_t)y * g.rs + (int64_t)x * ps + k]];
  }
  const float* p = static_cast<const float*>(src);
  return p[g.off + ((int64_t)k * g.h + y) * g.rs + x];
}

template <bool BYTES>
__global__ __launch_bounds__(kImgBlockX* kImgBlockY) void image_to_input_kernel(
    ImageBatch B, ByteTable T, const void* __restrict__ src, int channels, int ps, int netW,
    int netH, float* __restrict__ dst) {
  __shared__ float tab[256];
  if (BYTES) {
    const int t = threadIdx.y * kImgBlockX + threadIdx.x;
    tab[t] = T.v[t];
    __syncthreads();
  }
  const int x = blockIdx.x * kImgBlockX + threadIdx.x;
  const int r = blockIdx.y * kImgBlockY + threadIdx.y;
  if (x >= netW || r >= netH) return;
  const ImageGeom& g = B.g[blockIdx.z];
  const int64_t plane = (int64_t)netH * netW;
  float* out = dst + (int64_t)blockIdx.z * channels * plane + (int64_t)r * netW + x;
  const int xe = x - g.dx, re = r - g.dy;
  if (xe < 0 || xe >= g.nw || re < 0 || re >= g.nh) {  // letterBox's fill(0.5)
    for (int k = 0; k < channels; ++k) out[k * plane] = 0.5f;
    return;
  }
  const bool lastCol = xe == g.nw - 1 || g.w == 1;
  const bool lastRow = re == g.nh - 1 || g.h == 1;
  int ix = g.w - 1;
  float dx = 0.f;
  if (!lastCol) {
    const float sx = __fmul_rn((float)xe, g.ws);
    ix = (int)sx;
    dx = __fsub_rn(sx, (float)ix);
    ix = min(ix, g.w - 1);
  }
  const int ix1 = min(ix + 1, g.w - 1);
  const float sy = __fmul_rn((float)re, g.hs);
  int iy = (int)sy;
  const float dy = __fsub_rn(sy, (float)iy);
  iy = min(iy, g.h - 1);
  const int iy1 = min(iy + 1, g.h - 1);
  const float cx = __fsub_rn(1.f, dx), cy = __fsub_rn(1.f, dy);
  for (int k = 0; k < channels; ++k) {
    float p0, p1 = 0.f;
    if (lastCol) {
      p0 = img_src<BYTES>(src, g, ps, tab, ix, iy, k);
      if (!lastRow) p1 = img_src<BYTES>(src, g, ps, tab, ix, iy1, k);
    } else {
      p0 = __fadd_rn(__fmul_rn(cx, img_src<BYTES>(src, g, ps, tab, ix, iy, k)),
                     __fmul_rn(dx, img_src<BYTES>(src, g, ps, tab, ix1, iy, k)));
      if (!lastRow)
        p1 = __fadd_rn(__fmul_rn(cx, img_src<BYTES>(src, g, ps, tab, ix, iy1, k)),
                       __fmul_rn(dx, img_src<BYTES>(src, g, ps, tab, ix1, iy1, k)));
    }
    float val = __fmul_rn(cy, p0);
    if (!lastRow) val = __fadd_rn(val, __fmul_rn(dy, p1));
    out[k * plane] = val;
  }
}

}  // namespace

hipError_t launch_image_to_input(bool bytes, const ImageGeom* geom, int64_t count, const void* src,
                                 int channels, int pixelStride, const float* table, int netW,
                                 int netH, float* dst, hipStream_t s) {
  ByteTable T{};
  if (bytes)
    for (int i = 0; i < 256; ++i) T.v[i] = table[i];
  const dim3 block(kImgBlockX, kImgBlockY);
  const int64_t perImage = (int64_t)channels * netH * netW;
  for (int64_t at = 0; at < count; at += kImagePerLaunch) {
    const int n = (int)std::min<int64_t>(count - at, kImagePerLaunch);
    ImageBatch B{};
    for (int i = 0; i < n; ++i) B.g[i] = geom[at + i];
    const dim3 grid((netW + kImgBlockX - 1) / kImgBlockX, (netH + kImgBlockY - 1) / kImgBlockY, n);
    if (bytes)
      hipLaunchKernelGGL(image_to_input_kernel<true>, grid, block, 0, s, B, T, src, channels,
                         pixelStride, netW, netH, dst + at * perImage);
    else
      hipLaunchKernelGGL(image_to_input_kernel<false>, grid, block, 0, s, B, T, src, channels,
                         pixelStride, netW, netH, dst + at * perImage);
  }
  return hipGetLastError();
}

}  // namespace tns
