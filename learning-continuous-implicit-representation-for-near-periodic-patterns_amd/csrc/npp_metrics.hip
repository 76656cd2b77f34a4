// npp_metrics.hip -- the quality figures of a fitted or rendered image against a ground truth (metrics.py): the SSIM index map of
// Wang et al. (11 x 11 Gaussian window, sigma 1.5, K1 = 0.01, K2 = 0.03, data range 1, population variances) and the masked sums
// PSNR / MAE / mean SSIM of a region are made of.  Both images are read as they lie, (H, W, 3) fp32.  Everything is accumulated in
// float64: a variance is E[x^2] - mu^2, a difference of nearly equal numbers that is then divided by something as small as
// C2 = 9e-4, and 22 taps x 5 moments per pixel and channel cost nothing that matters in a once-per-image step.  Nothing is kept in
// device memory between launches and there are no atomics: every entry is bit-reproducible.
#include <math.h>
#include "npp_common.h"

namespace npp {

constexpr int kSsimWin = 11;                            // window taps per axis
constexpr int kSsimHalo = kSsimWin - 1;                 // the map is (H - 10) x (W - 10): pixels whose whole window lies inside
constexpr int kSsimTX = 32, kSsimTY = 16;               // map pixels per workgroup: 32 wide (one half-wave per row), 16 high
constexpr int kSsimSX = kSsimTX + kSsimHalo;            // 42 x 26 image pixels feed a tile
constexpr int kSsimSY = kSsimTY + kSsimHalo;
constexpr int kSsimRow = kSsimSX * 3;                   // a staged row as it lies in memory: 126 interleaved floats
constexpr double kSsimC1 = 0.01 * 0.01, kSsimC2 = 0.03 * 0.03;   // (K1 L)^2, (K2 L)^2 with L = 1
static_assert(kSsimTX == 32 && kSsimTX * kSsimTY == 2 * 256, "ssim_map_kernel: two map pixels per thread, a row per half-wave");

struct SsimWindow { double g[kSsimWin]; };              // the 1-D window, normalised to sum 1 (the 2-D one is its outer product)

// One tile of the map per workgroup.  The tile's pixels plus the 10-pixel halo of BOTH images go into LDS once (clamped at the far
// image border: the last tiles compute on repeated pixels what they do not store).  Per channel: a horizontal pass leaves the five
// row moments sum_k g[k] {x, y, x^2, y^2, x y} of the 26 x 32 (row, column) pairs in LDS, a vertical pass finishes them and forms the
// index; the three channels' indices are averaged in registers.  LDS reads: a half-wave walks one staged row at a stride of three
// floats (3 is odd: 32 distinct banks) in the horizontal pass and 32 consecutive doubles in the vertical one -- conflict-free.
__global__ __launch_bounds__(256) void ssim_map_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W, SsimWindow win,
                                                       double* __restrict__ out) {
  __shared__ float sa[kSsimSY][kSsimRow], sb[kSsimSY][kSsimRow];
  __shared__ double hm[5][kSsimSY][kSsimTX];
  const int x0 = blockIdx.x * kSsimTX, y0 = blockIdx.y * kSsimTY;
  for (int e = threadIdx.x; e < kSsimSY * kSsimRow; e += 256) {
    const int r = e / kSsimRow, q = e - r * kSsimRow, c = q / 3, ch = q - 3 * c;
    const int64_t src = ((int64_t)min(y0 + r, H - 1) * W + min(x0 + c, W - 1)) * 3 + ch;
    sa[r][q] = a[src];
    sb[r][q] = b[src];
  }
  __syncthreads();
  const int Ho = H - kSsimHalo, Wo = W - kSsimHalo;
  const int x = threadIdx.x & 31, yq = threadIdx.x >> 5;
  double mean[2] = {0.0, 0.0};
#pragma unroll 1
  for (int ch = 0; ch < 3; ++ch) {
    for (int r = yq; r < kSsimSY; r += 8) {
      double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
      for (int k = 0; k < kSsimWin; ++k) {
        const double w = win.g[k], p = (double)sa[r][(x + k) * 3 + ch], q = (double)sb[r][(x + k) * 3 + ch];
        mx += w * p;
        my += w * q;
        exx += w * (p * p);
        eyy += w * (q * q);
        exy += w * (p * q);
      }
      hm[0][r][x] = mx;
      hm[1][r][x] = my;
      hm[2][r][x] = exx;
      hm[3][r][x] = eyy;
      hm[4][r][x] = exy;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int y = yq + 8 * j;
      double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
      for (int k = 0; k < kSsimWin; ++k) {
        const double w = win.g[k];
        mx += w * hm[0][y + k][x];
        my += w * hm[1][y + k][x];
        exx += w * hm[2][y + k][x];
        eyy += w * hm[3][y + k][x];
        exy += w * hm[4][y + k][x];
      }
      const double vx = exx - mx * mx, vy = eyy - my * my, cxy = exy - mx * my;
      // (identical images: both factors of the numerator equal the denominator's bit for bit, the index is exactly 1)
      const double num = (2.0 * mx * my + kSsimC1) * (2.0 * cxy + kSsimC2);
      const double den = (mx * mx + my * my + kSsimC1) * (vx + vy + kSsimC2);
      mean[j] += num / den;
    }
    __syncthreads();                                                  // hm is rewritten for the next channel
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = y0 + yq + 8 * j, ox = x0 + x;
    if (oy < Ho && ox < Wo) out[(int64_t)oy * Wo + ox] = mean[j] / 3.0;
  }
}

// ---- masked sums of one region -----------------------------------------------------------------------------------------------------
// Block-stride over the pixels with a block count that depends on the shape only; per block five float64 sums, reduced in a fixed
// order (lane butterfly, then the four waves in turn) and written to part[block][5]: 0 the weights, 1 the weighted squared error and
// 2 the weighted absolute error over the three channels, 3 the weights of the pixels the SSIM map covers (rows and columns 5 .. n - 6)
// and 4 the weighted map there (3, 4 stay zero without a map).  The host adds the blocks in order.
constexpr int kRegionSums = 5;
constexpr int kRegionMaxBlocks = 256;

__global__ __launch_bounds__(256) void region_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ weight,
                                                          const double* __restrict__ ssim, int H, int W, double* __restrict__ part) {
  __shared__ double red[4][kRegionSums];
  const int64_t n = (int64_t)H * W;
  const int Wo = W - kSsimHalo, r = kSsimHalo / 2;
  double s[kRegionSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const double w = (double)weight[p];
    const double d0 = (double)a[p * 3] - (double)b[p * 3], d1 = (double)a[p * 3 + 1] - (double)b[p * 3 + 1],
                 d2 = (double)a[p * 3 + 2] - (double)b[p * 3 + 2];
    s[0] += w;
    s[1] += w * (d0 * d0 + d1 * d1 + d2 * d2);
    s[2] += w * (fabs(d0) + fabs(d1) + fabs(d2));
    if (ssim) {
      const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
      if (y >= r && y < H - r && x >= r && x < W - r) {
        s[3] += w;
        s[4] += w * ssim[(int64_t)(y - r) * Wo + (x - r)];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kRegionSums; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kRegionSums) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * kRegionSums + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

static bool metrics_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 36); }
static int region_blocks(int H, int W) {
  const int64_t b = ((int64_t)H * W + 255) / 256;
  return (int)(b > kRegionMaxBlocks ? kRegionMaxBlocks : b);
}

}  // namespace npp

using namespace npp;

extern "C" int npp_ssim_map(const float* d_a_hw3, const float* d_b_hw3, int H, int W, double* d_map, void* stream) {
  if (H < kSsimWin || W < kSsimWin) {
    set_error("npp_ssim_map: H=%d W=%d: both must be at least %d (one whole %d x %d window)", H, W, kSsimWin, kSsimWin, kSsimWin);
    return NPP_ERR_ARG;
  }
  if (!d_a_hw3 || !d_b_hw3 || !d_map || !metrics_shape_ok(H, W) || (H - kSsimHalo + kSsimTY - 1) / kSsimTY > 65535) {
    set_error("npp_ssim_map: bad argument (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  SsimWindow win;
  double sum = 0.0;
  for (int k = 0; k < kSsimWin; ++k) {
    const double d = (double)(k - kSsimWin / 2);
    win.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += win.g[k];
  }
  for (int k = 0; k < kSsimWin; ++k) win.g[k] /= sum;
  const dim3 grid((unsigned)((W - kSsimHalo + kSsimTX - 1) / kSsimTX), (unsigned)((H - kSsimHalo + kSsimTY - 1) / kSsimTY));
  hipLaunchKernelGGL(ssim_map_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_a_hw3, d_b_hw3, H, W, win, d_map);
  return check_launch("npp_ssim_map");
}

extern "C" int npp_region_sums_blocks(int H, int W) {
  if (!metrics_shape_ok(H, W)) {
    set_error("npp_region_sums_blocks: bad argument (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  return region_blocks(H, W);
}

extern "C" int npp_region_sums(const float* d_a_hw3, const float* d_b_hw3, const float* d_weight_hw, const double* d_ssim_map, int H, int W,
                               double* d_part, void* stream) {
  if (!d_a_hw3 || !d_b_hw3 || !d_weight_hw || !d_part || !metrics_shape_ok(H, W) || (d_ssim_map && (H < kSsimWin || W < kSsimWin))) {
    set_error("npp_region_sums: bad argument (H=%d W=%d; with a map both at least %d)", H, W, kSsimWin);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(region_sums_kernel, dim3((unsigned)region_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, d_a_hw3, d_b_hw3, d_weight_hw,
                     d_ssim_map, H, W, d_part);
  return check_launch("npp_region_sums");
}
