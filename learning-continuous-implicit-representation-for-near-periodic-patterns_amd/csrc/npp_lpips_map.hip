// npp_lpips_map.hip -- LPIPS of whole images as a quality figure (metrics.LPIPSMetric): the head of externel_lib/lpips/lpips.py:92-133
// (use_robust = False) on the fp32 features of two images, the bilinear composition of the taps' maps into the (H, W) distance map
// (spatial = True) and the masked sums a region's mean is made of.  The fp32 features are exact inputs; everything from there on is
// float64 and summed in a fixed order -- the trunk is the only fp32 stage of the metric.  Nothing is kept in device memory between
// launches and there are no atomics: every entry is bit-reproducible.
#include <math.h>
#include "npp_common.h"

namespace npp {

constexpr double kLpipsEps = 1e-10;                     // lpips/__init__.py:42-44 normalize_tensor
constexpr int kTapSplitPos = 4;                         // split form: positions per wave ...
constexpr int kTapSplitSlices = 64 / kTapSplitPos;      // ... and channel slices per position (lane = slice * 4 + position)
constexpr int64_t kTapSplitBelow = 16384;               // NCHW taps with fewer positions take the split form (launcher)
constexpr int64_t kTapMaxPos = (int64_t)1 << 36;

// The two passes of one position, written once: `load(c, a, b)` gives channel c of both images; channels c0, c0 + step, ... in that
// order.  Pass 1 the squared norms, pass 2 the lin-weighted squared difference of the unit-normalised features (the two-pass form:
// the expanded one-pass form |a|^2 / na^2 - 2 a.b / (na nb) + |b|^2 / nb^2 cancels for similar images).
template <typename Load>
__device__ __forceinline__ void tap_norms(const Load& load, int c0, int step, int C, double& sa, double& sb) {
  sa = 0.0;
  sb = 0.0;
#pragma unroll 4
  for (int c = c0; c < C; c += step) {
    float a, b;
    load(c, a, b);
    sa += (double)a * (double)a;
    sb += (double)b * (double)b;
  }
}
template <typename Load>
__device__ __forceinline__ double tap_diff(const Load& load, int c0, int step, int C, const float* __restrict__ lin, double na, double nb) {
  double s = 0.0;
#pragma unroll 4
  for (int c = c0; c < C; c += step) {
    float a, b;
    load(c, a, b);
    const double e = (double)a / na - (double)b / nb;
    s += (double)lin[c] * (e * e);
  }
  return s;
}

// NCHW, one lane per position, lanes along w: channel c of 64 neighbouring positions is one coalesced 256-byte load.  Every lane
// walks all C channels twice (the second pass finds a large tap in the L2 / Infinity Cache or streams it again); bound by those
// reads and by the two float64 divisions per channel.
__global__ __launch_bounds__(256) void lpips_tap_nchw_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int C, int64_t P,
                                                             const float* __restrict__ lin, double* __restrict__ d) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  auto load = [&](int c, float& a, float& b) {
    a = f0[(int64_t)c * P + p];
    b = f1[(int64_t)c * P + p];
  };
  double sa, sb;
  tap_norms(load, 0, 1, C, sa, sb);
  d[p] = tap_diff(load, 0, 1, C, lin, sqrt(sa) + kLpipsEps, sqrt(sb) + kLpipsEps);
}

// NCHW, the deep taps (few positions, many channels): a wave takes 4 neighbouring positions and splits the channels into 16
// slices, lane = slice * 4 + position, slice s walks channels s, s + 16, ...; the slices are added by a butterfly over the lane
// bits 2..5 (a fixed tree; every lane ends with the same bits).  16 x the waves of the form above at 1 / 16 of the trip count:
// bound by launch and load latency, not by bandwidth (such a tap is a few MB at most and its loads are 16-byte segments).
__global__ __launch_bounds__(256) void lpips_tap_nchw_split_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int C, int64_t P,
                                                                   const float* __restrict__ lin, double* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kTapSplitPos;
  if (p0 >= P) return;                                                // (wave-uniform: the shuffles below stay inside one wave)
  const int64_t pw = p0 + (lane & (kTapSplitPos - 1));
  const int64_t p = pw < P ? pw : P - 1;                             // surplus lanes of the last wave repeat the last position
  const int slice = lane >> 2;
  auto load = [&](int c, float& a, float& b) {
    a = f0[(int64_t)c * P + p];
    b = f1[(int64_t)c * P + p];
  };
  double sa, sb;
  tap_norms(load, slice, kTapSplitSlices, C, sa, sb);
#pragma unroll
  for (int off = kTapSplitPos; off < 64; off <<= 1) {
    sa += __shfl_xor(sa, off, 64);
    sb += __shfl_xor(sb, off, 64);
  }
  double s = tap_diff(load, slice, kTapSplitSlices, C, lin, sqrt(sa) + kLpipsEps, sqrt(sb) + kLpipsEps);
#pragma unroll
  for (int off = kTapSplitPos; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
  if (slice == 0 && pw < P) d[pw] = s;
}

// Position-major (h, w, C) features (segment.AlexFeatures.features_nhwc): one wave per position, lane l walks channels l, l + 64,
// ... of one contiguous row, butterfly over all six lane bits -- lpips_spatial_kernel's shape in float64.
__global__ __launch_bounds__(256) void lpips_tap_nhwc_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int C, int64_t P,
                                                             const float* __restrict__ lin, double* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;                                                 // (wave-uniform)
  const float* __restrict__ a0 = f0 + p * C;
  const float* __restrict__ b0 = f1 + p * C;
  auto load = [&](int c, float& a, float& b) {
    a = a0[c];
    b = b0[c];
  };
  double sa, sb;
  tap_norms(load, lane, 64, C, sa, sb);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sa += __shfl_xor(sa, off, 64);
    sb += __shfl_xor(sb, off, 64);
  }
  double s = tap_diff(load, lane, 64, C, lin, sqrt(sa) + kLpipsEps, sqrt(sb) + kLpipsEps);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) d[p] = s;
}

// ---- composition: D = sum_k upsample(d_k -> (H, W)) ------------------------------------------------------------------------------------
// F.interpolate(mode = 'bilinear', align_corners = False) of every tap's map, summed in tap order, one launch, one store per pixel:
// source index max(0, (o + 0.5) h / H - 0.5), the +1 neighbour clamped at the border (resize_bilinear_kernel of npp_segment.hip, in
// float64).  Bound by the H W stores; the taps' maps are read from the caches.
constexpr int kComposeMaxTaps = 8;
struct ComposeTaps {
  const double* map[kComposeMaxTaps];
  int h[kComposeMaxTaps], w[kComposeMaxTaps];
  int n;
};

__global__ __launch_bounds__(256) void lpips_compose_kernel(ComposeTaps T, int H, int W, double* __restrict__ out) {
  const int64_t total = (int64_t)H * W;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int oy = (int)(t / W), ox = (int)(t - (int64_t)oy * W);
    double sum = 0.0;
    for (int k = 0; k < T.n; ++k) {
      const int h = T.h[k], w = T.w[k];
      const double* __restrict__ s = T.map[k];
      const double sy = fmax((double)h / (double)H * ((double)oy + 0.5) - 0.5, 0.0);
      const double sx = fmax((double)w / (double)W * ((double)ox + 0.5) - 0.5, 0.0);
      const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
      const int yp = y0 < h - 1 ? 1 : 0, xp = x0 < w - 1 ? 1 : 0;
      const double ly = sy - (double)y0, lx = sx - (double)x0, hy = 1.0 - ly, hx = 1.0 - lx;
      const int64_t r0 = (int64_t)y0 * w, r1 = (int64_t)(y0 + yp) * w;
      sum += hy * (hx * s[r0 + x0] + lx * s[r0 + x0 + xp]) + ly * (hx * s[r1 + x0] + lx * s[r1 + x0 + xp]);
    }
    out[t] = sum;
  }
}

// ---- masked sums of a float64 map ----------------------------------------------------------------------------------------------------
// region_sums_kernel's scheme (npp_metrics.hip) for one map: block-stride over the pixels with a block count that depends on the
// shape only, per block (sum w, sum w map) reduced in a fixed order and written to part[block][2].  weight == nullptr: all ones.
constexpr int kMapRegionMaxBlocks = 256;

__global__ __launch_bounds__(256) void map_region_sums_kernel(const double* __restrict__ map, const float* __restrict__ weight, int64_t n,
                                                              double* __restrict__ part) {
  __shared__ double red[4][2];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const double w = weight ? (double)weight[p] : 1.0;
    s0 += w;
    s1 += w * map[p];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, 64);
    s1 += __shfl_xor(s1, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = s0;
    red[threadIdx.x >> 6][1] = s1;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * 2 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

static bool map_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= kTapMaxPos; }
static int map_region_blocks(int H, int W) {
  const int64_t b = ((int64_t)H * W + 255) / 256;
  return (int)(b > kMapRegionMaxBlocks ? kMapRegionMaxBlocks : b);
}

}  // namespace npp

using namespace npp;

extern "C" int npp_lpips_tap_map(const float* d_f0, const float* d_f1, int C, int h, int w, int layout, const float* d_lin, double* d_map,
                                 void* stream) {
  if (!d_f0 || !d_f1 || !d_lin || !d_map) {
    set_error("npp_lpips_tap_map: null pointer (C=%d h=%d w=%d)", C, h, w);
    return NPP_ERR_ARG;
  }
  if (C < 1) {
    set_error("npp_lpips_tap_map: C=%d: a tap has at least one channel", C);
    return NPP_ERR_ARG;
  }
  if (!map_shape_ok(h, w)) {
    set_error("npp_lpips_tap_map: empty or oversized map (h=%d w=%d)", h, w);
    return NPP_ERR_ARG;
  }
  if (layout < NPP_LPIPS_NCHW || layout > NPP_LPIPS_NCHW_SPLIT) {
    set_error("npp_lpips_tap_map: unknown layout code %d (0 NCHW, 1 NHWC, 2 NCHW one lane per position, 3 NCHW split channels)", layout);
    return NPP_ERR_ARG;
  }
  const int64_t P = (int64_t)h * w;
  if (layout == NPP_LPIPS_NCHW) layout = P < kTapSplitBelow ? NPP_LPIPS_NCHW_SPLIT : NPP_LPIPS_NCHW_LANE;
  hipStream_t st = (hipStream_t)stream;
  if (layout == NPP_LPIPS_NHWC)
    hipLaunchKernelGGL(lpips_tap_nhwc_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, d_f0, d_f1, C, P, d_lin, d_map);
  else if (layout == NPP_LPIPS_NCHW_LANE)
    hipLaunchKernelGGL(lpips_tap_nchw_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, d_f0, d_f1, C, P, d_lin, d_map);
  else
    hipLaunchKernelGGL(lpips_tap_nchw_split_kernel, dim3((unsigned)((P + 4 * kTapSplitPos - 1) / (4 * kTapSplitPos))), dim3(256), 0, st, d_f0,
                       d_f1, C, P, d_lin, d_map);
  return check_launch("npp_lpips_tap_map");
}

extern "C" int npp_lpips_compose(const double* const* d_maps, const int* hs, const int* ws, int n_taps, int H, int W, double* d_out,
                                 void* stream) {
  if (!d_maps || !hs || !ws || !d_out || n_taps < 1 || n_taps > kComposeMaxTaps) {
    set_error("npp_lpips_compose: bad argument (n_taps=%d, at most %d)", n_taps, kComposeMaxTaps);
    return NPP_ERR_ARG;
  }
  if (!map_shape_ok(H, W)) {
    set_error("npp_lpips_compose: empty or oversized map (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  ComposeTaps T{};
  T.n = n_taps;
  for (int k = 0; k < n_taps; ++k) {
    if (!d_maps[k] || !map_shape_ok(hs[k], ws[k])) {
      set_error("npp_lpips_compose: tap %d: null pointer or empty map (h=%d w=%d)", k, hs[k], ws[k]);
      return NPP_ERR_ARG;
    }
    T.map[k] = d_maps[k];
    T.h[k] = hs[k];
    T.w[k] = ws[k];
  }
  const int64_t blocks = ((int64_t)H * W + 255) / 256;
  hipLaunchKernelGGL(lpips_compose_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, (hipStream_t)stream, T, H, W, d_out);
  return check_launch("npp_lpips_compose");
}

extern "C" int npp_map_region_sums_blocks(int H, int W) {
  if (!map_shape_ok(H, W)) {
    set_error("npp_map_region_sums_blocks: empty or oversized map (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  return map_region_blocks(H, W);
}

extern "C" int npp_map_region_sums(const double* d_map, const float* d_weight_hw, int H, int W, double* d_part, void* stream) {
  if (!d_map || !d_part) {
    set_error("npp_map_region_sums: null pointer (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  if (!map_shape_ok(H, W)) {
    set_error("npp_map_region_sums: empty or oversized map (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(map_region_sums_kernel, dim3((unsigned)map_region_blocks(H, W)), dim3(256), 0, (hipStream_t)stream, d_map, d_weight_hw,
                     (int64_t)H * W, d_part);
  return check_launch("npp_map_region_sums");
}
