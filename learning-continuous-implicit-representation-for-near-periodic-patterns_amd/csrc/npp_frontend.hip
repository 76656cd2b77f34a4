// npp_frontend.hip -- the per-pixel image work in front of the periodicity search (completion task; frontend.py):
// the OpenCV steps of NPP_proposal/feature_searching.py:14-75 as cvlite.py restates them (8-bit resizes, normalisation to uint8,
// Gaussian 3 x 3, Canny with 8-connected hysteresis, the masked edge count) and the pseudo mask of utils/miscs.py:53-96 (exact
// squared Euclidean distance transform, greedy far-point selection).  The image and mask kernels are integer arithmetic; the
// resize index rules and the normalisation are float64 in the host definition's operation order with no contraction (the file is
// built with -ffp-contract=off and the operations are spelt __d*_rn).  No float atomics, no state in device memory between
// calls: every result is a pure function of its input, whatever the launch schedule.  Batched entries take (C, h, w) arrays and
// put the channel in a grid dimension: 66 channels are one launch sequence.
#include "npp_common.h"

namespace npp {

constexpr int kFeTile = 32;                 // Canny / hysteresis tile side (256 threads, 4 pixels each)
constexpr int kFeMaxDim = 32767;            // H, W of the distance transform: 2 * 32766^2 < 2^31
constexpr int kFeFarBlocks = 256;           // stage-1 blocks of the far-point argmax (== NPP_FAR_POINTS_SCRATCH_BYTES / 8)
constexpr int kFeFarMaxTopk = 16;
constexpr int kFeEdtChunk = 1024;           // columns of a row staged in LDS at a time
constexpr uint32_t kFeEdtInf = 0x80000000u; // "no zero pixel in this column": above every true squared distance, and
                                            // dx^2 + it still fits 32 bits

static bool fe_shape_ok(int C, int h, int w) { return C >= 1 && C <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31); }
static unsigned fe_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
__device__ __forceinline__ int fe_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- cvlite.resize_nearest: source index = min(trunc(dst * (src / dst_size)), src - 1), the product in float64 -------------------
__global__ __launch_bounds__(256) void fe_resize_nearest_kernel(const uint8_t* __restrict__ in, int H, int W, int h, int w, double sy,
                                                                double sx, uint8_t* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const int iy = min((int)__dmul_rn((double)y, sy), H - 1), ix = min((int)__dmul_rn((double)x, sx), W - 1);
  out[p] = in[(int64_t)iy * W + ix];
}

// ---- cvlite._linear_taps: OpenCV's bilinear tap of one axis (source indices, two 11-bit coefficients) -----------------------------
__device__ __forceinline__ void fe_linear_tap(int i, int src, double scale, int& s0, int& s1, int& c0, int& c1) {
  double f = __dsub_rn(__dmul_rn(__dadd_rn((double)i, 0.5), scale), 0.5);
  const double fl = floor(f);
  int s = (int)fl;
  f = __dsub_rn(f, fl);
  if (s < 0) { s = 0; f = 0.0; }
  if (s >= src - 1) { s = src - 1; f = 0.0; }
  c1 = (int)rint(__dmul_rn(f, 2048.0));
  c0 = (int)rint(__dmul_rn(__dsub_rn(1.0, f), 2048.0));
  s0 = s;
  s1 = min(s + 1, src - 1);
}

// cvlite.resize_linear_u8: horizontal pass into 11-bit fixed point, vertical pass (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2
__global__ __launch_bounds__(256) void fe_resize_linear_kernel(const uint8_t* __restrict__ in, int H, int W, int h, int w, double sy,
                                                               double sx, uint8_t* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  int y0, y1, b0, b1, x0, x1, a0, a1;
  fe_linear_tap(y, H, sy, y0, y1, b0, b1);
  fe_linear_tap(x, W, sx, x0, x1, a0, a1);
  const uint8_t* r0 = in + (int64_t)y0 * W;
  const uint8_t* r1 = in + (int64_t)y1 * W;
  const int S0 = (int)r0[x0] * a0 + (int)r0[x1] * a1, S1 = (int)r1[x0] * a0 + (int)r1[x1] * a1;
  const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
  out[p] = (uint8_t)fe_clamp(v, 0, 255);
}

// ---- cvlite.normalize_to_uint8 over the (h, w) axes: uint8((a - mn) / rng * 255) in float64, one workgroup per channel -----------
__global__ __launch_bounds__(256) void fe_normalize_kernel(const float* __restrict__ in, int64_t n, uint8_t* __restrict__ out) {
  __shared__ double s_mn[256], s_mx[256];
  const float* a = in + (int64_t)blockIdx.x * n;
  uint8_t* o = out + (int64_t)blockIdx.x * n;
  double mn = (double)a[0], mx = mn;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double v = (double)a[i];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  s_mn[threadIdx.x] = mn;
  s_mx[threadIdx.x] = mx;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      s_mn[threadIdx.x] = s_mn[threadIdx.x + k] < s_mn[threadIdx.x] ? s_mn[threadIdx.x + k] : s_mn[threadIdx.x];
      s_mx[threadIdx.x] = s_mx[threadIdx.x + k] > s_mx[threadIdx.x] ? s_mx[threadIdx.x + k] : s_mx[threadIdx.x];
    }
    __syncthreads();
  }
  mn = s_mn[0];
  mx = s_mx[0];
  const double rng = mx > mn ? __dsub_rn(mx, mn) : 1.0;
  for (int64_t i = threadIdx.x; i < n; i += 256)
    o[i] = (uint8_t)(int)__dmul_rn(__ddiv_rn(__dsub_rn((double)a[i], mn), rng), 255.0);
}

// ---- cvlite.gaussian_blur3_u8: [1 2 1]^2, BORDER_REFLECT_101, (v + 8) >> 4 -------------------------------------------------------
__device__ __forceinline__ int fe_reflect101(int i, int n) {
  const int r = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return fe_clamp(r, 0, n - 1);                                          // (an axis of length 1 sees itself)
}

__global__ __launch_bounds__(256) void fe_blur3_kernel(const uint8_t* __restrict__ in, int h, int w, uint8_t* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h * w) return;
  const int64_t base = (int64_t)blockIdx.y * h * w;
  const int y = p / w, x = p - y * w;
  const int ys[3] = {fe_reflect101(y - 1, h), y, fe_reflect101(y + 1, h)};
  const int xl = fe_reflect101(x - 1, w), xr = fe_reflect101(x + 1, w);
  int v = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint8_t* r = in + base + (int64_t)ys[k] * w;
    v += (k == 1 ? 2 : 1) * ((int)r[xl] + 2 * (int)r[x] + (int)r[xr]);
  }
  out[base + p] = (uint8_t)((v + 8) >> 4);
}

// ---- cvlite.canny_u8 up to the hysteresis: one launch writes 0 / 1 (weak) / 2 (strong) -------------------------------------------
// A 32 x 32 tile per workgroup: the 36 x 36 image bytes around it (replicated border) -> Sobel dx, dy of the 34 x 34 positions
// around it (zero outside the map: the magnitude there is zero) -> non-maximum suppression with the integer tangent test.
__global__ __launch_bounds__(256) void fe_canny_mark_kernel(const uint8_t* __restrict__ img, int h, int w, int low, int high,
                                                            uint8_t* __restrict__ map) {
  constexpr int T = kFeTile;
  __shared__ uint8_t s_img[T + 4][T + 4];
  __shared__ int16_t s_dx[T + 2][T + 2], s_dy[T + 2][T + 2];
  const int64_t base = (int64_t)blockIdx.z * h * w;
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  for (int e = threadIdx.x; e < (T + 4) * (T + 4); e += 256) {
    const int r = e / (T + 4), c = e - r * (T + 4);
    s_img[r][c] = img[base + (int64_t)fe_clamp(y0 - 2 + r, 0, h - 1) * w + fe_clamp(x0 - 2 + c, 0, w - 1)];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (T + 2) * (T + 2); e += 256) {
    const int r = e / (T + 2), c = e - r * (T + 2);
    const int py = y0 - 1 + r, px = x0 - 1 + c;
    int dx = 0, dy = 0;
    if (py >= 0 && py < h && px >= 0 && px < w) {
      const int a00 = s_img[r][c], a01 = s_img[r][c + 1], a02 = s_img[r][c + 2];
      const int a10 = s_img[r + 1][c], a12 = s_img[r + 1][c + 2];
      const int a20 = s_img[r + 2][c], a21 = s_img[r + 2][c + 1], a22 = s_img[r + 2][c + 2];
      dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
      dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
    }
    s_dx[r][c] = (int16_t)dx;
    s_dy[r][c] = (int16_t)dy;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < T * T; e += 256) {
    const int ty = e / T, tx = e - ty * T;
    const int py = y0 + ty, px = x0 + tx;
    if (py >= h || px >= w) continue;
    const int r = ty + 1, c = tx + 1;
    auto mag = [&](int rr, int cc) { return abs((int)s_dx[rr][cc]) + abs((int)s_dy[rr][cc]); };
    const int dx = s_dx[r][c], dy = s_dy[r][c];
    const int m = abs(dx) + abs(dy);
    const int ax = abs(dx), ay = abs(dy) << 15;
    const int tg22 = ax * 13573, tg67 = tg22 + (ax << 16);
    bool keep;
    if (ay < tg22) keep = m > mag(r, c - 1) && m >= mag(r, c + 1);
    else if (ay > tg67) keep = m > mag(r - 1, c) && m >= mag(r + 1, c);
    else if ((dx ^ dy) < 0) keep = m > mag(r - 1, c + 1) && m > mag(r + 1, c - 1);
    else keep = m > mag(r - 1, c - 1) && m > mag(r + 1, c + 1);
    const bool weak = keep && m > low;
    map[base + (int64_t)py * w + px] = weak ? (m > high ? 2 : 1) : 0;
  }
}

// One round of the hysteresis: every tile takes its 34 x 34 surroundings into LDS (zero outside the map), spreads the strong mark
// to 8-connected weak pixels until the tile is stable, writes the newly marked pixels back and raises *flag when there were any.
// A pixel only ever goes 1 -> 2, so a tile that reads a neighbour's pixel before that neighbour's write of the same round merely
// sees it one round later; the caller repeats rounds until one raises no flag, and that fixed point is unique.
__global__ __launch_bounds__(256) void fe_hysteresis_kernel(uint8_t* __restrict__ map, int h, int w, int32_t* __restrict__ flag) {
  constexpr int T = kFeTile;
  __shared__ volatile uint8_t s[T + 2][T + 2];
  uint8_t* m = map + (int64_t)blockIdx.z * h * w;
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  for (int e = threadIdx.x; e < (T + 2) * (T + 2); e += 256) {
    const int r = e / (T + 2), c = e - r * (T + 2);
    const int py = y0 - 1 + r, px = x0 - 1 + c;
    s[r][c] = (py >= 0 && py < h && px >= 0 && px < w) ? m[(int64_t)py * w + px] : (uint8_t)0;
  }
  __syncthreads();
  int mine = 0;                                                          // bit k: pixel k of this thread was marked here
  int changed;
  do {
    changed = 0;
#pragma unroll
    for (int k = 0; k < (T * T) / 256; ++k) {
      const int e = threadIdx.x + k * 256;
      const int r = e / T + 1, c = e % T + 1;
      if (s[r][c] != 1) continue;
      const bool hit = s[r - 1][c - 1] == 2 || s[r - 1][c] == 2 || s[r - 1][c + 1] == 2 || s[r][c - 1] == 2 || s[r][c + 1] == 2 ||
                       s[r + 1][c - 1] == 2 || s[r + 1][c] == 2 || s[r + 1][c + 1] == 2;
      if (hit) {
        s[r][c] = 2;
        mine |= 1 << k;
        changed = 1;
      }
    }
  } while (__syncthreads_or(changed));
#pragma unroll
  for (int k = 0; k < (T * T) / 256; ++k) {
    if (!(mine & (1 << k))) continue;
    const int e = threadIdx.x + k * 256;
    m[(int64_t)(y0 + e / T) * w + (x0 + e % T)] = 2;                      // (a marked pixel was weak, so it lies inside the map)
  }
  if (__syncthreads_or(mine) && threadIdx.x == 0) atomicOr(flag, 1);
}

// strong -> 255, everything else -> 0 (cvlite.canny_u8's output)
__global__ __launch_bounds__(256) void fe_canny_finish_kernel(const uint8_t* __restrict__ map, int64_t n, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < n) out[p] = map[p] == 2 ? 255 : 0;
}

// proposal.act2edge: sum over the channels of (Canny / 255) inside the eroded mask
__global__ __launch_bounds__(256) void fe_edge_count_kernel(const uint8_t* __restrict__ map, int C, int64_t n, const uint8_t* __restrict__ eroded,
                                                            float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int cnt = 0;
  if (eroded[p])
    for (int c = 0; c < C; ++c) cnt += map[(int64_t)c * n + p] == 2 ? 1 : 0;
  out[p] = (float)cnt;
}

// ---- exact squared Euclidean distance transform: squared distance to the nearest zero pixel ----------------------------------------
// Pass 1, one thread per column: g(y, x) = distance along the column to its nearest zero (two sweeps), stored squared, or kFeEdtInf.
__global__ __launch_bounds__(256) void fe_edt_col_kernel(const uint8_t* __restrict__ mask, int H, int W, uint32_t* __restrict__ g2) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  constexpr uint32_t kNone = 0xffffffffu;
  uint32_t d = kNone;
  for (int y = 0; y < H; ++y) {
    const int64_t p = (int64_t)y * W + x;
    d = mask[p] == 0 ? 0u : (d == kNone ? kNone : d + 1u);
    g2[p] = d;
  }
  d = kNone;
  for (int y = H - 1; y >= 0; --y) {
    const int64_t p = (int64_t)y * W + x;
    d = mask[p] == 0 ? 0u : (d == kNone ? kNone : d + 1u);
    const uint32_t up = g2[p], best = d < up ? d : up;
    g2[p] = best == kNone ? kFeEdtInf : best * best;
  }
}

// Pass 2, one thread per pixel: min over the columns x' of (x - x')^2 + g(y, x')^2, the row staged in LDS a chunk at a time.
__global__ __launch_bounds__(256) void fe_edt_row_kernel(const uint32_t* __restrict__ g2, int W, int32_t* __restrict__ out) {
  __shared__ uint32_t s[kFeEdtChunk];
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const uint32_t* row = g2 + (int64_t)y * W;
  uint32_t best = 0xffffffffu;
  for (int c0 = 0; c0 < W; c0 += kFeEdtChunk) {
    __syncthreads();
    for (int j = threadIdx.x; j < kFeEdtChunk; j += 256) s[j] = c0 + j < W ? row[c0 + j] : kFeEdtInf;
    __syncthreads();
    const int nj = min(kFeEdtChunk, W - c0);
    int dx = x - c0;
    for (int j = 0; j < nj; ++j, --dx) {
      const uint32_t v = (uint32_t)(dx * dx) + s[j];
      best = v < best ? v : best;
    }
  }
  if (x < W) out[(int64_t)y * W + x] = (int32_t)best;
}

// ---- far-point selection: the greedy walk of search.find_mask_centroid as at most topk argmax rounds -------------------------------
// Order of the walk: largest d^2 first, ties by smallest row-major index = descending 64-bit key (d^2 << 32) | ~index (never 0).
// A round considers the pixels that come after the last accepted one in that order and lie >= n_min (squared) from every accepted
// one.  Record (int32): [0] accepted count, [1] unused, then (index, d^2) pairs.

__device__ __forceinline__ unsigned long long fe_block_max(unsigned long long v, unsigned long long* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k && s[threadIdx.x + k] > s[threadIdx.x]) s[threadIdx.x] = s[threadIdx.x + k];
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(256) void fe_far_stage1_kernel(const int32_t* __restrict__ d2, int H, int W, int n_min, const int32_t* rec,
                                                            unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s[256];
  __shared__ int s_cy[kFeFarMaxTopk], s_cx[kFeFarMaxTopk];
  const int cnt = min(rec[0], kFeFarMaxTopk);
  if ((int)threadIdx.x < cnt) {
    const int idx = rec[2 + 2 * threadIdx.x];
    s_cy[threadIdx.x] = idx / W;
    s_cx[threadIdx.x] = idx - (idx / W) * W;
  }
  unsigned long long last = ~0ull;
  if (cnt > 0) last = ((unsigned long long)(uint32_t)rec[3 + 2 * (cnt - 1)] << 32) | (uint32_t)~(uint32_t)rec[2 + 2 * (cnt - 1)];
  __syncthreads();
  const int n = H * W;
  unsigned long long best = 0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
    const unsigned long long key = ((unsigned long long)(uint32_t)d2[p] << 32) | (uint32_t)~(uint32_t)p;
    if (key >= last || key <= best) continue;
    const int y = p / W, x = p - y * W;
    bool ok = true;
    for (int k = 0; k < cnt; ++k) {
      const int dy = y - s_cy[k], dx = x - s_cx[k];
      ok = ok && dy * dy + dx * dx >= n_min;
    }
    if (ok) best = key;
  }
  best = fe_block_max(best, s);
  if (threadIdx.x == 0) part[blockIdx.x] = best;
}

__global__ __launch_bounds__(256) void fe_far_stage2_kernel(const unsigned long long* __restrict__ part, int nb, int topk, int32_t* rec) {
  __shared__ unsigned long long s[256];
  const unsigned long long best = fe_block_max((int)threadIdx.x < nb ? part[threadIdx.x] : 0ull, s);
  if (threadIdx.x == 0 && best != 0 && rec[0] < topk) {
    const int cnt = rec[0];
    rec[2 + 2 * cnt] = (int32_t)~(uint32_t)best;
    rec[3 + 2 * cnt] = (int32_t)(best >> 32);
    rec[0] = cnt + 1;
  }
}

}  // namespace npp

using namespace npp;

extern "C" int npp_resize_nearest_u8(const uint8_t* d_in_hw, int H, int W, uint8_t* d_out_hw, int h, int w, void* stream) {
  if (!d_in_hw || !d_out_hw || d_in_hw == d_out_hw || !fe_shape_ok(1, H, W) || !fe_shape_ok(1, h, w)) {
    set_error("npp_resize_nearest_u8: bad argument (H=%d W=%d -> h=%d w=%d, all >= 1; the output needs an array of its own)", H, W, h, w);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(fe_resize_nearest_kernel, dim3(fe_blocks((int64_t)h * w)), dim3(256), 0, (hipStream_t)stream, d_in_hw, H, W, h, w,
                     (double)H / (double)h, (double)W / (double)w, d_out_hw);
  return check_launch("npp_resize_nearest_u8");
}

extern "C" int npp_resize_linear_u8(const uint8_t* d_in_hw, int H, int W, uint8_t* d_out_hw, int h, int w, void* stream) {
  if (!d_in_hw || !d_out_hw || d_in_hw == d_out_hw || !fe_shape_ok(1, H, W) || !fe_shape_ok(1, h, w)) {
    set_error("npp_resize_linear_u8: bad argument (H=%d W=%d -> h=%d w=%d, all >= 1; the output needs an array of its own)", H, W, h, w);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(fe_resize_linear_kernel, dim3(fe_blocks((int64_t)h * w)), dim3(256), 0, (hipStream_t)stream, d_in_hw, H, W, h, w,
                     (double)H / (double)h, (double)W / (double)w, d_out_hw);
  return check_launch("npp_resize_linear_u8");
}

extern "C" int npp_normalize_u8(const float* d_in_chw, int C, int h, int w, uint8_t* d_out_chw, void* stream) {
  if (!d_in_chw || !d_out_chw || !fe_shape_ok(C, h, w)) {
    set_error("npp_normalize_u8: bad argument (C=%d in 1..65535, h=%d w=%d)", C, h, w);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(fe_normalize_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, d_in_chw, (int64_t)h * w, d_out_chw);
  return check_launch("npp_normalize_u8");
}

extern "C" int npp_gaussian_blur3_u8(const uint8_t* d_in_chw, int C, int h, int w, uint8_t* d_out_chw, void* stream) {
  if (!d_in_chw || !d_out_chw || d_in_chw == d_out_chw || !fe_shape_ok(C, h, w)) {
    set_error("npp_gaussian_blur3_u8: bad argument (C=%d in 1..65535, h=%d w=%d; the output needs an array of its own)", C, h, w);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(fe_blur3_kernel, dim3(fe_blocks((int64_t)h * w), (unsigned)C), dim3(256), 0, (hipStream_t)stream, d_in_chw, h, w,
                     d_out_chw);
  return check_launch("npp_gaussian_blur3_u8");
}

static bool fe_tiles_ok(int h, int w) { return (h + kFeTile - 1) / kFeTile <= 65535 && (w + kFeTile - 1) / kFeTile <= 65535; }
static dim3 fe_tile_grid(int C, int h, int w) {
  return dim3((unsigned)((w + kFeTile - 1) / kFeTile), (unsigned)((h + kFeTile - 1) / kFeTile), (unsigned)C);
}

extern "C" int npp_canny_mark(const uint8_t* d_img_chw, int C, int h, int w, int low, int high, uint8_t* d_map_chw, void* stream) {
  if (!d_img_chw || !d_map_chw || d_img_chw == d_map_chw || !fe_shape_ok(C, h, w) || !fe_tiles_ok(h, w) || low < 0 || high < low) {
    set_error("npp_canny_mark: bad argument (C=%d in 1..65535, h=%d w=%d, 0 <= low=%d <= high=%d; the map needs an array of its own)", C, h,
              w, low, high);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(fe_canny_mark_kernel, fe_tile_grid(C, h, w), dim3(256), 0, (hipStream_t)stream, d_img_chw, h, w, low, high, d_map_chw);
  return check_launch("npp_canny_mark");
}

extern "C" int npp_canny_hysteresis(uint8_t* d_map_chw, int C, int h, int w, int rounds, int32_t* d_flags, void* stream) {
  if (!d_map_chw || !d_flags || !fe_shape_ok(C, h, w) || !fe_tiles_ok(h, w) || rounds < 1 || rounds > 1024) {
    set_error("npp_canny_hysteresis: bad argument (C=%d in 1..65535, h=%d w=%d, rounds=%d in 1..1024)", C, h, w, rounds);
    return NPP_ERR_ARG;
  }
  if (hipMemsetAsync(d_flags, 0, sizeof(int32_t) * (size_t)rounds, (hipStream_t)stream) != hipSuccess) {
    set_error("npp_canny_hysteresis: clearing the flags failed");
    return NPP_ERR_LAUNCH;
  }
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(fe_hysteresis_kernel, fe_tile_grid(C, h, w), dim3(256), 0, (hipStream_t)stream, d_map_chw, h, w, d_flags + r);
  return check_launch("npp_canny_hysteresis");
}

extern "C" int npp_canny_finish(const uint8_t* d_map_chw, int C, int h, int w, uint8_t* d_out_chw, void* stream) {
  if (!d_map_chw || !d_out_chw || !fe_shape_ok(C, h, w) || (int64_t)C * h * w >= ((int64_t)1 << 38)) {
    set_error("npp_canny_finish: bad argument (C=%d in 1..65535, h=%d w=%d)", C, h, w);
    return NPP_ERR_ARG;
  }
  const int64_t n = (int64_t)C * h * w;
  hipLaunchKernelGGL(fe_canny_finish_kernel, dim3(fe_blocks(n)), dim3(256), 0, (hipStream_t)stream, d_map_chw, n, d_out_chw);
  return check_launch("npp_canny_finish");
}

extern "C" int npp_edge_count(const uint8_t* d_map_chw, int C, int h, int w, const uint8_t* d_eroded_hw, float* d_out_hw, void* stream) {
  if (!d_map_chw || !d_eroded_hw || !d_out_hw || !fe_shape_ok(C, h, w)) {
    set_error("npp_edge_count: bad argument (C=%d in 1..65535, h=%d w=%d)", C, h, w);
    return NPP_ERR_ARG;
  }
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(fe_edge_count_kernel, dim3(fe_blocks(n)), dim3(256), 0, (hipStream_t)stream, d_map_chw, C, n, d_eroded_hw, d_out_hw);
  return check_launch("npp_edge_count");
}

extern "C" int npp_edt_sq(const uint8_t* d_mask_hw, int H, int W, uint32_t* d_tmp_hw, int32_t* d_dsq_hw, void* stream) {
  if (!d_mask_hw || !d_tmp_hw || !d_dsq_hw || (const void*)d_tmp_hw == (const void*)d_dsq_hw || H < 1 || W < 1 || H > kFeMaxDim ||
      W > kFeMaxDim) {
    set_error("npp_edt_sq: bad argument (H=%d W=%d, both in 1..%d; tmp must be a buffer of its own)", H, W, kFeMaxDim);
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(fe_edt_col_kernel, dim3(fe_blocks(W)), dim3(256), 0, (hipStream_t)stream, d_mask_hw, H, W, d_tmp_hw);
  hipLaunchKernelGGL(fe_edt_row_kernel, dim3(fe_blocks(W), (unsigned)H), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)d_tmp_hw, W,
                     d_dsq_hw);
  return check_launch("npp_edt_sq");
}

extern "C" int npp_far_points(const int32_t* d_dsq_hw, int H, int W, int topk, int n_min, void* d_scratch, int32_t* d_record, void* stream) {
  if (!d_dsq_hw || !d_scratch || !d_record || H < 1 || W < 1 || H > kFeMaxDim || W > kFeMaxDim || topk < 1 || topk > kFeFarMaxTopk ||
      n_min < 0) {
    set_error("npp_far_points: bad argument (H=%d W=%d, both in 1..%d; topk=%d in 1..%d; n_min=%d >= 0)", H, W, kFeMaxDim, topk,
              kFeFarMaxTopk, n_min);
    return NPP_ERR_ARG;
  }
  static_assert(kFeFarBlocks * 8 == NPP_FAR_POINTS_SCRATCH_BYTES, "far-point scratch");
  if (hipMemsetAsync(d_record, 0, sizeof(int32_t) * (size_t)(2 + 2 * topk), (hipStream_t)stream) != hipSuccess) {
    set_error("npp_far_points: clearing the record failed");
    return NPP_ERR_LAUNCH;
  }
  const int64_t n = (int64_t)H * W;
  const int nb = (int)(fe_blocks(n) < (unsigned)kFeFarBlocks ? fe_blocks(n) : (unsigned)kFeFarBlocks);
  for (int r = 0; r < topk; ++r) {
    hipLaunchKernelGGL(fe_far_stage1_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, d_dsq_hw, H, W, n_min,
                       (const int32_t*)d_record, (unsigned long long*)d_scratch);
    hipLaunchKernelGGL(fe_far_stage2_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)d_scratch, nb, topk,
                       d_record);
  }
  return check_launch("npp_far_points");
}
