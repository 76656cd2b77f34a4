// npp_slic.hip -- the per-pixel half of the segmentation task's INITIAL coarse segmentation (loaders/loaders.py:162-205): SLIC
// superpixels (imsegm/superpixels.py:53-64 -> skimage.segmentation.slic) and the per-superpixel colour statistics
// (imsegm/pipelines.py:253-278, descriptors.py:787-858).  What works on a few hundred superpixels -- the mixture model, the graph
// cut, the connectivity repair -- stays on the host (init_segment.py).
//
// Every kernel here gives bit-identical results from run to run: the sums over a superpixel's members are INTEGER sums (exact,
// so their order is irrelevant): pixel coordinates, 8-bit colours, doubled central differences and 256-bin histograms are integers
// to begin with; the Lab values of the centre update are rounded once, per pixel, to a 2^-20 fixed point before they are added.
// No float atomics anywhere (cdna_hip_programming.md Guideline 12).
#include "npp_common.h"

namespace npp {

struct SlicTaps { float w[9]; };            // Gaussian, sigma = 1, truncated at 4 sigma, normalised (scipy.ndimage.gaussian_filter)

// scipy.ndimage 'reflect' (d c b a | a b c d ...), valid for any n >= 1
__device__ __forceinline__ int slic_reflect(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
  return i;
}

// ---- prepare, pass 1: scale to [0, 1] by (v - vmin) * inv_range and blur along x; planar fp32 out (3, H, W) -----------------
__global__ __launch_bounds__(256) void slic_blur_x_kernel(const uint8_t* __restrict__ img, int H, int W, float vmin, float inv_range,
                                                          SlicTaps taps, float* __restrict__ tmp) {
  const int64_t hw = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int xs = slic_reflect(x + t - 4, W);
    const uint8_t* q = img + ((int64_t)y * W + xs) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += taps.w[t] * (((float)q[c] - vmin) * inv_range);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) tmp[c * hw + p] = acc[c];
}

__device__ __forceinline__ float srgb_linear(float v) { return v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f; }
__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; }

// ---- prepare, pass 2: blur along y, sRGB -> CIELAB (D65), times inv_m; planar fp32 out (3, H, W) ------------------------
__global__ __launch_bounds__(256) void slic_blur_y_lab_kernel(const float* __restrict__ tmp, int H, int W, SlicTaps taps, float inv_m,
                                                              float* __restrict__ lab) {
  const int64_t hw = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  float rgb[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int64_t q = (int64_t)slic_reflect(y + t - 4, H) * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] += taps.w[t] * tmp[c * hw + q];
  }
  const float r = srgb_linear(rgb[0]), g = srgb_linear(rgb[1]), b = srgb_linear(rgb[2]);
  const float X = (0.412453f * r + 0.357580f * g + 0.180423f * b) / 0.95047f;
  const float Y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
  const float Z = (0.019334f * r + 0.119193f * g + 0.950227f * b) / 1.08883f;
  const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
  lab[p] = (116.0f * fy - 16.0f) * inv_m;
  lab[hw + p] = (500.0f * (fx - fy)) * inv_m;
  lab[2 * hw + p] = (200.0f * (fy - fz)) * inv_m;
}

// ---- assign: one 16 x 16 pixel tile per workgroup ------------------------------------------------------------------------
// The centres are walked in chunks of 256; thread t of the block tests centre c0 + t against the tile's window (the tile grown by
// 2S) and the survivors go to an LDS list, which every pixel of the tile then scans.  The list's order is arbitrary (an LDS
// counter hands out the slots): the minimum is taken with an explicit tie rule (lowest k), so the result does not depend on it.
// A mask pixel with NO centre inside its own +-2S window (thin mask peninsulas) takes the nearest centre of all by the same D2,
// in a second walk that only tiles with such a pixel make.
constexpr int kSlicTile = 16;

struct SlicCand { float y, x, l, a, b; int k; };

__device__ __forceinline__ void slic_consider(const SlicCand& c, float py, float px, float l, float a, float b, float two_s, float inv_s2,
                                              bool windowed, float& best, int& best_k) {
  const float dy = c.y - py, dx = c.x - px;
  if (windowed && !(fabsf(dy) <= two_s && fabsf(dx) <= two_s)) return;
  const float dl = l - c.l, da = a - c.a, db = b - c.b;
  const float d2 = (dl * dl + da * da + db * db) + (dy * dy + dx * dx) * inv_s2;
  if (d2 < best || (d2 == best && c.k < best_k)) { best = d2; best_k = c.k; }
}

__global__ __launch_bounds__(256) void slic_assign_kernel(const float* __restrict__ lab, const uint8_t* __restrict__ mask, int H, int W,
                                                          const float* __restrict__ centres, int K, float S, int32_t* __restrict__ labels) {
  __shared__ SlicCand list[256];
  __shared__ int n_list;
  const int tx = threadIdx.x & (kSlicTile - 1), ty = threadIdx.x / kSlicTile;
  const int x0 = blockIdx.x * kSlicTile, y0 = blockIdx.y * kSlicTile;
  const int x = x0 + tx, y = y0 + ty;
  const bool in_img = x < W && y < H;
  const int64_t hw = (int64_t)H * W, p = (int64_t)y * W + x;
  const bool active = in_img && mask[p] != 0;
  float l = 0.0f, a = 0.0f, b = 0.0f;
  if (active) { l = lab[p]; a = lab[hw + p]; b = lab[2 * hw + p]; }
  const float py = (float)y, px = (float)x;
  const float two_s = 2.0f * S, inv_s2 = 1.0f / (S * S);
  const float wy0 = (float)y0 - two_s, wy1 = (float)(y0 + kSlicTile - 1) + two_s;
  const float wx0 = (float)x0 - two_s, wx1 = (float)(x0 + kSlicTile - 1) + two_s;
  float best = INFINITY;
  int best_k = -1;
  for (int pass = 0; pass < 2; ++pass) {
    const bool windowed = pass == 0;
    const bool search = active && (windowed || best_k < 0);
    for (int c0 = 0; c0 < K; c0 += 256) {
      if (threadIdx.x == 0) n_list = 0;
      __syncthreads();
      const int k = c0 + (int)threadIdx.x;
      if (k < K) {
        SlicCand c;
        c.y = centres[k * 5]; c.x = centres[k * 5 + 1]; c.l = centres[k * 5 + 2]; c.a = centres[k * 5 + 3]; c.b = centres[k * 5 + 4];
        c.k = k;
        if (!windowed || (c.y >= wy0 && c.y <= wy1 && c.x >= wx0 && c.x <= wx1)) list[atomicAdd(&n_list, 1)] = c;   // (<= 256 slots)
      }
      __syncthreads();
      const int n = n_list;
      if (search)
        for (int i = 0; i < n; ++i) slic_consider(list[i], py, px, l, a, b, two_s, inv_s2, windowed, best, best_k);
      __syncthreads();
    }
    if (!__syncthreads_or(active && best_k < 0)) break;        // every mask pixel of the tile has found a centre in its window
  }
  if (in_img) labels[p] = active ? best_k + 1 : 0;             // (K >= 1: an active pixel always ends with a centre)
}

// ---- update: integer member sums, then the means ---------------------------------------------------------------------------
constexpr float kSlicFix = 1048576.0f;        // 2^20: the Lab (/ m) values enter their sums rounded to this fixed point

__global__ __launch_bounds__(256) void slic_sum_kernel(const float* __restrict__ lab, const int32_t* __restrict__ labels, int H, int W,
                                                       int K, unsigned long long* __restrict__ acc) {
  const int64_t hw = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int k = labels[p] - 1;
  if (k < 0 || k >= K) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  unsigned long long* a = acc + (int64_t)k * 6;
  atomicAdd(a, 1ull);
  atomicAdd(a + 1, (unsigned long long)y);
  atomicAdd(a + 2, (unsigned long long)x);
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(a + 3 + c, (unsigned long long)llrintf(lab[c * hw + p] * kSlicFix));   // (two's complement: signed sums)
}

__global__ __launch_bounds__(256) void slic_mean_kernel(const unsigned long long* __restrict__ acc, int K, float* __restrict__ centres) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const unsigned long long* a = acc + (int64_t)k * 6;
  const unsigned long long n = a[0];
  if (n == 0) return;                                           // a centre without members keeps its previous value
  const double inv = 1.0 / (double)n;
  centres[k * 5] = (float)((double)a[1] * inv);
  centres[k * 5 + 1] = (float)((double)a[2] * inv);
#pragma unroll
  for (int c = 0; c < 3; ++c) centres[k * 5 + 2 + c] = (float)((double)(long long)a[3 + c] * inv * (1.0 / (double)kSlicFix));
}

// ---- features: integer sums and histograms per superpixel, then means and exact medians --------------------------------------
// acc: [N][9] 64-bit sums (count, y, x, colour x 3, 2 * (d/dy + d/dx) x 3); hist: [N][3][256] 32-bit counts.
__device__ __forceinline__ int slic_grad2(const uint8_t* __restrict__ img, int y, int x, int c, int H, int W) {
  // 2 * (np.gradient(ch)[0] + np.gradient(ch)[1]) at (y, x): central differences inside, one-sided at the border
  auto v = [&](int yy, int xx) { return (int)img[((int64_t)yy * W + xx) * 3 + c]; };
  const int gy = y == 0 ? 2 * (v(1, x) - v(0, x)) : y == H - 1 ? 2 * (v(H - 1, x) - v(H - 2, x)) : v(y + 1, x) - v(y - 1, x);
  const int gx = x == 0 ? 2 * (v(y, 1) - v(y, 0)) : x == W - 1 ? 2 * (v(y, W - 1) - v(y, W - 2)) : v(y, x + 1) - v(y, x - 1);
  return gy + gx;
}

__global__ __launch_bounds__(256) void slic_feat_sum_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ labels, int H, int W,
                                                            int N, unsigned long long* __restrict__ acc, unsigned* __restrict__ hist) {
  const int64_t hw = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int k = labels[p] - 1;                                  // label 0 (outside the mask) is skipped
  if (k < 0 || k >= N) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  unsigned long long* a = acc + (int64_t)k * 9;
  atomicAdd(a, 1ull);
  atomicAdd(a + 1, (unsigned long long)y);
  atomicAdd(a + 2, (unsigned long long)x);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned v = img[p * 3 + c];
    atomicAdd(a + 3 + c, (unsigned long long)v);
    atomicAdd(a + 6 + c, (unsigned long long)(long long)slic_grad2(img, y, x, c, H, W));
    atomicAdd(hist + ((int64_t)k * 3 + c) * 256 + v, 1u);
  }
}

// one thread per (superpixel, channel); feat row: cy, cx, mean x 3, median x 3, meanGrad x 3.  An empty superpixel gives NaN
// (numpy's mean of nothing) and count 0.
__global__ __launch_bounds__(256) void slic_feat_out_kernel(const unsigned long long* __restrict__ acc, const unsigned* __restrict__ hist, int N,
                                                            int32_t* __restrict__ count, float* __restrict__ feat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * 3) return;
  const int k = i / 3, c = i - k * 3;
  const unsigned long long* a = acc + (int64_t)k * 9;
  const unsigned long long n = a[0];
  float* f = feat + (int64_t)k * 11;
  if (c == 0) count[k] = (int32_t)n;
  if (n == 0) {
    if (c < 2) f[c] = NAN;
    f[2 + c] = NAN; f[5 + c] = NAN; f[8 + c] = NAN;
    return;
  }
  const double inv = 1.0 / (double)n;
  if (c < 2) f[c] = (float)((double)a[1 + c] * inv);
  f[2 + c] = (float)((double)a[3 + c] * inv);
  f[8 + c] = (float)((double)(long long)a[6 + c] * inv * 0.5);
  // median: ranks (n - 1) / 2 and n / 2 of the sorted values (equal for odd n)
  const unsigned* h = hist + ((int64_t)k * 3 + c) * 256;
  const unsigned long long r0 = (n - 1) / 2, r1 = n / 2;
  unsigned long long seen = 0;
  int v0 = -1, v1 = -1;
  for (int v = 0; v < 256 && v1 < 0; ++v) {
    seen += h[v];
    if (v0 < 0 && seen > r0) v0 = v;
    if (seen > r1) v1 = v;
  }
  f[5 + c] = 0.5f * (float)(v0 + v1);
}

static SlicTaps slic_taps() {
  SlicTaps t;
  double w[9], s = 0.0;
  for (int i = 0; i < 9; ++i) { w[i] = exp(-0.5 * (double)((i - 4) * (i - 4))); s += w[i]; }
  for (int i = 0; i < 9; ++i) t.w[i] = (float)(w[i] / s);
  return t;
}

}  // namespace npp

using namespace npp;

static inline unsigned slic_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
static inline bool slic_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= (int64_t)1 << 30; }

extern "C" int npp_slic_prepare(const uint8_t* d_img_hw3, int H, int W, float vmin, float vmax, float m, float* d_tmp_3hw, float* d_lab_3hw,
                                void* stream) {
  if (!d_img_hw3 || !d_tmp_3hw || !d_lab_3hw || !slic_shape_ok(H, W) || !(m > 0.0f) || !(vmax >= vmin)) {
    set_error("npp_slic_prepare: bad argument (H=%d W=%d m=%g min=%g max=%g)", H, W, (double)m, (double)vmin, (double)vmax);
    return NPP_ERR_ARG;
  }
  const SlicTaps taps = slic_taps();
  const int64_t hw = (int64_t)H * W;
  const float inv_range = vmax > vmin ? 1.0f / (vmax - vmin) : 0.0f;          // a constant image scales to zeros
  hipLaunchKernelGGL(slic_blur_x_kernel, dim3(slic_blocks(hw)), dim3(256), 0, (hipStream_t)stream, d_img_hw3, H, W, vmin, inv_range, taps,
                     d_tmp_3hw);
  hipLaunchKernelGGL(slic_blur_y_lab_kernel, dim3(slic_blocks(hw)), dim3(256), 0, (hipStream_t)stream, (const float*)d_tmp_3hw, H, W, taps,
                     1.0f / m, d_lab_3hw);
  return check_launch("npp_slic_prepare");
}

extern "C" int npp_slic_assign(const float* d_lab_3hw, const uint8_t* d_mask_hw, int H, int W, const float* d_centres_k5, int K, float S,
                               int32_t* d_labels_hw, void* stream) {
  if (!d_lab_3hw || !d_mask_hw || !d_centres_k5 || !d_labels_hw || !slic_shape_ok(H, W) || K < 1 || !(S > 0.0f)) {
    set_error("npp_slic_assign: bad argument (H=%d W=%d K=%d S=%g)", H, W, K, (double)S);
    return NPP_ERR_ARG;
  }
  const dim3 grid((unsigned)((W + kSlicTile - 1) / kSlicTile), (unsigned)((H + kSlicTile - 1) / kSlicTile));
  hipLaunchKernelGGL(slic_assign_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_lab_3hw, d_mask_hw, H, W, d_centres_k5, K, S, d_labels_hw);
  return check_launch("npp_slic_assign");
}

extern "C" int64_t npp_slic_update_scratch_bytes(int K) {
  if (K < 1) { set_error("npp_slic_update_scratch_bytes: K=%d", K); return NPP_ERR_ARG; }
  return (int64_t)K * 6 * 8;
}

extern "C" int npp_slic_update(const float* d_lab_3hw, const int32_t* d_labels_hw, int H, int W, float* d_centres_k5, int K, void* d_scratch,
                               int64_t scratch_bytes, void* stream) {
  if (!d_lab_3hw || !d_labels_hw || !d_centres_k5 || !d_scratch || !slic_shape_ok(H, W) || K < 1 || scratch_bytes < (int64_t)K * 6 * 8) {
    set_error("npp_slic_update: bad argument (H=%d W=%d K=%d scratch=%lld)", H, W, K, (long long)scratch_bytes);
    return NPP_ERR_ARG;
  }
  if (hipMemsetAsync(d_scratch, 0, (size_t)K * 6 * 8, (hipStream_t)stream) != hipSuccess) return check_launch("npp_slic_update (memset)");
  hipLaunchKernelGGL(slic_sum_kernel, dim3(slic_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream, d_lab_3hw, d_labels_hw, H, W, K,
                     (unsigned long long*)d_scratch);
  hipLaunchKernelGGL(slic_mean_kernel, dim3(slic_blocks(K)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)d_scratch, K,
                     d_centres_k5);
  return check_launch("npp_slic_update");
}

extern "C" int64_t npp_slic_features_scratch_bytes(int N) {
  if (N < 1) { set_error("npp_slic_features_scratch_bytes: N=%d", N); return NPP_ERR_ARG; }
  return (int64_t)N * (9 * 8 + 3 * 256 * 4);
}

extern "C" int npp_slic_features(const uint8_t* d_img_hw3, const int32_t* d_labels_hw, int H, int W, int N, int32_t* d_count_n, float* d_feat_n11,
                                 void* d_scratch, int64_t scratch_bytes, void* stream) {
  if (!d_img_hw3 || !d_labels_hw || !d_count_n || !d_feat_n11 || !d_scratch || !slic_shape_ok(H, W) || H < 2 || W < 2 || N < 1 ||
      scratch_bytes < (int64_t)N * (9 * 8 + 3 * 256 * 4)) {
    set_error("npp_slic_features: bad argument (H=%d W=%d (>= 2 each: np.gradient) N=%d scratch=%lld)", H, W, N, (long long)scratch_bytes);
    return NPP_ERR_ARG;
  }
  const size_t used = (size_t)N * (9 * 8 + 3 * 256 * 4);
  if (hipMemsetAsync(d_scratch, 0, used, (hipStream_t)stream) != hipSuccess) return check_launch("npp_slic_features (memset)");
  unsigned long long* acc = (unsigned long long*)d_scratch;
  unsigned* hist = (unsigned*)(acc + (size_t)N * 9);
  hipLaunchKernelGGL(slic_feat_sum_kernel, dim3(slic_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream, d_img_hw3, d_labels_hw, H, W, N,
                     acc, hist);
  hipLaunchKernelGGL(slic_feat_out_kernel, dim3(slic_blocks((int64_t)N * 3)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)acc,
                     (const unsigned*)hist, N, d_count_n, d_feat_n11);
  return check_launch("npp_slic_features");
}
