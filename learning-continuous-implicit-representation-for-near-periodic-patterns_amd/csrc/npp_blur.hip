// npp_blur.hip -- the remapping task's blur detection (NPP_remapping/blur_detection.py:13-60): the gray conversion, the per-pixel
// share of the largest singular values of the 20 x 20 gray block around every pixel, and the binary erosion / dilation of the
// thresholded map.  The normalisation and the percentile between them are a few passes over H W numbers and stay with the caller
// (blur.py).  Nothing is kept in device memory between launches and there are no atomics: every entry is bit-reproducible.
#include "npp_common.h"

namespace npp {

constexpr int kBlurWin = 10;                            // win_size of blur_detection.py:13 (the block is 2 win_size wide)
constexpr int kBlurN = 2 * kBlurWin;                    // 20 x 20 block
constexpr int kBlurTile = 16;                           // output pixels per workgroup side
constexpr int kBlurStage = kBlurTile + kBlurN - 1;      // 35 x 35 gray bytes feed a tile
constexpr int kBlurSlots = 3;                           // windows per wave: 3 x 20 lanes, 4 lanes idle
constexpr int kBlurPasses = (kBlurTile * kBlurTile + 4 * kBlurSlots - 1) / (4 * kBlurSlots);
// Sweeps: cyclic Jacobi converges quadratically once the columns are nearly orthogonal.  tests/blur_restatement.py restates this
// very loop (same ordering, same tolerance) in NumPy and tests/test_blur_cpu.py runs it on the window kinds of the tests: uniform
// and saturated noise are the slowest with at most 12 sweeps, the last of which only finds nothing left to rotate (rank <= 3
// and flat blocks need 1-7, ramps 9), and the share then lies within 1e-13 of LAPACK's; with the tolerance loosened to 1e-6 it
// still lies within 1e-11.  16 leaves four sweeps in hand; a block that did reach the cap would be returned as it stands.
constexpr int kBlurSweeps = 16;
constexpr double kBlurTol = 1e-9;                       // rotate while |a_p . a_q| > tol |a_p| |a_q|

// ---- blur_detection.py:14: cv2.cvtColor(img, COLOR_RGB2GRAY) on uint8, OpenCV's 14-bit fixed point --------------------------
__global__ __launch_bounds__(256) void rgb_to_gray_u8_kernel(const uint8_t* __restrict__ img, int64_t n, uint8_t* __restrict__ gray) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint8_t* q = img + p * 3;
  gray[p] = (uint8_t)(((uint32_t)q[0] * 4899u + (uint32_t)q[1] * 9617u + (uint32_t)q[2] * 1868u + 8192u) >> 14);
}

// blur_detection.py:18-29: source row (column) of row i of the padded image, i in [0, n + 20).  Not a plain reflection: the far
// border restarts at n - 10.  For n < 19 the far border's index 2n - i runs below zero and NumPy counts from the end (p + n).
__device__ __forceinline__ int blur_mirror(int i, int n) {
  const int p = i < kBlurWin ? kBlurWin - i : (i > n + kBlurWin - 1 ? 2 * n - i : i - kBlurWin);
  return p < 0 ? p + n : p;
}

// ---- blur_detection.py:32-46: sum(s[:sv_num]) / (sum(s) + 1e-6) of every 20 x 20 block ---------------------------------------
// One 16 x 16 tile of output pixels per workgroup; its 35 x 35 gray bytes are gathered through the index map into LDS once.
// One-sided (Hestenes) Jacobi in float64, one column of a block per lane (20 values, rows indexed statically: no scratch), three
// blocks per wave.  Round-robin ordering: in step s of a sweep column 19 meets column s and column c meets (2s - c) mod 19, ten
// disjoint pairs at once, 19 steps per sweep; a column never leaves its lane, the partner's values come by lane permute.  Both
// lanes of a pair compute the same rotation from the same three numbers (|a_p|^2, |a_q|^2, a_p . a_q; the dot product's terms
// commute, the partner's norm is fetched, not recomputed), so they stay consistent bit for bit.  The singular values are the
// final column norms; the top sv_num are selected by rank (ties by column), not sorted.
__global__ __launch_bounds__(256) void blur_sv_share_kernel(const uint8_t* __restrict__ gray, int H, int W, int sv_num, double* __restrict__ out) {
  __shared__ uint8_t tile[kBlurStage][kBlurStage + 1];
  const int x0 = blockIdx.x * kBlurTile, y0 = blockIdx.y * kBlurTile;
  for (int e = threadIdx.x; e < kBlurStage * kBlurStage; e += 256) {
    const int r = e / kBlurStage, c = e - r * kBlurStage;
    const int py = y0 + r, px = x0 + c;
    uint8_t v = 0;
    if (py < H + kBlurN && px < W + kBlurN) v = gray[(int64_t)blur_mirror(py, H) * W + blur_mirror(px, W)];
    tile[r][c] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane / kBlurN, col = lane - slot * kBlurN;
  const bool lane_used = slot < kBlurSlots;
  const int base = slot * kBlurN;
  for (int pass = 0; pass < kBlurPasses; ++pass) {
    const int t = (pass * 4 + wave) * kBlurSlots + slot;
    const int ty = t / kBlurTile, tx = t - ty * kBlurTile;
    const bool live = lane_used && t < kBlurTile * kBlurTile && y0 + ty < H && x0 + tx < W;
    if (!__any(live)) continue;                                       // wave-uniform
    const int wy = live ? ty : 0, wx = live ? tx + col : 0;           // (lanes without a window stay inside the tile)
    double a[kBlurN];
#pragma unroll
    for (int r = 0; r < kBlurN; ++r) a[r] = live ? (double)tile[wy + r][wx] : 0.0;
    for (int sweep = 0; sweep < kBlurSweeps; ++sweep) {
      bool rotated = false;
#pragma unroll 1
      for (int s = 0; s < kBlurN - 1; ++s) {
        const int pc = col == kBlurN - 1 ? s : (col == s ? kBlurN - 1 : (2 * s - col + (kBlurN - 1)) % (kBlurN - 1));
        const int pl = lane_used ? base + pc : lane;
        double o[kBlurN];
#pragma unroll
        for (int r = 0; r < kBlurN; ++r) o[r] = __shfl(a[r], pl, 64);
        double nm = 0.0, g = 0.0;
#pragma unroll
        for (int r = 0; r < kBlurN; ++r) {
          nm = fma(a[r], a[r], nm);
          g = fma(a[r], o[r], g);
        }
        const double no = __shfl(nm, pl, 64);
        const bool lo = col < pc;
        const double al = lo ? nm : no, be = lo ? no : nm;            // the pair's (p, q) = (lower, higher) column
        const bool rot = g * g > (kBlurTol * kBlurTol) * (al * be) && fabs(g) > 1e-18;
        double cs = 1.0, sn = 0.0;
        if (rot) {
          const double zeta = (be - al) / (2.0 * g);
          const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
          cs = rsqrt(fma(tn, tn, 1.0));
          sn = cs * tn;
        }
        const double so = lo ? -sn : sn;                              // a_p' = c a_p - s a_q,  a_q' = s a_p + c a_q
#pragma unroll
        for (int r = 0; r < kBlurN; ++r) a[r] = fma(so, o[r], cs * a[r]);
        rotated |= rot;
      }
      if (!__any(rotated)) break;                                     // wave vote: all three blocks have converged
    }
    double nm = 0.0;
#pragma unroll
    for (int r = 0; r < kBlurN; ++r) nm = fma(a[r], a[r], nm);
    const double sv = sqrt(nm);
    int rank = 0;
    double total = sv;
#pragma unroll 1
    for (int k = 1; k < kBlurN; ++k) {
      const int oc = (col + k) % kBlurN;
      const double other = __shfl(sv, lane_used ? base + oc : lane, 64);
      rank += (other > sv || (other == sv && oc < col)) ? 1 : 0;
      total += other;
    }
    const double mine = rank < sv_num ? sv : 0.0;
    double top = mine;
#pragma unroll 1
    for (int k = 1; k < kBlurN; ++k) top += __shfl(mine, lane_used ? base + (col + k) % kBlurN : lane, 64);
    if (live && col == 0) out[(int64_t)(y0 + ty) * W + (x0 + tx)] = top / (total + 1e-6);
  }
}

// ---- blur_detection.py:54-56: scipy.ndimage.binary_erosion / binary_dilation(iterations = r), default cross, border 0 ---------
// r iterations of the 4-connected cross are one pass with the L1 ball of radius r (on the zero-padded image; for a dilation the
// image is a rectangle, so every shortest L1 path stays inside it).  The ball test is an exact L1 distance, built separably:
// pass 1 writes, per pixel, the distance along its row to the nearest TARGET pixel (erode: a zero, the image border counting as
// one; dilate: a one), capped at r + 1; pass 2 takes min over the rows dy of |dy| + that.  erode: keep where the distance > r;
// dilate: set where it is <= r.
__global__ __launch_bounds__(256) void morph_row_kernel(const uint8_t* __restrict__ in, int H, int W, int r, int dilate, uint8_t* __restrict__ d1) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const uint8_t* row = in + (int64_t)y * W;
  int d = r + 1;
  for (int k = 0; k <= r; ++k) {
    const int xl = x - k, xr = x + k;
    const bool hit_l = xl < 0 ? !dilate : ((row[xl] != 0) == (dilate != 0));
    const bool hit_r = xr >= W ? !dilate : ((row[xr] != 0) == (dilate != 0));
    if (hit_l || hit_r) { d = k; break; }
  }
  d1[p] = (uint8_t)d;
}

__global__ __launch_bounds__(256) void morph_col_kernel(const uint8_t* __restrict__ d1, int H, int W, int r, int dilate, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  int d = r + 1;
  if (!dilate) d = min(d, min(y + 1, H - y));                          // rows -1 and H are zeros
  const int ya = max(0, y - r), yb = min(H - 1, y + r);
  for (int yy = ya; yy <= yb; ++yy) d = min(d, abs(yy - y) + (int)d1[(int64_t)yy * W + x]);
  out[p] = dilate ? (d <= r ? 1 : 0) : (d > r ? 1 : 0);
}

static bool blur_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 38); }   // one thread per pixel, 256 per block
static unsigned blur_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace npp

using namespace npp;

extern "C" int npp_rgb_to_gray_u8(const uint8_t* d_img_hw3, int H, int W, uint8_t* d_gray_hw, void* stream) {
  if (!d_img_hw3 || !d_gray_hw || !blur_shape_ok(H, W)) {
    set_error("npp_rgb_to_gray_u8: bad argument (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(rgb_to_gray_u8_kernel, dim3(blur_blocks(n)), dim3(256), 0, (hipStream_t)stream, d_img_hw3, n, d_gray_hw);
  return check_launch("npp_rgb_to_gray_u8");
}

extern "C" int npp_blur_sv_share(const uint8_t* d_gray_hw, int H, int W, int sv_num, double* d_share_hw, void* stream) {
  if (!d_gray_hw || !d_share_hw || !blur_shape_ok(H, W) || H <= kBlurWin || W <= kBlurWin || sv_num < 1 || sv_num > kBlurN ||
      (H + kBlurTile - 1) / kBlurTile > 65535) {
    set_error("npp_blur_sv_share: bad argument (H=%d W=%d, both > %d; sv_num=%d in 1..%d)", H, W, kBlurWin, sv_num, kBlurN);
    return NPP_ERR_ARG;
  }
  const dim3 grid((unsigned)((W + kBlurTile - 1) / kBlurTile), (unsigned)((H + kBlurTile - 1) / kBlurTile));
  hipLaunchKernelGGL(blur_sv_share_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_gray_hw, H, W, sv_num, d_share_hw);
  return check_launch("npp_blur_sv_share");
}

extern "C" int npp_binary_morph(const uint8_t* d_in_hw, int H, int W, int iterations, int dilate, uint8_t* d_tmp_hw, uint8_t* d_out_hw,
                                void* stream) {
  if (!d_in_hw || !d_tmp_hw || !d_out_hw || !blur_shape_ok(H, W) || iterations < 1 || iterations > 254 || d_tmp_hw == d_out_hw ||
      d_tmp_hw == d_in_hw) {
    set_error("npp_binary_morph: bad argument (H=%d W=%d iterations=%d in 1..254; tmp must be a buffer of its own)", H, W, iterations);
    return NPP_ERR_ARG;
  }
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(morph_row_kernel, dim3(blur_blocks(n)), dim3(256), 0, (hipStream_t)stream, d_in_hw, H, W, iterations, dilate ? 1 : 0,
                     d_tmp_hw);
  hipLaunchKernelGGL(morph_col_kernel, dim3(blur_blocks(n)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_tmp_hw, H, W, iterations,
                     dilate ? 1 : 0, d_out_hw);
  return check_launch("npp_binary_morph");
}
