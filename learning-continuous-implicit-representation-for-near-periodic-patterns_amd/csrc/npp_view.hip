// npp_view.hip -- perspective views (view.py, DESIGN.md "Perspective views"): the uint8 image / mask warp under a 3 x 3 map with its
// coverage mask, and the host twins of the view rule.  The warp's positions and bilinear blend are float64 in the operation order
// include/npp_hip.h writes down, every product and sum rounded separately: one function body serves the kernel (spelt __d*_rn) and
// the host twin (plain operators; the file is built with -ffp-contract=off and the pragma holds it without the flag), so NumPy, the
// host and the device agree bit for bit.  One thread per canvas pixel, all channels; no atomics, no state between calls.  The
// antialiased warp (npp_warp_image_u8_ss) is the same thread looping over its pixel's ss x ss samples in the rule's order.
#include "npp_coord.h"

namespace npp {

#ifdef __HIP_DEVICE_COMPILE__
#define NPP_WARP_OP(name, intr, op) __host__ __device__ __forceinline__ double name(double a, double b) { return intr(a, b); }
#else
#define NPP_WARP_OP(name, intr, op) \
  __host__ __device__ __forceinline__ double name(double a, double b) { _Pragma("clang fp contract(off)") return a op b; }
#endif
NPP_WARP_OP(warp_mul, __dmul_rn, *)
NPP_WARP_OP(warp_add, __dadd_rn, +)
NPP_WARP_OP(warp_sub, __dsub_rn, -)
NPP_WARP_OP(warp_div, __ddiv_rn, /)
#undef NPP_WARP_OP

struct WarpMap { double m[9]; };

// Canvas pixel (i, j): C bytes of out and one of inside (nullable)
__host__ __device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ src, int Hs, int Ws, int C, const WarpMap& M, int mode,
                                                    int i, int j, uint8_t* __restrict__ out, uint8_t* __restrict__ inside) {
  const double fi = (double)i, fj = (double)j;
  const double d = warp_add(warp_add(warp_mul(M.m[6], fi), warp_mul(M.m[7], fj)), M.m[8]);
  const double y = warp_div(warp_add(warp_add(warp_mul(M.m[0], fi), warp_mul(M.m[1], fj)), M.m[2]), d);
  const double x = warp_div(warp_add(warp_add(warp_mul(M.m[3], fi), warp_mul(M.m[4], fj)), M.m[5]), d);
  bool in = d > 0.0 && __builtin_isfinite(y) && __builtin_isfinite(x);
  if (mode == 0) {
    // the comparisons are on the floored doubles: no integer conversion of a position out of range
    const double ry = floor(warp_add(y, 0.5)), rx = floor(warp_add(x, 0.5));
    in = in && ry >= 0.0 && ry < (double)Hs && rx >= 0.0 && rx < (double)Ws;
    const uint8_t* s = src + ((int64_t)(in ? (int)ry : 0) * Ws + (in ? (int)rx : 0)) * C;
    for (int c = 0; c < C; ++c) out[c] = in ? s[c] : 0;
  } else {
    in = in && y >= 0.0 && y <= (double)(Hs - 1) && x >= 0.0 && x <= (double)(Ws - 1);
    const double y0f = in ? floor(y) : 0.0, x0f = in ? floor(x) : 0.0;
    const int y0 = (int)y0f, x0 = (int)x0f;
    const int y1 = y0 + 1 < Hs ? y0 + 1 : Hs - 1, x1 = x0 + 1 < Ws ? x0 + 1 : Ws - 1;
    const double fy = in ? warp_sub(y, y0f) : 0.0, fx = in ? warp_sub(x, x0f) : 0.0;
    const double gy = warp_sub(1.0, fy), gx = warp_sub(1.0, fx);
    const uint8_t* r0 = src + (int64_t)y0 * Ws * C;
    const uint8_t* r1 = src + (int64_t)y1 * Ws * C;
    for (int c = 0; c < C; ++c) {
      const int64_t c0 = (int64_t)x0 * C + c, c1 = (int64_t)x1 * C + c;
      const double a00 = (double)r0[c0], a01 = (double)r0[c1], a10 = (double)r1[c0], a11 = (double)r1[c1];
      const double top = warp_add(warp_mul(gx, a00), warp_mul(fx, a01)), bot = warp_add(warp_mul(gx, a10), warp_mul(fx, a11));
      double v = floor(warp_add(warp_add(warp_mul(gy, top), warp_mul(fy, bot)), 0.5));
      v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
      out[c] = in ? (uint8_t)(int)v : 0;
    }
  }
  if (inside) *inside = in ? 255 : 0;
}

// ---- ss x ss samples per canvas pixel (include/npp_hip.h npp_warp_image_u8_ss) -----------------------------------------------------
// warp_pixel's rule taken apart for a loop over samples: the position and its taps once per sample (warp_tap), the unrounded value
// per channel (warp_value), the rounding once per pixel (warp_byte).  warp_pixel itself stays as it was written, so that the point
// kernel's code is instruction for instruction what it was; ss = 1 through these gives its bytes.

// One canvas position (fi, fj) under the map: whether it is in the source by its mode's test, where its taps lie (byte offsets of
// channel 0; nearest: o00 alone) and the bilinear weights.  A position outside computes on source pixel (0, 0).
struct WarpTap {
  bool in;
  int64_t o00, o01, o10, o11;
  double fy, fx, gy, gx;
};

__host__ __device__ __forceinline__ WarpTap warp_tap(int Hs, int Ws, int C, const WarpMap& M, int mode, double fi, double fj) {
  WarpTap t;
  const double d = warp_add(warp_add(warp_mul(M.m[6], fi), warp_mul(M.m[7], fj)), M.m[8]);
  const double y = warp_div(warp_add(warp_add(warp_mul(M.m[0], fi), warp_mul(M.m[1], fj)), M.m[2]), d);
  const double x = warp_div(warp_add(warp_add(warp_mul(M.m[3], fi), warp_mul(M.m[4], fj)), M.m[5]), d);
  bool in = d > 0.0 && __builtin_isfinite(y) && __builtin_isfinite(x);
  if (mode == 0) {
    // the comparisons are on the floored doubles: no integer conversion of a position out of range
    const double ry = floor(warp_add(y, 0.5)), rx = floor(warp_add(x, 0.5));
    in = in && ry >= 0.0 && ry < (double)Hs && rx >= 0.0 && rx < (double)Ws;
    t.o00 = t.o01 = t.o10 = t.o11 = ((int64_t)(in ? (int)ry : 0) * Ws + (in ? (int)rx : 0)) * C;
    t.fy = t.fx = t.gy = t.gx = 0.0;
  } else {
    in = in && y >= 0.0 && y <= (double)(Hs - 1) && x >= 0.0 && x <= (double)(Ws - 1);
    const double y0f = in ? floor(y) : 0.0, x0f = in ? floor(x) : 0.0;
    const int y0 = (int)y0f, x0 = (int)x0f;
    const int y1 = y0 + 1 < Hs ? y0 + 1 : Hs - 1, x1 = x0 + 1 < Ws ? x0 + 1 : Ws - 1;
    t.fy = in ? warp_sub(y, y0f) : 0.0;
    t.fx = in ? warp_sub(x, x0f) : 0.0;
    t.gy = warp_sub(1.0, t.fy);
    t.gx = warp_sub(1.0, t.fx);
    const int64_t r0 = (int64_t)y0 * Ws * C, r1 = (int64_t)y1 * Ws * C;
    t.o00 = r0 + (int64_t)x0 * C;
    t.o01 = r0 + (int64_t)x1 * C;
    t.o10 = r1 + (int64_t)x0 * C;
    t.o11 = r1 + (int64_t)x1 * C;
  }
  t.in = in;
  return t;
}

// Channel c of the source at a tap, before rounding: the tapped byte (nearest) or the blend in the written order (bilinear)
__host__ __device__ __forceinline__ double warp_value(const uint8_t* __restrict__ src, const WarpTap& t, int mode, int c) {
  if (mode == 0) return (double)src[t.o00 + c];
  const double a00 = (double)src[t.o00 + c], a01 = (double)src[t.o01 + c], a10 = (double)src[t.o10 + c], a11 = (double)src[t.o11 + c];
  const double top = warp_add(warp_mul(t.gx, a00), warp_mul(t.fx, a01)), bot = warp_add(warp_mul(t.gx, a10), warp_mul(t.fx, a11));
  return warp_add(warp_mul(t.gy, top), warp_mul(t.fy, bot));
}

__host__ __device__ __forceinline__ uint8_t warp_byte(double v) {
  v = floor(warp_add(v, 0.5));
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (uint8_t)(int)v;
}

// Canvas pixel (i, j) from its samples: sample a ss + b at (i + off[a], j + off[b]), reduced in that order over the samples that
// count; the pixel keeps the inside byte of its centre, and is empty where that is 0 or no sample counts.
__host__ __device__ __forceinline__ double warp_ss_off(int ss, int a) {
  return warp_sub(warp_div((double)(2 * a + 1), (double)(2 * ss)), 0.5);
}

__host__ __device__ __forceinline__ void warp_pixel_ss(const uint8_t* __restrict__ src, int Hs, int Ws, int C, const WarpMap& M, int mode,
                                                       int ss, int reduce, int i, int j, uint8_t* __restrict__ out,
                                                       uint8_t* __restrict__ inside) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};                   // reduce 0: the ordered sum; reduce 1: the smallest value so far
  int cnt = 0;
  if (warp_tap(Hs, Ws, C, M, mode, (double)i, (double)j).in) {      // a centre outside: empty whatever its samples say
    for (int a = 0; a < ss; ++a) {
      const double fi = warp_add((double)i, warp_ss_off(ss, a));
      for (int b = 0; b < ss; ++b) {
        const WarpTap t = warp_tap(Hs, Ws, C, M, mode, fi, warp_add((double)j, warp_ss_off(ss, b)));
        if (!t.in) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c)                       // unrolled with a guard: acc stays in registers
          if (c < C) {
            const double v = warp_value(src, t, mode, c);
            acc[c] = reduce == 0 ? warp_add(acc[c], v) : (cnt == 0 || v < acc[c] ? v : acc[c]);
          }
        ++cnt;
      }
    }
  }
  const double n = (double)(cnt ? cnt : 1);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < C) out[c] = cnt ? warp_byte(reduce == 0 ? warp_div(acc[c], n) : acc[c]) : 0;
  if (inside) *inside = cnt ? 255 : 0;
}

__global__ __launch_bounds__(256) void warp_image_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int C, int Ho, int Wo, WarpMap M,
                                                         int mode, uint8_t* __restrict__ out, uint8_t* __restrict__ inside) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)Ho * Wo) return;
  const int i = (int)(p / Wo), j = (int)(p - (int64_t)i * Wo);
  warp_pixel(src, Hs, Ws, C, M, mode, i, j, out + p * C, inside ? inside + p : nullptr);
}

__global__ __launch_bounds__(256) void warp_image_ss_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int C, int Ho, int Wo,
                                                            WarpMap M, int mode, int ss, int reduce, uint8_t* __restrict__ out,
                                                            uint8_t* __restrict__ inside) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)Ho * Wo) return;
  const int i = (int)(p / Wo), j = (int)(p - (int64_t)i * Wo);
  warp_pixel_ss(src, Hs, Ws, C, M, mode, ss, reduce, i, j, out + p * C, inside ? inside + p : nullptr);
}

// ---- the supersampling class of a view's canvas pixel (include/npp_hip.h "adaptive supersampling") ---------------------------------
// |det M| of a view's fp32 matrix in float64, in the written order: formed once on the host by the entry points
static double view_abs_det(const npp_view& v) {
  const double a = v.m[0], b = v.m[1], c = v.m[2], d1 = v.m[3], e = v.m[4], f = v.m[5], g = v.m[6], h = v.m[7], k = v.m[8];
  const double t0 = warp_mul(a, warp_sub(warp_mul(e, k), warp_mul(f, h)));
  const double t1 = warp_mul(b, warp_sub(warp_mul(d1, k), warp_mul(f, g)));
  const double t2 = warp_mul(c, warp_sub(warp_mul(d1, h), warp_mul(e, g)));
  return fabs(warp_add(warp_sub(t0, t1), t2));
}

// Canvas pixel p (row-major): class 0 where the point launch's inside byte (returned in `in`) is 0; else the smallest S in {1, 2, 4, 8}
// with adet <= (2.25 S^2) t, t = (d d) d, d = |(m6 i + m7 j) + m8| in float64, every operation rounded separately; 8 where none does.
__host__ __device__ __forceinline__ uint8_t view_ss_class(const npp_view& v, int H, int W, double adet, int64_t p, uint8_t& in) {
  float y, x;
  in = view_coord(v, H, W, p, y, x);
  if (!in) return 0;
  const int64_t i = p / v.width;
  const double fi = (double)i, fj = (double)(p - i * v.width);
  const double d = fabs(warp_add(warp_add(warp_mul((double)v.m[6], fi), warp_mul((double)v.m[7], fj)), (double)v.m[8]));
  const double t = warp_mul(warp_mul(d, d), d);
  return adet <= warp_mul(2.25, t) ? 1 : adet <= warp_mul(9.0, t) ? 2 : adet <= warp_mul(36.0, t) ? 4 : 8;
}

__global__ __launch_bounds__(256) void view_ss_classes_kernel(npp_view v, int H, int W, double adet, uint8_t* __restrict__ cls,
                                                              uint8_t* __restrict__ inside) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= v.n) return;
  uint8_t in;
  cls[r] = view_ss_class(v, H, W, adet, v.start + r, in);
  if (inside) inside[r] = in;
}

static int classes_check(const char* who, const npp_view* view, int H, int W, const void* cls) {
  const int rc = check_view(view, who);
  if (rc) return rc;
  if (H < 1 || W < 1) { set_error("%s: image size %d x %d must be >= 1", who, H, W); return NPP_ERR_ARG; }
  if (view->n > 0 && !cls) { set_error("%s: null pointer", who); return NPP_ERR_ARG; }
  return NPP_OK;
}

static int warp_check(const char* who, const void* src, int Hs, int Ws, int C, int Ho, int Wo, const double* m, int mode, const void* out) {
  if (!src || !out || src == out || !m) { set_error("%s: null pointer (the output needs an array of its own)", who); return NPP_ERR_ARG; }
  if (Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || (int64_t)Hs * Ws >= ((int64_t)1 << 31) || (int64_t)Ho * Wo >= ((int64_t)1 << 31)) {
    set_error("%s: bad shape (source %d x %d, canvas %d x %d: all >= 1 and fewer than 2^31 pixels)", who, Hs, Ws, Ho, Wo);
    return NPP_ERR_ARG;
  }
  if (C < 1 || C > 4) { set_error("%s: C=%d channels (1..4)", who, C); return NPP_ERR_ARG; }
  if (mode != 0 && mode != 1) { set_error("%s: mode=%d (0 nearest, 1 bilinear)", who, mode); return NPP_ERR_ARG; }
  for (int k = 0; k < 9; ++k)
    if (!isfinite(m[k])) { set_error("%s: matrix entry m[%d] = %g is not finite", who, k, m[k]); return NPP_ERR_ARG; }
  return NPP_OK;
}

static int warp_check_ss(const char* who, const void* src, int Hs, int Ws, int C, int Ho, int Wo, const double* m, int mode, int ss,
                         int reduce, const void* out) {
  const int rc = warp_check(who, src, Hs, Ws, C, Ho, Wo, m, mode, out);
  if (rc) return rc;
  if (ss != 1 && ss != 2 && ss != 4 && ss != 8) { set_error("%s: ss=%d samples per canvas pixel and direction (1, 2, 4 or 8)", who, ss); return NPP_ERR_ARG; }
  if (reduce != 0 && reduce != 1) { set_error("%s: reduce=%d (0 mean, 1 min)", who, reduce); return NPP_ERR_ARG; }
  return NPP_OK;
}

}  // namespace npp

using namespace npp;

extern "C" int npp_warp_image_u8(const uint8_t* d_src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, uint8_t* d_out,
                                 uint8_t* d_inside, void* stream) {
  const int rc = warp_check("npp_warp_image_u8", d_src, Hs, Ws, C, Ho, Wo, m, mode, d_out);
  if (rc) return rc;
  WarpMap M;
  for (int k = 0; k < 9; ++k) M.m[k] = m[k];
  hipLaunchKernelGGL(warp_image_kernel, dim3((unsigned)(((int64_t)Ho * Wo + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_src, Hs, Ws,
                     C, Ho, Wo, M, mode, d_out, d_inside);
  return check_launch("npp_warp_image_u8");
}

extern "C" int npp_warp_image_u8_host(const uint8_t* src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, uint8_t* out,
                                      uint8_t* inside) {
  const int rc = warp_check("npp_warp_image_u8_host", src, Hs, Ws, C, Ho, Wo, m, mode, out);
  if (rc) return rc;
  WarpMap M;
  for (int k = 0; k < 9; ++k) M.m[k] = m[k];
  for (int i = 0; i < Ho; ++i)
    for (int j = 0; j < Wo; ++j) {
      const int64_t p = (int64_t)i * Wo + j;
      warp_pixel(src, Hs, Ws, C, M, mode, i, j, out + p * C, inside ? inside + p : nullptr);
    }
  return NPP_OK;
}

extern "C" int npp_warp_image_u8_ss(const uint8_t* d_src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, int ss,
                                    int reduce, uint8_t* d_out, uint8_t* d_inside, void* stream) {
  const int rc = warp_check_ss("npp_warp_image_u8_ss", d_src, Hs, Ws, C, Ho, Wo, m, mode, ss, reduce, d_out);
  if (rc) return rc;
  WarpMap M;
  for (int k = 0; k < 9; ++k) M.m[k] = m[k];
  hipLaunchKernelGGL(warp_image_ss_kernel, dim3((unsigned)(((int64_t)Ho * Wo + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_src, Hs,
                     Ws, C, Ho, Wo, M, mode, ss, reduce, d_out, d_inside);
  return check_launch("npp_warp_image_u8_ss");
}

extern "C" int npp_warp_image_u8_ss_host(const uint8_t* src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, int ss,
                                         int reduce, uint8_t* out, uint8_t* inside) {
  const int rc = warp_check_ss("npp_warp_image_u8_ss_host", src, Hs, Ws, C, Ho, Wo, m, mode, ss, reduce, out);
  if (rc) return rc;
  WarpMap M;
  for (int k = 0; k < 9; ++k) M.m[k] = m[k];
  for (int i = 0; i < Ho; ++i)
    for (int j = 0; j < Wo; ++j) {
      const int64_t p = (int64_t)i * Wo + j;
      warp_pixel_ss(src, Hs, Ws, C, M, mode, ss, reduce, i, j, out + p * C, inside ? inside + p : nullptr);
    }
  return NPP_OK;
}

// The positions and inside bytes of a view launch (npp_mlp_fwd_view / npp_mlp_fwd32_view) on the host: view_coord of npp_coord.h
extern "C" int npp_view_coords_host(const npp_view* view, int H, int W, float* out_yx, uint8_t* inside) {
  const char* who = "npp_view_coords_host";
  const int rc = check_view(view, who);
  if (rc) return rc;
  if (H < 1 || W < 1) { set_error("%s: image size %d x %d must be >= 1", who, H, W); return NPP_ERR_ARG; }
  if (view->n == 0) return NPP_OK;
  if (!out_yx) { set_error("%s: null pointer", who); return NPP_ERR_ARG; }
  for (int64_t r = 0; r < view->n; ++r) {
    float y, x;
    const uint8_t in = view_coord(*view, H, W, view->start + r, y, x);
    out_yx[2 * r] = y;
    out_yx[2 * r + 1] = x;
    if (inside) inside[r] = in;
  }
  return NPP_OK;
}

// The supersampling class (0, 1, 2, 4, 8) of canvas pixels [start, start + n), one thread per pixel, and the centre's inside byte
extern "C" int npp_view_ss_classes(const npp_view* view, int H, int W, uint8_t* d_cls, uint8_t* d_inside, void* stream) {
  const char* who = "npp_view_ss_classes";
  const int rc = classes_check(who, view, H, W, d_cls);
  if (rc || view->n == 0) return rc;
  hipLaunchKernelGGL(view_ss_classes_kernel, dim3((unsigned)((view->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *view, H, W,
                     view_abs_det(*view), d_cls, d_inside);
  return check_launch(who);
}

// ... and its host twin: the same function per pixel on host memory
extern "C" int npp_view_ss_classes_host(const npp_view* view, int H, int W, uint8_t* cls, uint8_t* inside) {
  const int rc = classes_check("npp_view_ss_classes_host", view, H, W, cls);
  if (rc) return rc;
  const double adet = view_abs_det(*view);
  for (int64_t r = 0; r < view->n; ++r) {
    uint8_t in;
    cls[r] = view_ss_class(*view, H, W, adet, view->start + r, in);
    if (inside) inside[r] = in;
  }
  return NPP_OK;
}

// The sample positions of a supersampled grid launch (npp_mlp_fwd_grid_ss / npp_mlp_fwd32_grid_ss) on the host: grid_sample of npp_coord.h
extern "C" int npp_grid_samples_host(const npp_grid* grid, int ss, float* out_yx) {
  const char* who = "npp_grid_samples_host";
  int rc = check_grid(grid, who);
  if (rc || (rc = check_ss(ss, grid->start, grid->n, grid->width, who)) || grid->n == 0) return rc;
  if (!out_yx) { set_error("%s: null pointer", who); return NPP_ERR_ARG; }
  for (int64_t r = 0; r < grid->n * ss * ss; ++r) grid_sample(*grid, ss, r, out_yx[2 * r], out_yx[2 * r + 1]);
  return NPP_OK;
}

// ... and of a supersampled view launch: view_sample per sample, view_coord of the pixel centre for the inside bytes
extern "C" int npp_view_samples_host(const npp_view* view, int ss, int H, int W, float* out_yx, uint8_t* sample_in_view, uint8_t* inside) {
  const char* who = "npp_view_samples_host";
  int rc = check_view(view, who);
  if (rc || (rc = check_ss(ss, view->start, view->n, view->width, who))) return rc;
  if (H < 1 || W < 1) { set_error("%s: image size %d x %d must be >= 1", who, H, W); return NPP_ERR_ARG; }
  if (view->n == 0) return NPP_OK;
  if (!out_yx) { set_error("%s: null pointer", who); return NPP_ERR_ARG; }
  const int ss2 = ss * ss;
  for (int64_t q = 0; q < view->n; ++q) {
    int cnt = 0;
    for (int64_t r = q * ss2; r < (q + 1) * ss2; ++r) {
      const uint8_t in = view_sample(*view, H, W, ss, r, out_yx[2 * r], out_yx[2 * r + 1]);
      cnt += in != 0;
      if (sample_in_view) sample_in_view[r] = in != 0;
    }
    float y, x;
    if (inside) inside[q] = cnt ? view_coord(*view, H, W, view->start + q, y, x) : 0;
  }
  return NPP_OK;
}
