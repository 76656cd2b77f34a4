// npp_coord.h -- the embedder's maths (warped coordinates, precise sin / cos), how a row's position enters the forward kernels and
// how its colour leaves them (include/npp_hip.h "continuous coordinates"), with the host-side argument checks the entry points of
// those kernels share.  A new coordinate mode is one
// CoordMode value, one branch in row_coord and one in store_rgb, one entry point per chain and one table row in ops.render.  (The
// supersampled modes also need the samples of a pixel together: average_rgb, behind a barrier after store_rgb.  The listed mode is
// the supersampled view over pixels named by an index list: the same three branches.)
#pragma once
#include "npp_common.h"

namespace npp {

// ---- embedder maths ----------------------------------------------------------------------------------------------------------
// Embedder constants precomputed on the host from npp_embed_cfg (kernel argument).
// models/embedder.py:117-127: freq = period + offset, theta = deg2rad(angle).
struct EmbedDev {
  int32_t K, H, W, pad;
  float inv_w, inv_h;
  float cs[NPP_MAX_K][2], sn[NPP_MAX_K][2];            // cos/sin(theta_i)
  float per[NPP_MAX_K][2][NPP_N_OFF];                  // period_i + offset_o
  float freq[NPP_N_FREQ];                              // Fourier freq (rad per unit)
  float freq_rev[NPP_N_FREQ];                          // freq / 2pi (revolutions)
};

// sin / cos of an fp32 argument to ~1 ulp without libm's slow path: three-term Cody-Waite reduction by pi/2 (exact products
// for |x| up to ~1e5 rad; the embedder's arguments are |f v| < ~50) + the cephes single-precision minimax polynomials on
// [-pi/4, pi/4].  ~20 vector instructions, no branches: what lets the precise fp32 embedder run at the store rate instead of
// at libm's (5.0 vs 2.4 TB/s at 1024^2).
__device__ __forceinline__ float sincos_pi2(float x, bool want_cos) {
  const float jf = rintf(x * 0.636619772367581343f);           // x * 2 / pi
  float y = fmaf(-jf, 1.5703125f, x);
  y = fmaf(-jf, 4.837512969970703125e-4f, y);
  y = fmaf(-jf, 7.54978995489188e-8f, y);
  const int q = ((int)jf + (want_cos ? 1 : 0)) & 3;
  const float z = y * y;
  const float s = fmaf(y * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), y);
  const float c = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                       fmaf(z, -0.5f, 1.0f));
  const float r = (q & 1) ? c : s;
  return (q & 2) ? -r : r;
}

// ---- a1: one warped coordinate (models/embedder.py:110-133) -------------------
// i in [0,22): 0 -> x/W*2-1 ; 1..10 -> sin/cos pairs of orientation 0 over the 5
// offsets ; 11 -> y/H*2-1 ; 12..21 -> orientation 1.
template <bool PRECISE>
__device__ __forceinline__ float warp_value(const EmbedDev& e, int p, int i, float y, float x) {
  const int ori = i >= 11;
  const int ii = ori ? i - 11 : i;
  if (ii == 0) {
    // (x / res[1] - 0.5) * 2   (embedder.py:112-113)
    return ori ? (y / (float)e.H - 0.5f) * 2.0f : (x / (float)e.W - 0.5f) * 2.0f;
  }
  const int o = (ii - 1) >> 1;
  const bool is_cos = (ii - 1) & 1;
  const float per = e.per[p][ori][o];
  // y*cos + x*sin, rounded like the reference's two torch ops (no fma contraction)
  const float t = __fadd_rn(__fmul_rn(y, e.cs[p][ori]), __fmul_rn(x, e.sn[p][ori]));
  if (PRECISE) {
    float r = fmodf(t, per);                       // torch.remainder: sign of divisor
    if (r != 0.0f && ((per < 0.0f) != (r < 0.0f))) r += per;
    const float phi = ((r / per) * 2.0f) * 3.14159265358979323846f;
    return sincos_pi2(phi, is_cos);
  } else {
    const float q = floorf(t / per);
    float r = fmaf(-q, per, t);                    // exact remainder for |q| < 2^24
    r = r < 0.0f ? r + per : r;
    r = r >= per ? r - per : r;
    const float rev = r / per;                     // phase in revolutions, [0,1)
    return is_cos ? __builtin_amdgcn_cosf(rev) : __builtin_amdgcn_sinf(rev);
  }
}

// Both functions of one argument from ONE reduction (bitwise the values sincos_pi2(x, false) / (x, true) return): the
// precise embedder needs sin(f v) and cos(f v) of every (frequency, coordinate) pair.
__device__ __forceinline__ void sincos_pi2_both(float x, float& sn, float& cs) {
  const float jf = rintf(x * 0.636619772367581343f);
  float y = fmaf(-jf, 1.5703125f, x);
  y = fmaf(-jf, 4.837512969970703125e-4f, y);
  y = fmaf(-jf, 7.54978995489188e-8f, y);
  const int q = (int)jf;
  const float z = y * y;
  const float s = fmaf(y * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), y);
  const float c = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                       fmaf(z, -0.5f, 1.0f));
  const float rs = (q & 1) ? c : s;
  sn = (q & 2) ? -rs : rs;
  const int qc = q + 1;
  const float rc = (qc & 1) ? c : s;
  cs = (qc & 2) ? -rc : rc;
}

// ---- host side: embedder constants and argument checks (npp_embed.hip) ----------------------------------------------------------
EmbedDev make_embed_dev(const npp_embed_cfg& c);
int check_embed_cfg(const npp_embed_cfg* c, const char* who);
// The canvas half of a grid / view launch: pixels [start, start + n) of a canvas `width` wide.  NPP_OK also for n == 0.
int check_canvas(int64_t start, int64_t n, int32_t width, const char* who);
int check_grid(const npp_grid* g, const char* who);
int check_view(const npp_view* v, const char* who);
// What supersampling adds to a checked canvas (include/npp_hip.h "supersampled launches"): ss in {1, 2, 4, 8}; with ss > 1 indices
// below 2^20 and n ss^2 rows within one launch
int check_ss(int ss, int64_t start, int64_t n, int32_t width, const char* who);
// What an index list adds to a checked supersampled view (include/npp_hip.h "listed launches"): n_list >= 0, a list where n_list > 0,
// n_list ss^2 rows within one launch
int check_list(int ss, const int64_t* pix, int64_t n_list, const char* who);

// The checks every fused-forward entry point makes before it launches, in this order: network width (NPP_ERR_UNSUPPORTED), the row
// count, null pointers, out_act (NPP_ERR_ARG).  canvas: `rows` is the pixel count n of a grid / view launch (already >= 0 by
// check_canvas; 0 passes before any pointer is looked at and the caller returns), else Bp of a launch on `coords`.
static inline int fwd_args_check(const char* who, int width, int64_t rows, bool canvas, const void* coords, const void* pack,
                                 const float* params, const void* out, int out_act) {
  if (width != NPP_WIDTH) { set_error("%s: width %d unsupported (build is %d)", who, width, NPP_WIDTH); return NPP_ERR_UNSUPPORTED; }
  if (canvas && rows == 0) return NPP_OK;
  if (!canvas && (rows <= 0 || rows % NPP_ROW_TILE || rows / NPP_ROW_TILE > 0x7fffffffLL)) {
    set_error("%s: Bp=%lld must be a positive multiple of %d (at most 2^31 - 1 tiles)", who, (long long)rows, NPP_ROW_TILE);
    return NPP_ERR_ARG;
  }
  if ((!canvas && !coords) || !pack || !params || !out) { set_error("%s: null pointer", who); return NPP_ERR_ARG; }
  if (out_act < 0 || out_act > 2) { set_error("%s: out_act=%d (0 raw, 1 sigmoid, 2 tanh)", who, out_act); return NPP_ERR_ARG; }
  return NPP_OK;
}
// ... behind the embedder configuration (the entry points that take one)
static inline int fwd_entry_check(const char* who, const npp_embed_cfg* cfg, int width, int64_t rows, bool canvas, const void* coords,
                                  const void* pack, const float* params, const void* out, int out_act) {
  const int rc = check_embed_cfg(cfg, who);
  return rc ? rc : fwd_args_check(who, width, rows, canvas, coords, pack, params, out, out_act);
}

// ---- coordinate intake of the render paths ------------------------------------------------------------------------------------
// Coordinate modes of the forward kernels: how row r's (y, x) enters.  A template parameter: the int32 form compiles as before.
// The SS modes are the grid and the view with ss x ss samples per canvas pixel, averaged in the store epilogue (src.ss > 1).
// kCoordViewList is the view's SS mode over a listed subset of the canvas window (src.pix; src.ss may be 1 there).
enum CoordMode { kCoordI32 = 0, kCoordF32 = 1, kCoordGrid = 2, kCoordView = 3, kCoordGridSS = 4, kCoordViewSS = 5, kCoordViewList = 6 };
constexpr bool coord_is_ss(int cm) { return cm == kCoordGridSS || cm == kCoordViewSS || cm == kCoordViewList; }

// What a view launch adds to the forward kernels' arguments (the other modes never read it)
struct ViewArgs {
  npp_view v;
  uint8_t* inside;        // nullable: v.n bytes
  int32_t H, W;           // the fit's image size (the rectangle of inside byte 3)
};

// The render-only tail of the forward kernels' argument structs (CM != kCoordI32, inference only): fp32 positions instead of the
// int32 coords, the implicit canvas grid (pred then holds g.n rows) or that canvas under a projective map (view.v.n rows)
struct CoordSrc {
  const float* coordsf;
  npp_grid g;
  ViewArgs view;
  int32_t ss;             // the SS modes: samples per canvas pixel in each direction (2, 4 or 8; the listed mode also 1)
  const int64_t* pix;     // the listed mode: n_list absolute row-major canvas pixel indices (include/npp_hip.h "listed launches")
  int64_t n_list;
};

// One separately rounded fp32 operation: the _rn intrinsics on the device, the plain operator on the host (every source is compiled
// with -ffp-contract=off, and the pragma holds it without the flag)
#ifdef __HIP_DEVICE_COMPILE__
#define NPP_VIEW_OP(name, intr, op) __host__ __device__ __forceinline__ float name(float a, float b) { return intr(a, b); }
#else
#define NPP_VIEW_OP(name, intr, op) \
  __host__ __device__ __forceinline__ float name(float a, float b) { _Pragma("clang fp contract(off)") return a op b; }
#endif
NPP_VIEW_OP(view_mul, __fmul_rn, *)
NPP_VIEW_OP(view_add, __fadd_rn, +)
NPP_VIEW_OP(view_div, __fdiv_rn, /)
#undef NPP_VIEW_OP

// Canvas pixel p (row-major) of a view (include/npp_hip.h npp_view): d = (m6 i + m7 j) + m8, y = ((m0 i + m1 j) + m2) / d,
// x = ((m3 i + m4 j) + m5) / d; i, j < 2^24 (checked at launch).  Returns the inside byte: 0 not in view (d <= 0 or a non-finite
// position; y = x = 0 then, so nothing non-finite enters the chain), 1 in view, 3 also inside [-0.5, H - 0.5) x [-0.5, W - 0.5).
// view_at: the same at the canvas position (fi, fj), which a supersampled launch places between the pixel centres.
__host__ __device__ __forceinline__ uint8_t view_at(const npp_view& v, int H, int W, float fi, float fj, float& y, float& x) {
  const float d = view_add(view_add(view_mul(v.m[6], fi), view_mul(v.m[7], fj)), v.m[8]);
  y = view_div(view_add(view_add(view_mul(v.m[0], fi), view_mul(v.m[1], fj)), v.m[2]), d);
  x = view_div(view_add(view_add(view_mul(v.m[3], fi), view_mul(v.m[4], fj)), v.m[5]), d);
  if (!(d > 0.0f && __builtin_isfinite(y) && __builtin_isfinite(x))) {
    y = x = 0.0f;
    return 0;
  }
  return y >= -0.5f && y < (float)H - 0.5f && x >= -0.5f && x < (float)W - 0.5f ? 3 : 1;
}
__host__ __device__ __forceinline__ uint8_t view_coord(const npp_view& v, int H, int W, int64_t p, float& y, float& x) {
  const int64_t i = p / v.width;
  return view_at(v, H, W, (float)i, (float)(int32_t)(p - i * v.width), y, x);
}

// Row r of a view launch: canvas pixel start + min(r, n - 1), as in a grid launch
__device__ __forceinline__ uint8_t view_row(const ViewArgs& a, int64_t r, float& y, float& x) {
  return view_coord(a.v, a.H, a.W, a.v.start + (r < a.v.n ? r : a.v.n - 1), y, x);
}

// Row r of a grid launch: canvas pixel start + min(r, n - 1) in row-major order (the surplus rows of the last 64-row tile
// compute on the last pixel and are not stored), at y = y0 + i / sy, x = x0 + j / sx -- an IEEE quotient, then a separate add;
// i, j < 2^24 (checked at launch), so their fp32 conversion is exact.
__device__ __forceinline__ void grid_coord(const npp_grid& g, int64_t r, float& y, float& x) {
  const int64_t p = g.start + (r < g.n ? r : g.n - 1);
  const int64_t i = p / g.width;
  const int32_t j = (int32_t)(p - i * g.width);
  y = __fadd_rn(g.y0, __fdiv_rn((float)i, g.sy));
  x = __fadd_rn(g.x0, __fdiv_rn((float)j, g.sx));
}

// ---- supersampled launches (include/npp_hip.h "supersampled launches") ---------------------------------------------------------
// Row r of a launch with ss x ss samples per pixel is sample r % ss^2 of canvas pixel start + min(r / ss^2, n - 1); ss^2 divides the
// 64-row tile, so a tile holds 64 / ss^2 whole pixels.  Sample s = a ss + b sits at the canvas position (i + off[a], j + off[b]),
// off[a] = (2 a + 1) / (2 ss) - 0.5: exact in fp32, and so is the sum for i, j < 2^20 (checked at launch).
__host__ __device__ __forceinline__ float ss_off(int ss, int a) { return view_add(view_div((float)(2 * a + 1), (float)(2 * ss)), -0.5f); }
__host__ __device__ __forceinline__ void ss_canvas_pos(int32_t width, int ss, int64_t start, int64_t n, int64_t r, float& fi, float& fj) {
  const int lg = __builtin_ctz((unsigned)ss);                 // ss is a power of two
  const int64_t q = r >> (2 * lg);
  const int s = (int)(r & ((1 << (2 * lg)) - 1));
  const int64_t p = start + (q < n ? q : n - 1);
  const int64_t i = p / width;
  fi = view_add((float)i, ss_off(ss, s >> lg));
  fj = view_add((float)(int32_t)(p - i * width), ss_off(ss, s & (ss - 1)));
}
// ... of a grid: the grid rule on that position (an IEEE quotient, then a separate add)
__host__ __device__ __forceinline__ void grid_sample(const npp_grid& g, int ss, int64_t r, float& y, float& x) {
  float fi, fj;
  ss_canvas_pos(g.width, ss, g.start, g.n, r, fi, fj);
  y = view_add(g.y0, view_div(fi, g.sy));
  x = view_add(g.x0, view_div(fj, g.sx));
}
// ... of a view: view_at's operation order; returns the sample's inside byte (0: it does not count and computes on (0, 0))
__host__ __device__ __forceinline__ uint8_t view_sample(const npp_view& v, int H, int W, int ss, int64_t r, float& y, float& x) {
  float fi, fj;
  ss_canvas_pos(v.width, ss, v.start, v.n, r, fi, fj);
  return view_at(v, H, W, fi, fj, y, x);
}

// ---- listed launches (include/npp_hip.h "listed launches") ---------------------------------------------------------------------
// Pixel q of a listed launch: pix[min(q, n_list - 1)] as an offset into the window [v.start, v.start + v.n), or -1 where the index
// lies outside it (such a pixel computes on the window's first pixel and stores nothing)
__device__ __forceinline__ int64_t list_pixel(const CoordSrc& src, int64_t q) {
  const int64_t w = src.pix[q < src.n_list ? q : src.n_list - 1] - src.view.v.start;
  return w >= 0 && w < src.view.v.n ? w : -1;
}
// Row r of a listed launch: sample r % ss^2 of listed pixel r / ss^2 at view_sample's position (ss = 1: the pixel centre, off[0] = 0)
__device__ __forceinline__ uint8_t list_sample(const CoordSrc& src, int64_t r, float& y, float& x) {
  const int lg2 = 2 * __builtin_ctz((unsigned)src.ss);
  const int64_t w = list_pixel(src, r >> lg2);
  float fi, fj;
  ss_canvas_pos(src.view.v.width, src.ss, src.view.v.start + (w < 0 ? 0 : w), 1, r & ((1 << lg2) - 1), fi, fj);
  return view_at(src.view.v, src.view.H, src.view.W, fi, fj, y, x);
}

// (y, x) of row r in coordinate mode CM: int32 pixel indices (coords, (N, 2) [y, x]), fp32 positions (src.coordsf, the same shape),
// the implicit grid or the view.  Returns the inside byte of the position: a view's (0: not in view, y = x = 0), 3 in every other mode.
template <int CM>
__device__ __forceinline__ uint8_t row_coord(const int32_t* coords, const CoordSrc& src, int64_t r, float& y, float& x) {
  if (CM == kCoordView) return view_row(src.view, r, y, x);
  if (CM == kCoordViewSS) return view_sample(src.view.v, src.view.H, src.view.W, src.ss, r, y, x);
  if (CM == kCoordViewList) return list_sample(src, r, y, x);
  if (CM == kCoordGridSS) {
    grid_sample(src.g, src.ss, r, y, x);
  } else if (CM == kCoordGrid) {
    grid_coord(src.g, r, y, x);
  } else if (CM == kCoordF32) {
    const float2 c = ((const float2*)src.coordsf)[r];
    y = c.x;
    x = c.y;
  } else {
    const int2 c = ((const int2*)coords)[r];
    y = (float)c.x;              // (row = y, col = x)
    x = (float)c.y;
  }
  return 3;
}

// Channel c of output row `row` leaves the chain as o: a grid launch stores exactly g.n rows; a view launch exactly view.v.n, with
// the inside byte formed again from the map (nothing is carried through the chain), zeros for a pixel not in view and the byte
// itself by the thread of channel 0; every other launch stores all its rows.  The SS modes store nothing here: o goes to
// stage[64 rows][3] in LDS, and behind it a view's thread of channel 0 leaves whether its sample counts; average_rgb follows behind
// a barrier.  `stage` is 4 * kStageWords bytes of LDS that nothing else uses until the kernel ends (null in every other mode).
constexpr int kStageWords = NPP_ROW_TILE * 4;
template <int CM>
__device__ __forceinline__ void store_rgb(const CoordSrc& src, float* pred, int64_t row, int c, float o, float* stage = nullptr) {
  if (coord_is_ss(CM)) {
    const int lr = (int)(row & (NPP_ROW_TILE - 1));
    stage[lr * 3 + c] = o;
    if (CM == kCoordViewSS && c == 0) {
      float y, x;
      ((uint32_t*)stage)[NPP_ROW_TILE * 3 + lr] = view_sample(src.view.v, src.view.H, src.view.W, src.ss, row, y, x) != 0;
    }
    if (CM == kCoordViewList && c == 0) {
      float y, x;
      ((uint32_t*)stage)[NPP_ROW_TILE * 3 + lr] = list_sample(src, row, y, x) != 0;
    }
  } else if (CM == kCoordView) {
    if (row < src.view.v.n) {
      float y, x;
      const uint8_t in = view_coord(src.view.v, src.view.H, src.view.W, src.view.v.start + row, y, x);   // (row < n: view_row without its clamp)
      pred[row * 3 + c] = in ? o : 0.0f;
      if (c == 0 && src.view.inside) src.view.inside[row] = in;
    }
  } else if (CM != kCoordGrid || row < src.g.n) pred[row * 3 + c] = o;
}

// The second half of an SS store, by every thread of the workgroup behind a barrier after store_rgb: thread 3 q + c < (64 / ss^2) * 3
// forms channel c of the tile's pixel q -- acc = +0, then the ss^2 staged samples in order, one rounded add for each that counts (in a
// grid all do), and an IEEE quotient by their number -- and stores it if the pixel is one of the launch's n.  A view's pixel keeps the
// inside byte of its centre (view_coord, what the point launch writes); where that is 0 or no sample counts it stores zeros and byte 0.
// The listed mode: pixel q of the tile is listed pixel row0 / ss^2 + q, stored at its place in the window (nothing for a surplus
// pixel or an index outside the window); with ss = 1 the colour is the one staged sample itself, as the point launch stores it
// (+0 + o would turn -0.0 into +0.0).
template <int CM>
__device__ __forceinline__ void average_rgb(const CoordSrc& src, float* pred, int64_t row0, int tid, const float* stage) {
  const int lg2 = 2 * __builtin_ctz((unsigned)src.ss);
  if (tid >= (NPP_ROW_TILE >> lg2) * 3) return;
  const int q = tid / 3, c = tid - q * 3;
  int64_t pix = (row0 >> lg2) + q;
  if (CM == kCoordViewList) {
    if (pix >= src.n_list || (pix = list_pixel(src, pix)) < 0) return;
  } else if (pix >= (CM == kCoordViewSS ? src.view.v.n : src.g.n)) return;
  const uint32_t* counts = (const uint32_t*)stage + NPP_ROW_TILE * 3;
  float acc = 0.0f;
  int cnt = 0;
  for (int s = 0; s < (1 << lg2); ++s) {
    const int lr = (q << lg2) + s;
    if (CM != kCoordGridSS && !counts[lr]) continue;
    acc = __fadd_rn(acc, stage[lr * 3 + c]);
    ++cnt;
  }
  uint8_t in = 3;
  if (CM != kCoordGridSS) {
    float y, x;
    in = cnt ? view_coord(src.view.v, src.view.H, src.view.W, src.view.v.start + pix, y, x) : 0;
    if (c == 0 && src.view.inside) src.view.inside[pix] = in;
  }
  if (CM == kCoordViewList && lg2 == 0) acc = stage[q * 3 + c];          // (cnt is 1 wherever `in` is not 0)
  pred[pix * 3 + c] = in ? __fdiv_rn(acc, (float)cnt) : 0.0f;
}

// ---- the warp table of the fused forward kernels --------------------------------------------------------------------------------
// Branch-free generation of the warped coordinates is driven by a small LDS table built once per workgroup, WarpEnt[K][22]: per
// warped coordinate cos / sin(theta), period, 1 / period and phase, or the linear form of the two normalised raw coordinates.
struct WarpEnt { float cs, sn, per, inv_per, phase, lin; };   // lin: value = t - 1 (normalised raw coordinate)
// (mlp_fwd32_kernel carries this loop written out: see the comment there)
__device__ __forceinline__ void build_warp_table(const EmbedDev& ed, WarpEnt* tWarp, int n_threads) {
  for (int wi = threadIdx.x; wi < ed.K * 22; wi += n_threads) {
    const int p = wi / 22, i = wi - p * 22, ori = i >= 11, ii = ori ? i - 11 : i;
    WarpEnt w{0.0f, 0.0f, 1.0f, 1.0f, 0.0f, 0.0f};
    if (ii == 0) {                                          // (x / res[1] - 0.5) * 2, (y / res[0] - 0.5) * 2
      w.lin = 1.0f;
      if (ori) w.cs = 2.0f * ed.inv_h; else w.sn = 2.0f * ed.inv_w;
    } else {
      const int o = (ii - 1) >> 1;
      w.cs = ed.cs[p][ori]; w.sn = ed.sn[p][ori];
      w.per = ed.per[p][ori][o]; w.inv_per = 1.0f / w.per;
      w.phase = ((ii - 1) & 1) ? 0.25f : 0.0f;
    }
    tWarp[wi] = w;
  }
}

}  // namespace npp
