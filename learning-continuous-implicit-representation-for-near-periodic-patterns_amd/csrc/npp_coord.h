// npp_coord.h -- how a row's position enters the forward kernels and how its colour leaves them (include/npp_hip.h "continuous
// coordinates"), with the host-side argument checks the entry points of those kernels share.  A new coordinate mode is one
// CoordMode value, one branch in row_coord and one in store_rgb, one entry point per chain and one table row in ops.render.
#pragma once
#include "npp_common.h"

namespace npp {

// ---- host side: embedder constants and argument checks (npp_embed.hip) ----------------------------------------------------------
EmbedDev make_embed_dev(const npp_embed_cfg& c);
int check_embed_cfg(const npp_embed_cfg* c, const char* who);
// The canvas half of a grid / view launch: pixels [start, start + n) of a canvas `width` wide.  NPP_OK also for n == 0.
int check_canvas(int64_t start, int64_t n, int32_t width, const char* who);
int check_grid(const npp_grid* g, const char* who);
int check_view(const npp_view* v, const char* who);

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
enum CoordMode { kCoordI32 = 0, kCoordF32 = 1, kCoordGrid = 2, kCoordView = 3 };

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
__host__ __device__ __forceinline__ uint8_t view_coord(const npp_view& v, int H, int W, int64_t p, float& y, float& x) {
  const int64_t i = p / v.width;
  const float fi = (float)i, fj = (float)(int32_t)(p - i * v.width);
  const float d = view_add(view_add(view_mul(v.m[6], fi), view_mul(v.m[7], fj)), v.m[8]);
  y = view_div(view_add(view_add(view_mul(v.m[0], fi), view_mul(v.m[1], fj)), v.m[2]), d);
  x = view_div(view_add(view_add(view_mul(v.m[3], fi), view_mul(v.m[4], fj)), v.m[5]), d);
  if (!(d > 0.0f && __builtin_isfinite(y) && __builtin_isfinite(x))) {
    y = x = 0.0f;
    return 0;
  }
  return y >= -0.5f && y < (float)H - 0.5f && x >= -0.5f && x < (float)W - 0.5f ? 3 : 1;
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

// (y, x) of row r in coordinate mode CM: int32 pixel indices (coords, (N, 2) [y, x]), fp32 positions (src.coordsf, the same shape),
// the implicit grid or the view.  Returns the inside byte of the position: a view's (0: not in view, y = x = 0), 3 in every other mode.
template <int CM>
__device__ __forceinline__ uint8_t row_coord(const int32_t* coords, const CoordSrc& src, int64_t r, float& y, float& x) {
  if (CM == kCoordView) return view_row(src.view, r, y, x);
  if (CM == kCoordGrid) {
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
// itself by the thread of channel 0; every other launch stores all its rows.
template <int CM>
__device__ __forceinline__ void store_rgb(const CoordSrc& src, float* pred, int64_t row, int c, float o) {
  if (CM == kCoordView) {
    if (row < src.view.v.n) {
      float y, x;
      const uint8_t in = view_coord(src.view.v, src.view.H, src.view.W, src.view.v.start + row, y, x);   // (row < n: view_row without its clamp)
      pred[row * 3 + c] = in ? o : 0.0f;
      if (c == 0 && src.view.inside) src.view.inside[row] = in;
    }
  } else if (CM != kCoordGrid || row < src.g.n) pred[row * 3 + c] = o;
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
