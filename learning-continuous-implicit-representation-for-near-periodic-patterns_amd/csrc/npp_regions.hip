// npp_regions.hip -- 4-connected components of an (H, W) int32 label image (0 = outside; two pixels are connected when they are
// 4-neighbours carrying the same non-zero value), their raster numbering and their per-component statistics: the per-pixel half of
// the SLIC connectivity repair (init_segment.enforce_connectivity) and of the final non-periodic mask (segment.segmentation_eval:
// hole filling, removal of small objects).  DESIGN.md 6h.
//
// The root of a pixel is the SMALLEST row-major index i W + j of its component (-1 outside): a pure function of the input, whatever
// the launch schedule.  npp_cc_label is three launches over ONE parent array, the output itself, with parent[i] <= i throughout:
//   1. every 16 x 16 tile is labelled in LDS by union-find and written out with its tile-local roots as global indices;
//   2. the pairs across tile borders are united in global memory.  Workgroups on different XCDs update the same parent array here,
//      so EVERY access to it in this launch is a device-scope atomic (a relaxed agent-scope load, or atomicMin, which is
//      device-scope); a plain load could be served from a stale line.  The loops are driven by the values the atomics return:
//      every chain strictly descends, so each terminates on its own, whatever another workgroup does or has yet to do;
//   3. every pixel walks to its root and stores it.  A store of this launch replaces an ancestor by a lower ancestor of the same
//      component, so a walk that meets it (or misses it) still ends at the one root.
// The launch boundaries make each phase's result visible to the next; there is no fence, no flag and no loop that waits for another
// workgroup.  Nothing is kept in device memory between launches; the sums of npp_cc_stats are integer atomics: bit-reproducible.
#include <climits>
#include <vector>
#include "npp_common.h"

namespace npp {

constexpr int kCcTile = 16;                              // tile side: one pixel per thread of a 256-thread workgroup
constexpr int kCcScanPix = 1024;                         // pixels per workgroup of the numbering launches (4 per thread)
constexpr int kCcMaxCh = 4;                              // channels npp_cc_stats sums

// ---- union of two nodes under "parent[i] <= i, the lower root wins" ------------------------------------------------------------
// a > b: old = min-exchange(parent[a], b).  old == a: a was a root and now hangs under b, done.  Otherwise old < a was a's parent,
// a now hangs under min(old, b), and old and b remain to be united: max(a, b) falls with every round.
__device__ __forceinline__ void cc_unite_lds(int* par, int a, int b) {
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) break;
    a = old;
  }
}
__device__ __forceinline__ int cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_find(const int32_t* par, int a) {               // strictly descending: at most a steps
  for (int p = cc_load(par + a); p != a; p = cc_load(par + a)) a = p;
  return a;
}
__device__ __forceinline__ void cc_unite(int32_t* par, int a, int b) {
  a = cc_find(par, a);
  b = cc_find(par, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);                                        // device scope
    if (old == a) break;
    a = old;
  }
}

// ---- launch 1: one tile per workgroup, union-find in LDS ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_tile_kernel(const int32_t* __restrict__ lab, int H, int W, int32_t* __restrict__ par) {
  __shared__ int s_lab[kCcTile * kCcTile];
  __shared__ int s_par[kCcTile * kCcTile];
  const int t = threadIdx.x, ly = t / kCcTile, lx = t - ly * kCcTile;
  const int y0 = blockIdx.y * kCcTile, x0 = blockIdx.x * kCcTile;
  const int y = y0 + ly, x = x0 + lx;
  const bool in = y < H && x < W;
  const int v = in ? lab[(int64_t)y * W + x] : 0;
  s_lab[t] = v;
  s_par[t] = t;
  __syncthreads();
  if (v != 0) {
    if (lx > 0 && s_lab[t - 1] == v) cc_unite_lds(s_par, t, t - 1);
    if (ly > 0 && s_lab[t - kCcTile] == v) cc_unite_lds(s_par, t, t - kCcTile);
  }
  __syncthreads();
  if (!in) return;
  int r = t;
  for (int p = s_par[r]; p != r; p = s_par[r]) r = p;                             // nothing changes any more; strictly descending
  const int ry = r / kCcTile, rx = r - ry * kCcTile;
  par[(int64_t)y * W + x] = v != 0 ? (y0 + ry) * W + (x0 + rx) : -1;             // H W < 2^31
}

// ---- launch 2: the pairs across tile borders ------------------------------------------------------------------------------------
// Thread e < n_v H: pixel (e mod H) of the e / H-th vertical border (column 16 (k + 1)) against its left neighbour; the others:
// a pixel of a horizontal border (row 16 (k + 1)) against the one above it.
__global__ __launch_bounds__(256) void cc_border_kernel(const int32_t* __restrict__ lab, int H, int W, int n_v, int n_h, int32_t* par) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nv = (int64_t)n_v * H;
  int y, x, q;
  if (e < nv) {
    const int k = (int)(e / H);
    y = (int)(e - (int64_t)k * H);
    x = (k + 1) * kCcTile;
    q = y * W + x - 1;
  } else {
    const int64_t f = e - nv;
    if (f >= (int64_t)n_h * W) return;
    const int k = (int)(f / W);
    x = (int)(f - (int64_t)k * W);
    y = (k + 1) * kCcTile;
    q = (y - 1) * W + x;
  }
  const int p = y * W + x;
  const int v = lab[p];
  if (v != 0 && lab[q] == v) cc_unite(par, p, q);
}

// ---- launch 3: every pixel to its root ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_flatten_kernel(int64_t n, int32_t* par) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int a = cc_load(par + p);
  if (a < 0 || a == (int)p) return;
  par[p] = cc_find(par, a);
}

// ---- numbering: roots -> 1..C in ascending root order -------------------------------------------------------------------------
// A pixel is a root when root[p] == p.  count: roots per block of 1024 pixels; offsets: their exclusive prefix (one workgroup) and
// the total; rank: the exclusive rank of every root, stored at the root's own position of the scratch image; apply: a gather.
__device__ __forceinline__ int cc_block_excl_scan(int c, int* s_wave, int& total) {      // 256 threads; -> exclusive prefix of c
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  return base + inc - c;
}

__device__ __forceinline__ int cc_thread_flags(const int32_t* __restrict__ root, int64_t n, int64_t p0, bool (&f)[4]) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t p = p0 + k;
    f[k] = p < n && root[p] == (int32_t)p;
    c += f[k] ? 1 : 0;
  }
  return c;
}

__global__ __launch_bounds__(256) void cc_count_kernel(const int32_t* __restrict__ root, int64_t n, int32_t* __restrict__ block_sum) {
  __shared__ int s_wave[4];
  bool f[4];
  const int c = cc_thread_flags(root, n, (int64_t)blockIdx.x * kCcScanPix + threadIdx.x * 4, f);
  int total;
  cc_block_excl_scan(c, s_wave, total);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void cc_offsets_kernel(int32_t* __restrict__ block_sum, int nb, int32_t* __restrict__ count) {
  __shared__ int s_wave[4];
  const int per = (nb + 255) / 256;
  const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
  int c = 0;
  for (int b = b0; b < b1; ++b) c += block_sum[b];
  int total;
  int run = cc_block_excl_scan(c, s_wave, total);
  for (int b = b0; b < b1; ++b) {
    const int v = block_sum[b];
    block_sum[b] = run;
    run += v;
  }
  if (threadIdx.x == 0) count[0] = total;
}

__global__ __launch_bounds__(256) void cc_rank_kernel(const int32_t* __restrict__ root, int64_t n, const int32_t* __restrict__ block_off,
                                                      int32_t* __restrict__ rank) {
  __shared__ int s_wave[4];
  bool f[4];
  const int64_t p0 = (int64_t)blockIdx.x * kCcScanPix + threadIdx.x * 4;
  const int c = cc_thread_flags(root, n, p0, f);
  int total;
  int r = block_off[blockIdx.x] + cc_block_excl_scan(c, s_wave, total);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f[k]) rank[p0 + k] = r++;
}

__global__ __launch_bounds__(256) void cc_apply_kernel(const int32_t* root, int64_t n, const int32_t* __restrict__ rank, int32_t* numbered) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int r = root[p];
  numbered[p] = (r >= 0 && r < n) ? rank[r] + 1 : 0;
}

// ---- per-component statistics --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_stats_init_kernel(int C, int nch, int64_t* __restrict__ size, int64_t* __restrict__ sums,
                                                            int32_t* __restrict__ box) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  size[c] = 0;
  for (int k = 0; k < nch; ++k) sums[(int64_t)c * nch + k] = 0;
  box[(int64_t)c * 4 + 0] = INT_MAX;
  box[(int64_t)c * 4 + 1] = INT_MAX;
  box[(int64_t)c * 4 + 2] = -1;
  box[(int64_t)c * 4 + 3] = -1;
}

// One pixel per thread, 64 consecutive pixels per wave.  The wave is peeled by number, up to kCcPeel times: the number of its first
// pixel still to do is taken, the pixels carrying it are reduced across the wave and added once, from that lane (the inside of a
// large component: one round, one set of atomics per wave instead of 64 on the same words); what is left after the rounds adds per
// lane.  Integer atomics: any order gives the same bits.
constexpr int kCcPeel = 4;
__device__ __forceinline__ void cc_stats_add(int c, int nch, unsigned cnt, const unsigned (&v)[kCcMaxCh], int y0, int x0, int y1, int x1,
                                             int64_t* size, int64_t* sums, int32_t* box) {
  atomicAdd((unsigned long long*)&size[c], (unsigned long long)cnt);
  for (int k = 0; k < nch; ++k) atomicAdd((unsigned long long*)&sums[(int64_t)c * nch + k], (unsigned long long)v[k]);
  atomicMin(&box[(int64_t)c * 4 + 0], y0);
  atomicMin(&box[(int64_t)c * 4 + 1], x0);
  atomicMax(&box[(int64_t)c * 4 + 2], y1);
  atomicMax(&box[(int64_t)c * 4 + 3], x1);
}

__global__ __launch_bounds__(256) void cc_stats_kernel(const int32_t* __restrict__ numbered, int H, int W, int C,
                                                       const uint8_t* __restrict__ values, int nch, int64_t* size, int64_t* sums, int32_t* box) {
  const int64_t n = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int l = p < n ? numbered[p] : 0;
  if (l < 1 || l > C) l = 0;                                                      // outside, or not a number of this image: skipped
  const int y = p < n ? (int)(p / W) : 0, x = p < n ? (int)(p - (int64_t)y * W) : 0;
  unsigned v[kCcMaxCh] = {0, 0, 0, 0};
  if (l)
    for (int k = 0; k < nch; ++k) v[k] = values[p * nch + k];
  bool todo = l != 0;
  for (int round = 0; round < kCcPeel; ++round) {                                  // every lane of the wave takes every round
    const unsigned long long act = __ballot(todo);
    if (act == 0) return;                                                         // wave-uniform
    const int leader = __ffsll((long long)act) - 1;
    const int cur = __shfl(l, leader, 64);
    const bool mine = todo && l == cur;
    unsigned cnt = mine ? 1u : 0u, s[kCcMaxCh];
    int y0 = mine ? y : INT_MAX, x0 = mine ? x : INT_MAX, y1 = mine ? y : -1, x1 = mine ? x : -1;
#pragma unroll
    for (int k = 0; k < kCcMaxCh; ++k) s[k] = mine ? v[k] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
      for (int k = 0; k < kCcMaxCh; ++k) s[k] += __shfl_xor(s[k], off, 64);
      y0 = min(y0, __shfl_xor(y0, off, 64));
      x0 = min(x0, __shfl_xor(x0, off, 64));
      y1 = max(y1, __shfl_xor(y1, off, 64));
      x1 = max(x1, __shfl_xor(x1, off, 64));
    }
    if (lane == leader) cc_stats_add(cur - 1, nch, cnt, s, y0, x0, y1, x1, size, sums, box);
    todo = todo && !mine;
  }
  if (todo) cc_stats_add(l - 1, nch, 1u, v, y, x, y, x, size, sums, box);
}

// a component touches the image border exactly when its bounding box does
__host__ __device__ inline uint8_t cc_box_on_border(const int32_t* b, int H, int W) {
  return (b[2] >= b[0] && (b[0] == 0 || b[1] == 0 || b[2] == H - 1 || b[3] == W - 1)) ? 1 : 0;
}
__global__ __launch_bounds__(256) void cc_border_flag_kernel(int C, int H, int W, const int32_t* __restrict__ box, uint8_t* __restrict__ border) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) border[c] = cc_box_on_border(box + (int64_t)c * 4, H, W);
}

static bool cc_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31); }
static unsigned cc_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
static int64_t cc_scan_blocks(int H, int W) { return ((int64_t)H * W + kCcScanPix - 1) / kCcScanPix; }
static int64_t cc_number_bytes(int H, int W) { return ((int64_t)H * W + cc_scan_blocks(H, W)) * 4; }

// ---- host twins ---------------------------------------------------------------------------------------------------------------
static int cc_host_find(int32_t* par, int a) {
  while (par[a] != a) {                                                           // path halving: parent[i] <= i is kept
    par[a] = par[par[a]];
    a = par[a];
  }
  return a;
}
static void cc_host_unite(int32_t* par, int a, int b) {
  a = cc_host_find(par, a);
  b = cc_host_find(par, b);
  if (a < b) par[b] = a;
  else par[a] = b;
}

}  // namespace npp

using namespace npp;

extern "C" int npp_cc_label(const int32_t* d_labels_hw, int H, int W, int32_t* d_root_hw, void* stream) {
  if (!d_labels_hw || !d_root_hw || !cc_shape_ok(H, W) || (const void*)d_labels_hw == (const void*)d_root_hw ||
      (H + kCcTile - 1) / kCcTile > 65535) {
    set_error("npp_cc_label: bad argument (H=%d W=%d, both >= 1, H W < 2^31, H <= %d; the roots need an array of their own)", H, W,
              65535 * kCcTile);
    return NPP_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  const dim3 tiles((unsigned)((W + kCcTile - 1) / kCcTile), (unsigned)((H + kCcTile - 1) / kCcTile));
  hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, s, d_labels_hw, H, W, d_root_hw);
  const int n_v = (W - 1) / kCcTile, n_h = (H - 1) / kCcTile;
  const int64_t pairs = (int64_t)n_v * H + (int64_t)n_h * W;
  if (pairs > 0) hipLaunchKernelGGL(cc_border_kernel, dim3(cc_blocks(pairs, 256)), dim3(256), 0, s, d_labels_hw, H, W, n_v, n_h, d_root_hw);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(n, 256)), dim3(256), 0, s, n, d_root_hw);
  return check_launch("npp_cc_label");
}

extern "C" int64_t npp_cc_number_scratch_bytes(int H, int W) {
  if (!cc_shape_ok(H, W)) {
    set_error("npp_cc_number_scratch_bytes: bad argument (H=%d W=%d, both >= 1, H W < 2^31)", H, W);
    return NPP_ERR_ARG;
  }
  return cc_number_bytes(H, W);
}

extern "C" int npp_cc_number(const int32_t* d_root_hw, int H, int W, int32_t* d_numbered_hw, int32_t* d_count, void* d_scratch,
                             int64_t scratch_bytes, void* stream) {
  if (!d_root_hw || !d_numbered_hw || !d_count || !d_scratch || !cc_shape_ok(H, W) || scratch_bytes < cc_number_bytes(H, W) ||
      ((uintptr_t)d_scratch & 3)) {
    set_error("npp_cc_number: bad argument (H=%d W=%d, both >= 1, H W < 2^31; scratch %lld bytes, 4-byte aligned, needs "
              "npp_cc_number_scratch_bytes = %lld)", H, W, (long long)scratch_bytes, cc_shape_ok(H, W) ? (long long)cc_number_bytes(H, W) : -1ll);
    return NPP_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  const int nb = (int)cc_scan_blocks(H, W);
  int32_t* rank = (int32_t*)d_scratch;
  int32_t* block_sum = rank + n;
  hipLaunchKernelGGL(cc_count_kernel, dim3(nb), dim3(256), 0, s, d_root_hw, n, block_sum);
  hipLaunchKernelGGL(cc_offsets_kernel, dim3(1), dim3(256), 0, s, block_sum, nb, d_count);
  hipLaunchKernelGGL(cc_rank_kernel, dim3(nb), dim3(256), 0, s, d_root_hw, n, (const int32_t*)block_sum, rank);
  hipLaunchKernelGGL(cc_apply_kernel, dim3(cc_blocks(n, 256)), dim3(256), 0, s, d_root_hw, n, (const int32_t*)rank, d_numbered_hw);
  return check_launch("npp_cc_number");
}

static bool cc_stats_args_ok(const char* who, const void* numbered, int H, int W, int C, const void* values, int nch, const void* size,
                             const void* sums, const void* border, const void* box) {
  if (numbered && cc_shape_ok(H, W) && C >= 0 && (int64_t)C <= (int64_t)H * W && nch >= 0 && nch <= kCcMaxCh && (nch == 0 || values) &&
      (C == 0 || (size && border && box && (nch == 0 || sums))))
    return true;
  set_error("%s: bad argument (H=%d W=%d, both >= 1, H W < 2^31; C=%d in 0..H W; nch=%d in 0..%d, with an image and sums when > 0)", who, H,
            W, C, nch, kCcMaxCh);
  return false;
}

extern "C" int npp_cc_stats(const int32_t* d_numbered_hw, int H, int W, int C, const uint8_t* d_values_hwc, int nch, int64_t* d_size_c,
                            int64_t* d_sums_cn, uint8_t* d_border_c, int32_t* d_box_c4, void* stream) {
  if (!cc_stats_args_ok("npp_cc_stats", d_numbered_hw, H, W, C, d_values_hwc, nch, d_size_c, d_sums_cn, d_border_c, d_box_c4)) return NPP_ERR_ARG;
  if (C == 0) return NPP_OK;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(cc_stats_init_kernel, dim3(cc_blocks(C, 256)), dim3(256), 0, s, C, nch, d_size_c, d_sums_cn, d_box_c4);
  hipLaunchKernelGGL(cc_stats_kernel, dim3(cc_blocks(n, 256)), dim3(256), 0, s, d_numbered_hw, H, W, C, d_values_hwc, nch, d_size_c, d_sums_cn,
                     d_box_c4);
  hipLaunchKernelGGL(cc_border_flag_kernel, dim3(cc_blocks(C, 256)), dim3(256), 0, s, C, H, W, (const int32_t*)d_box_c4, d_border_c);
  return check_launch("npp_cc_stats");
}

// ---- the same definitions in plain C++ (host memory, no GPU) --------------------------------------------------------------------
extern "C" int npp_cc_label_host(const int32_t* labels_hw, int H, int W, int32_t* root_hw) {
  if (!labels_hw || !root_hw || !cc_shape_ok(H, W) || (const void*)labels_hw == (const void*)root_hw) {
    set_error("npp_cc_label_host: bad argument (H=%d W=%d, both >= 1, H W < 2^31; the roots need an array of their own)", H, W);
    return NPP_ERR_ARG;
  }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int p = y * W + x, v = labels_hw[p];
      root_hw[p] = v != 0 ? p : -1;
      if (v == 0) continue;
      if (x > 0 && labels_hw[p - 1] == v) cc_host_unite(root_hw, p, p - 1);
      if (y > 0 && labels_hw[p - W] == v) cc_host_unite(root_hw, p, p - W);
    }
  const int64_t n = (int64_t)H * W;
  for (int64_t p = 0; p < n; ++p)                                                  // ascending: a parent is final before its children
    if (root_hw[p] >= 0) root_hw[p] = root_hw[root_hw[p]];
  return NPP_OK;
}

extern "C" int npp_cc_number_host(const int32_t* root_hw, int H, int W, int32_t* numbered_hw, int32_t* count) {
  if (!root_hw || !numbered_hw || !count || !cc_shape_ok(H, W)) {
    set_error("npp_cc_number_host: bad argument (H=%d W=%d, both >= 1, H W < 2^31)", H, W);
    return NPP_ERR_ARG;
  }
  const int64_t n = (int64_t)H * W;
  std::vector<int32_t> rank((size_t)n);
  int32_t c = 0;
  for (int64_t p = 0; p < n; ++p)
    if (root_hw[p] == (int32_t)p) rank[(size_t)p] = c++;
  for (int64_t p = 0; p < n; ++p) {
    const int32_t r = root_hw[p];
    numbered_hw[p] = (r >= 0 && r < n) ? rank[(size_t)r] + 1 : 0;
  }
  *count = c;
  return NPP_OK;
}

extern "C" int npp_cc_stats_host(const int32_t* numbered_hw, int H, int W, int C, const uint8_t* values_hwc, int nch, int64_t* size_c,
                                 int64_t* sums_cn, uint8_t* border_c, int32_t* box_c4) {
  if (!cc_stats_args_ok("npp_cc_stats_host", numbered_hw, H, W, C, values_hwc, nch, size_c, sums_cn, border_c, box_c4)) return NPP_ERR_ARG;
  for (int c = 0; c < C; ++c) {
    size_c[c] = 0;
    for (int k = 0; k < nch; ++k) sums_cn[(int64_t)c * nch + k] = 0;
    int32_t* b = box_c4 + (int64_t)c * 4;
    b[0] = b[1] = INT_MAX;
    b[2] = b[3] = -1;
  }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int64_t p = (int64_t)y * W + x;
      const int l = numbered_hw[p];
      if (l < 1 || l > C) continue;
      const int c = l - 1;
      size_c[c] += 1;
      for (int k = 0; k < nch; ++k) sums_cn[(int64_t)c * nch + k] += values_hwc[p * nch + k];
      int32_t* b = box_c4 + (int64_t)c * 4;
      b[0] = y < b[0] ? y : b[0];
      b[1] = x < b[1] ? x : b[1];
      b[2] = y > b[2] ? y : b[2];
      b[3] = x > b[3] ? x : b[3];
    }
  for (int c = 0; c < C; ++c) border_c[c] = cc_box_on_border(box_c4 + (int64_t)c * 4, H, W);
  return NPP_OK;
}
