// npp_mlp_train32.hip -- the backward half of the exact-fp32 fit (NPPNet(precision="fp32")): what loss.backward() does through
// models/networks.py:56-95 / :145-173 behind render()'s output activation (models/helpers.py:55-58), every contraction on
// v_mfma_f32_32x32x2_f32 with f32 operands -- the reference's own arithmetic type.  Two launches after npp_mlp_fwd32_train
// (npp_mlp_fwd32.hip), on the arrays of npp_layout.h "exact-fp32 TRAINING chain":
//
//   npp_mlp_bwd32    d pred -> d raw -> d z_p -> (K > 1: d f2 -> d z_s) -> d f1 -> d z_7 .. d z_0    the data gradients, ONE launch:
//                    the chain of npp_light.hip's light_bwd_kernel for the D = 8 skip-connected net (a 64-row tile per workgroup,
//                    GEMMs transposed, W^T streamed from a packed fp32 buffer as the A operand, the gradient of the layer above in
//                    one LDS region [feature][64 rows] as the B operand); no gradient into the embedding.
//   npp_mlp_wgrad32  d W_l = d z_l^T x_l, d b_l = sum over rows of d z_l, for every layer in one grouped launch: 64 x 64 output tiles,
//                    32-row chunks of both operands staged through LDS (the scheme of npp_linear.hip).  The layer input x_l is formed
//                    while it is staged: snake(z) of the stashed pre-activation, or sin(f v + phase) of a stashed warped coordinate.
//
// Fixed-order sums: the rows of a batch are dealt to the ksplit slabs by a fixed rule (row tile t of T belongs to slab s with
// s T / ksplit <= t < (s + 1) T / ksplit), ONE workgroup owns an (output tile, slab) pair, walks its rows in order and is the only writer
// of that part of the slab -- zeros included, so a slab without rows holds zeros.  No float atomics anywhere: two runs give the same
// bits, and npp_adam_step_net / npp_grad_reduce add the slabs in slab order.
#include "npp_chain32.h"
#include "npp_coord.h"

namespace npp {

constexpr int kTB32 = 32 * kNT;                    // threads of the backward chain: 2 feature tiles per wave
constexpr int kRegionB32 = kW * kRowTile * 4;
constexpr int kSmemB32 = kRegionB32 + 4 * kRowTile * 4;

struct Bwd32Args {
  const float* dpred; const float* pred; int64_t Bp;
  const float* wb;           // transposed fp32 pack (npp_layout.h BDesc32)
  const float* params;
  const float* stash;
  float* dz;
  int32_t out_act;
};

// epilogue of a data-gradient step: d h (acc) -> d z = d h * snake'(z) (z from the stash; DERIV false: d z = d h) -> gradient rows
// drow0 + feature (+ the region, the next step's B operand).  Not merged with npp_light.hip's light_bepi: the two spell the
// region address differently, light_bwd_kernel<1> spills in this spelling and this kernel ran 1.8 % slower at K = 3 in that one,
// with 6 % fewer instructions (profiles/chain32_resource_usage.txt)
template <bool DERIV>
__device__ __forceinline__ void bepi32(f32x16 (&acc)[2][kNB], char* region, const float* __restrict__ zT, float* __restrict__ dT, int64_t Bp,
                                       int64_t row0, int nt0, int b, int h) {
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt) {
      const int f0 = (nt0 + nt) * 32 + 4 * h;
      const int64_t g = (int64_t)f0 * Bp + row0 + bt * 32 + b;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int fo = (r & 3) + 8 * (r >> 2);
        float dv = acc[nt][bt][r];
        if (DERIV) dv *= snake_deriv32(zT[g + (int64_t)fo * Bp]);
        dT[g + (int64_t)fo * Bp] = dv;
        if (region) *(float*)(region + ((f0 + fo) * kRowTile + bt * 32 + b) * 4) = dv;
      }
    }
}

template <bool MULTI>
__global__ __launch_bounds__(kTB32, 2) void mlp_bwd32_kernel(Bwd32Args a, NetDesc d, BDesc32 bd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* R = smem;
  float* sD = (float*)(smem + kRegionB32);         // d raw [64 rows][3]
  const int tid = threadIdx.x, lane = tid & 63, b = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t Bp = a.Bp, row0 = (int64_t)blockIdx.x * kRowTile;
  const float* P = a.params;
  const float* S = a.stash;
  float* D = a.dz;
  const int nt0 = 2 * wave;
  // d raw = d pred * act'(pred) (models/helpers.py:55-58: sigmoid / tanh from their outputs): kept in LDS and as rows of the gradient array
  if (tid < kRowTile * 3) {
    const int64_t g = row0 * 3 + tid;
    const float p = a.pred[g];
    const float da = a.out_act == 1 ? p * (1.0f - p) : (a.out_act == 2 ? 1.0f - p * p : 1.0f);
    const float dv = a.dpred[g] * da;
    sD[tid] = dv;
    D[(int64_t)(kD32Raw + tid % 3) * Bp + row0 + tid / 3] = dv;
  }
  wg_barrier();
  // d a_p = d raw W_rgb; d z_p = d a_p * snake'(z_p) -> region features 0 .. W / 2 - 1 + gradient rows
  {
    const float* Wr = P + d.w_off[LRGB];
    float* Rf = (float*)R;
    for (int i = tid; i < (kW / 2) * kRowTile; i += kTB32) {
      const int k = i / kRowTile, row = i % kRowTile;
      float dv = sD[row * 3] * Wr[k];
      dv = fmaf(sD[row * 3 + 1], Wr[kW / 2 + k], dv);
      dv = fmaf(sD[row * 3 + 2], Wr[kW + k], dv);
      const int64_t g = (int64_t)(kS32ZP + k) * Bp + row0 + row;
      dv *= snake_deriv32(S[g]);
      D[g] = dv;
      Rf[k * kRowTile + row] = dv;
    }
  }
  wg_barrier();
  const wrsrc_t rsrc = make_wrsrc(a.wb, bd.total16);
  const ActSrc32 act{R + ((4 * h) * kRowTile + b) * 4};
  auto wb = [&](int v) -> uint32_t { return (uint32_t)bd.off16[v]; };
  constexpr int GA = kW / 8, GP = kW / 16;         // k-step groups of a contraction over W / over W / 2 output neurons
  f32x16 df1[2][kNB], acc[2][kNB];
  // d f1 = W_p[:, :W]^T d z_p (+ W_s[:, :W]^T d z_s when K > 1)
  zero32(df1);
  part32<2, kNT>(df1, rsrc, wb(BP1), GP, nt0, lane, act);
  if (MULTI) {
    zero32(acc);
    part32<2, kNT>(acc, rsrc, wb(BP2), GP, nt0, lane, act);                 // d f2 = W_p[:, W:]^T d z_p  (feature_linear2 is linear)
    wg_barrier();
    bepi32<false>(acc, R, nullptr, D + (int64_t)kS32F2 * Bp, Bp, row0, nt0, b, h);
    wg_barrier();
    zero32(acc);
    part32<2, kNT>(acc, rsrc, wb(BF2), GA, nt0, lane, act);                 // d a_s = W_f2^T d f2
    wg_barrier();
    bepi32<true>(acc, R, S + (int64_t)kS32ZS * Bp, D + (int64_t)kS32ZS * Bp, Bp, row0, nt0, b, h);
    wg_barrier();
    part32<2, kNT>(df1, rsrc, wb(BS), GA, nt0, lane, act);
  }
  wg_barrier();
  bepi32<false>(df1, R, nullptr, D + (int64_t)kS32F1 * Bp, Bp, row0, nt0, b, h);
  wg_barrier();
  // d z_7 = (W_f1^T d f1) * snake'(z_7), d z_6 = (W_7^T d z_7) * snake'(z_6), ..., d z_4 through the h columns of layer 5 (the skip's
  // embedding columns get no gradient), ..., d z_0
#pragma unroll 1
  for (int j = 0; j < 8; ++j) {
    const int l = 7 - j;
    zero32(acc);
    part32<2, kNT>(acc, rsrc, wb(BF1 + j), GA, nt0, lane, act);
    wg_barrier();
    bepi32<true>(acc, l > 0 ? R : nullptr, S + (int64_t)l * kW * Bp, D + (int64_t)l * kW * Bp, Bp, row0, nt0, b, h);
    wg_barrier();
  }
}

__global__ void pack32_bwd_kernel(const float* __restrict__ P, float* __restrict__ out, NetDesc d, BDesc32 bd) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= bd.total16) return;
  int v = 0;
  for (int q = 0; q < kNumBwd; ++q)
    if (bd.present[q] && u >= bd.off16[q]) v = q;
  const int64_t r = u - bd.off16[v];
  const int lane = (int)(r & 63), nt = (int)((r >> 6) % kNT), g = (int)((r >> 6) / kNT);
  const int l = bd.layer[v], m = bd.col0[v] + nt * 32 + (lane & 31), h = lane >> 5;
  f32x4_t o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 8 * g + e + 4 * h;
    o[e] = k < d.n_out[l] ? P[d.w_off[l] + (int64_t)k * d.n_in[l] + m] : 0.0f;
  }
  ((f32x4_t*)out)[u] = o;
}

// ---- weight gradients -------------------------------------------------------------------------------------------------------
// A layer's input columns come from up to two sources (cat of models/networks.py:71,76,85): stash rows (plain, or snake() of a stashed
// pre-activation) or the embedding of proposals p0.. (462 columns each, formed from the stashed warped coordinates).
struct Wg32Seg { int32_t emb, row0, snake; };      // emb: row0 = first proposal; else row0 = first stash row
struct Wg32Layer {
  int32_t dz_row, n_out, n_in, gx, gy, first_wg, split;      // columns < split: seg[0], the others seg[1]
  Wg32Seg seg[2];
  int64_t w_off, b_off;
};
struct Wg32Args {
  const float* dz; const float* stash; float* gslabs;
  int64_t Bp, slab_stride, total;
  int32_t ksplit, n_layers;
  float fr[NPP_N_FREQ];      // freq / 2 pi (EmbedDev.freq_rev)
  Wg32Layer L[kNumLayers];
};

// operand tile in LDS as in npp_linear.hip: k-pairs interleaved, s[k >> 1][m][k & 1], 66 pairs per row (conflict-free both ways)
constexpr int kWgLdp = 66;
constexpr int kWgTile = 16 * kWgLdp * 2;

// what one thread stages of an operand per 32-row chunk: two runs of 4 consecutive rows of feature (tid >> 3) + 32 r
struct Wg32Run { const float* p; int32_t kind; float f, ph; };      // kind 0 zero, 1 plain, 2 snake(x), 3 sin(f x + ph) (hardware sine, revolutions)
__device__ __forceinline__ float wg32_val(const Wg32Run& r, float x) {
  if (r.kind == 2) return snake_fast(x);
  if (r.kind == 3) return __builtin_amdgcn_sinf(fmaf(x, r.f, r.ph));          // == EmbSrc32::frag of the forward
  return r.kind ? x : 0.0f;
}
__device__ __forceinline__ void wg32_sstore(float* __restrict__ S, int tid, const Wg32Run (&run)[2], const f32x4_t (&reg)[2]) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int m = (tid >> 3) + 32 * r, kp = 2 * (tid & 7);
    *(f32x2_t*)(S + ((kp + 0) * kWgLdp + m) * 2) = f32x2_t{wg32_val(run[r], reg[r][0]), wg32_val(run[r], reg[r][1])};
    *(f32x2_t*)(S + ((kp + 1) * kWgLdp + m) * 2) = f32x2_t{wg32_val(run[r], reg[r][2]), wg32_val(run[r], reg[r][3])};
  }
}

__global__ __launch_bounds__(256) void mlp_wgrad32_kernel(Wg32Args a) {
  __shared__ __attribute__((aligned(16))) float sA[kWgTile];
  __shared__ __attribute__((aligned(16))) float sB[kWgTile];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, kh = lane >> 5, wm = wave >> 1, wn = wave & 1;
  int li = 0;
  for (int q = 1; q < a.n_layers; ++q) if ((int)blockIdx.x >= a.L[q].first_wg) li = q;
  const Wg32Layer& Ld = a.L[li];
  const int local = (int)blockIdx.x - Ld.first_wg, bx = local % Ld.gx, by = local / Ld.gx;
  const int m0 = by * 64, n0 = bx * 64, s = (int)blockIdx.y;
  const int64_t Bp = a.Bp, T = Bp / kRowTile;
  const int64_t kbeg = (s * T / a.ksplit) * kRowTile, kend = ((s + 1) * T / a.ksplit) * kRowTile;      // this slab's rows (fixed rule)
  float* slab = a.gslabs + (int64_t)s * a.slab_stride;
  if (blockIdx.x == 0 && a.total + tid < a.slab_stride) slab[a.total + tid] = 0.0f;                    // the stride's padding floats
  // this thread's two runs of each operand (fixed over the chunks)
  Wg32Run ra[2], rb[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int f = (tid >> 3) + 32 * r, k4 = 4 * (tid & 7);
    const int m = m0 + f, n = n0 + f;
    ra[r] = Wg32Run{a.dz + (int64_t)(Ld.dz_row + min(m, Ld.n_out - 1)) * Bp + k4, m < Ld.n_out ? 1 : 0, 0.0f, 0.0f};
    Wg32Run q{a.stash + k4, 0, 0.0f, 0.0f};
    if (n < Ld.n_in) {
      const int sg = n >= Ld.split;
      const int c = n - (sg ? Ld.split : 0);
      const Wg32Seg seg = Ld.seg[sg];
      if (!seg.emb) {
        q.p += (int64_t)(seg.row0 + c) * Bp;
        q.kind = seg.snake ? 2 : 1;
      } else {                                     // reference column c % 462 of proposal row0 + c / 462 (models/embedder.py:41-44,56)
        const int p = seg.row0 + c / kE, cc = c % kE, blk = cc / 22, i = cc - 22 * blk;
        q.p += (int64_t)(kS32V + 22 * p + i) * Bp;
        if (blk == 0) q.kind = 1;
        else { q.kind = 3; q.f = a.fr[(blk - 1) >> 1]; q.ph = ((blk - 1) & 1) ? 0.25f : 0.0f; }
      }
    }
    rb[r] = q;
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const bool do_rowsum = bx == 0 && tid < 64;
  float rs = 0.0f;
  f32x4_t va[2], vb[2];
  const int nchunk = (int)((kend - kbeg) / 32);
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      va[r] = *(const f32x4_t*)(ra[r].p + k0);
      vb[r] = *(const f32x4_t*)(rb[r].p + k0);
    }
  };
  if (nchunk > 0) gload(kbeg);
  const float* __restrict__ fa = sA + (wm * 32 + l31) * 2 + kh;
  const float* __restrict__ fb = sB + (wn * 32 + l31) * 2 + kh;
  for (int c = 0; c < nchunk; ++c) {
    wg32_sstore(sA, tid, ra, va);
    wg32_sstore(sB, tid, rb, vb);
    wg_barrier();
    if (c + 1 < nchunk) gload(kbeg + 32 * (int64_t)(c + 1));
    if (do_rowsum) {
      const float* q = sA + tid * 2;
#pragma unroll
      for (int kp = 0; kp < 16; ++kp) rs += q[kp * kWgLdp * 2] + q[kp * kWgLdp * 2 + 1];
    }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) acc = mfma32(fa[ks * kWgLdp * 2], fb[ks * kWgLdp * 2], acc);
    wg_barrier();
  }
  if (do_rowsum && m0 + tid < Ld.n_out) slab[Ld.b_off + m0 + tid] = rs;
  const int n = n0 + wn * 32 + l31;
  if (n >= Ld.n_in) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + acc_row(r, kh);
    if (m < Ld.n_out) slab[Ld.w_off + (int64_t)m * Ld.n_in + n] = acc[r];
  }
}

static Wg32Args wgrad32_args(int K) {
  const NetDesc d = make_desc(K);
  Wg32Args a{};
  int n = 0, wg = 0;
  for (int l = 0; l < kNumLayers; ++l) {
    if (!d.present[l]) continue;
    Wg32Layer& L = a.L[n++];
    L.n_out = d.n_out[l]; L.n_in = d.n_in[l]; L.w_off = d.w_off[l]; L.b_off = d.b_off[l];
    L.split = L.n_in;
    const Wg32Seg prev{0, (l - 1) * kW, 1};        // snake(z) of the layer below
    switch (l) {
      case L0: L.dz_row = 0; L.seg[0] = Wg32Seg{1, 0, 0}; break;
      case L5: L.dz_row = L5 * kW; L.seg[0] = Wg32Seg{1, 0, 0}; L.split = kE; L.seg[1] = prev; break;
      case LF1: L.dz_row = kS32F1; L.seg[0] = Wg32Seg{0, L7 * kW, 1}; break;
      case LS: L.dz_row = kS32ZS; L.seg[0] = Wg32Seg{0, kS32F1, 0}; L.split = kW; L.seg[1] = Wg32Seg{1, 1, 0}; break;
      case LF2: L.dz_row = kS32F2; L.seg[0] = Wg32Seg{0, kS32ZS, 1}; break;
      case LP: L.dz_row = kS32ZP; L.seg[0] = Wg32Seg{0, kS32F1, 0}; L.split = kW; L.seg[1] = Wg32Seg{0, kS32F2, 0}; break;
      case LRGB: L.dz_row = kD32Raw; L.seg[0] = Wg32Seg{0, kS32ZP, 1}; break;
      default: L.dz_row = l * kW; L.seg[0] = prev; break;          // L1..L4, L6, L7
    }
    L.gx = (L.n_in + 63) / 64; L.gy = (L.n_out + 63) / 64; L.first_wg = wg;
    wg += L.gx * L.gy;
  }
  a.n_layers = n;
  a.total = d.total_params;
  a.slab_stride = slab_stride_of(d.total_params);
  a.ksplit = wg;             // (the caller replaces it: carries the workgroup count out)
  return a;
}

}  // namespace npp

using namespace npp;

extern "C" int npp_train_workspace32(int K, int width, int64_t Bp, int ksplit, int64_t sizes[4]) {
  if (K < 1 || K > NPP_MAX_K || width != NPP_WIDTH) { set_error("npp_train_workspace32: K=%d width=%d (build is %d)", K, width, NPP_WIDTH); return NPP_ERR_UNSUPPORTED; }
  if (Bp <= 0 || Bp % kRowTile || ksplit < 1 || !sizes) { set_error("npp_train_workspace32: bad Bp/ksplit"); return NPP_ERR_ARG; }
  sizes[0] = 0;
  sizes[1] = (int64_t)stash32_rows(K) * Bp * 4;
  sizes[2] = (int64_t)kD32Rows * Bp * 4;
  sizes[3] = (int64_t)ksplit * slab_stride_of(make_desc(K).total_params) * 4;
  return NPP_OK;
}

extern "C" int64_t npp_pack32_bwd_bytes(int K, int width) {
  if (K < 1 || K > NPP_MAX_K || width != NPP_WIDTH) { set_error("npp_pack32_bwd_bytes: K=%d width=%d", K, width); return -1; }
  return make_bdesc32(K).total16 * 16;
}

extern "C" int npp_pack_weights32_bwd(const float* d_params, void* d_w32_bwd, int K, int width, void* stream) {
  if (K < 1 || K > NPP_MAX_K || width != NPP_WIDTH || !d_params || !d_w32_bwd) { set_error("npp_pack_weights32_bwd: bad argument"); return NPP_ERR_ARG; }
  const BDesc32 bd = make_bdesc32(K);
  hipLaunchKernelGGL(pack32_bwd_kernel, dim3((unsigned)((bd.total16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_params,
                     (float*)d_w32_bwd, make_desc(K), bd);
  return check_launch("npp_pack_weights32_bwd");
}

extern "C" int npp_mlp_bwd32(const float* d_dpred, const float* d_pred, int64_t Bp, int K, int width, const void* d_w32_bwd,
                             const float* d_params, const void* d_stash, void* d_dz, int out_act, void* stream) {
  const char* who = "npp_mlp_bwd32";
  if (K < 1 || K > NPP_MAX_K || width != NPP_WIDTH) { set_error("%s: K=%d width=%d (build is %d)", who, K, width, NPP_WIDTH); return NPP_ERR_UNSUPPORTED; }
  if (Bp <= 0 || Bp % kRowTile || Bp / kRowTile > 0x7fffffffLL) { set_error("%s: Bp=%lld must be a positive multiple of %d", who, (long long)Bp, kRowTile); return NPP_ERR_ARG; }
  if (!d_dpred || !d_pred || !d_w32_bwd || !d_params || !d_stash || !d_dz || out_act < 0 || out_act > 2) { set_error("%s: bad argument", who); return NPP_ERR_ARG; }
  Bwd32Args a{d_dpred, d_pred, Bp, (const float*)d_w32_bwd, d_params, (const float*)d_stash, (float*)d_dz, out_act};
  const dim3 grid((unsigned)(Bp / kRowTile)), block(kTB32);
  const hipStream_t st = (hipStream_t)stream;
  return K > 1 ? launch_lds<mlp_bwd32_kernel<true>>(who, grid, block, kSmemB32, kSmemB32, st, a, make_desc(K), make_bdesc32(K))
               : launch_lds<mlp_bwd32_kernel<false>>(who, grid, block, kSmemB32, kSmemB32, st, a, make_desc(K), make_bdesc32(K));
}

extern "C" int npp_mlp_wgrad32(const void* d_dz, const void* d_stash, const npp_embed_cfg* cfg, int64_t Bp, int K, int width, int ksplit,
                               float* d_gslabs, void* stream) {
  const char* who = "npp_mlp_wgrad32";
  int rc = check_embed_cfg(cfg, who);
  if (rc) return rc;
  if (K != cfg->K || width != NPP_WIDTH) { set_error("%s: K=%d (cfg %d) width=%d (build is %d)", who, K, cfg->K, width, NPP_WIDTH); return NPP_ERR_UNSUPPORTED; }
  if (Bp <= 0 || Bp % kRowTile || ksplit < 1 || ksplit > 65535 || !d_dz || !d_stash || !d_gslabs) {
    set_error("%s: bad argument (Bp=%lld a positive multiple of %d, ksplit=%d in 1..65535)", who, (long long)Bp, kRowTile, ksplit);
    return NPP_ERR_ARG;
  }
  Wg32Args a = wgrad32_args(K);
  const int n_wg = a.ksplit;
  a.ksplit = ksplit;
  a.dz = (const float*)d_dz; a.stash = (const float*)d_stash; a.gslabs = d_gslabs; a.Bp = Bp;
  const EmbedDev e = make_embed_dev(*cfg);
  for (int j = 0; j < NPP_N_FREQ; ++j) a.fr[j] = e.freq_rev[j];
  hipLaunchKernelGGL(mlp_wgrad32_kernel, dim3((unsigned)n_wg, (unsigned)ksplit), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(who);
}
