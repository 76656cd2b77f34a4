// npp_mlp_fwd32.hip -- the fused embedder + coordinate-MLP forward in EXACT fp32 (BASELINE config c4: "1024 x 1024 ...
// full-resolution coord grid, fp32").  Same function as npp_mlp_fwd.hip (models/embedder.py:102-148 + :11-56,
// models/networks.py:56-95 / :145-173, models/helpers.py:55-56), same fused structure, but every contraction runs on
// v_mfma_f32_32x32x2_f32: f32 operands, f32 accumulate, bit for bit a k-ordered fmaf chain (157 TFLOP/s peak, 1/16 of the bf16
// rate) -- the reference's own arithmetic type, no bf16 rounding anywhere.  The render of train.py:270-331, and -- with STASH -- the
// forward of the exact-fp32 fit (NPPNet(precision="fp32")): the same kernel also leaves the fp32 stash (npp_layout.h "exact-fp32
// TRAINING chain") that npp_mlp_bwd32 / npp_mlp_wgrad32 (npp_mlp_train32.hip) read; the stores touch no arithmetic, so the prediction
// of a stashing launch equals the render's bit for bit.  The default fit keeps the bf16 chain (BASELINE c2).
//
// Structure: one 256-thread workgroup = 64 pixel rows (two 32-column batch tiles), GEMMs transposed (Z^T = W X^T): the
// weights are the A operand (lane l: W[32 nt + (l & 31)][k-step's feature l >> 5]), streamed from L2 as 16-byte loads that
// carry FOUR consecutive k-steps each; the activations are the B operand (lane l: X[feature l >> 5][row l & 31]).  A 32 x 32
// accumulator tile holds feature acc_row(r, h) of row (lane & 31) in register r of lane half h, so register r of a tile IS
// the B operand of the k-step that contracts features (acc_row(r, 0), acc_row(r, 1)) = (n, n + 4): hidden activations cross
// LDS as plain fp32 [feature][64 rows] (one region, written in place behind a barrier), read back with one conflict-free
// ds_read_b32 per k-step and batch tile.  The 462 Fourier features of a proposal are never materialised: a k-step
// contracts (sin(f v_i), cos(f v_i)) -- lane half 0 / 1, one v_sin each -- and every wave generates its own B operands in
// registers right before the MFMAs that consume them (4 x redundant vector work that hides under the 64-cycle MFMAs, and no
// LDS ring, no barrier inside an embedding pass): 231 k-steps per proposal, no padding slots.
//
// Algorithmic work: 2 * ((K+1)*462*256 + 11*256^2 + 384) FLOP per row.
#include "npp_chain32.h"
#include "npp_coord.h"

namespace npp {

constexpr int kT32 = 32 * kNT;                     // threads: 2 neuron tiles per wave (4 waves at W = 256, 8 at W = 512)
constexpr int kRegion32 = kW * kRowTile * 4;       // 64 KiB: 256 features x 64 rows fp32
constexpr int kSmem32 = kRegion32 + 22 * kRowTile * 4 + 2 * kRowTile * 4 + ((sizeof(EmbedDev) + 15) / 16) * 16 +
                        NPP_MAX_K * 22 * (int)sizeof(WarpEnt);

struct Fwd32Args {
  const int32_t* coords;
  int64_t Bp;
  const float* w32;          // fp32 pack (npp_layout.h: Desc32)
  const float* params;
  float* pred;
  int32_t out_act;
  float* stash;              // STASH: (stash32_rows(K), Bp) fp32, feature-major
  CoordSrc src;              // render paths (CM != kCoordI32, inference only)
};

// B operands generated from the 22 warped coordinates of one proposal (sV[i][row], fp32): k-step q < 220 contracts
// (sin, cos)(f_{q / 22} v_{q % 22}); k-steps 220..230 the raw block (v_{2 (q - 220)}, v_{2 (q - 220) + 1}); k-step 231 is padding
struct EmbSrc32 {
  const float* sV;           // + (lane & 31)
  const float* fr;           // freq / 2 pi
  int h;
  __device__ __forceinline__ void frag(int g, int e, float (&b)[kNB]) const {
    const int q = 4 * g + e;                       // wave-uniform
    if (q < 220) {
      const int fj = (q * 2979) >> 16, i = q - 22 * fj;             // q / 22 exact for q < 240
      const float f = fr[fj], ph = h ? 0.25f : 0.0f;
#pragma unroll
      for (int bt = 0; bt < kNB; ++bt) b[bt] = __builtin_amdgcn_sinf(fmaf(sV[i * kRowTile + bt * 32], f, ph));
    } else {
      const int i = 2 * (q - 220) + h;
      const bool ok = i < 22;
#pragma unroll
      for (int bt = 0; bt < kNB; ++bt) b[bt] = ok ? sV[(ok ? i : 0) * kRowTile + bt * 32] : 0.0f;
    }
  }
};

// the pre-activations (or linear outputs) of this wave's tiles -> stash rows frow0 + feature: one 128-byte store per register and half
template <int NTW>
__device__ __forceinline__ void stash32_tiles(const f32x16 (&acc)[NTW][kNB], float* __restrict__ S, int frow0, int64_t Bp, int64_t row0,
                                              int nt0, int b, int h) {
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt) {
      float* p = S + (int64_t)(frow0 + (nt0 + nt) * 32 + 4 * h) * Bp + row0 + bt * 32 + b;
#pragma unroll
      for (int r = 0; r < 16; ++r) p[(int64_t)((r & 3) + 8 * (r >> 2)) * Bp] = acc[nt][bt][r];
    }
}

// CM: coordinate mode (npp_coord.h CoordMode) -- int32 pixel indices, fp32 positions, the implicit canvas grid or that canvas
// under a projective map
// STASH: also write the training stash (A_.stash)
template <bool MULTI, int CM = kCoordI32, bool STASH = false>
__global__ __launch_bounds__(kT32, 2) void mlp_fwd32_kernel(Fwd32Args A_, EmbedDev e_arg, NetDesc d, Desc32 d32) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* R = smem;
  float* sV = (float*)(smem + kRegion32);
  float* sY = sV + 22 * kRowTile;
  float* sX = sY + kRowTile;
  EmbedDev& ed = *(EmbedDev*)(sX + kRowTile);
  WarpEnt* tWarp = (WarpEnt*)((char*)&ed + ((sizeof(EmbedDev) + 15) / 16) * 16);
  if (threadIdx.x == 0) {
    const uint32_t* src = (const uint32_t*)&e_arg;
    uint32_t* dst = (uint32_t*)&ed;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(EmbedDev) / 4); ++i) dst[i] = src[i];
  }
  wg_barrier();
  // build_warp_table(ed, tWarp, kT32), written out: as a call the compiler forms the same table with seven more instructions, and the
  // grid launches of this kernel then measured 0.4 - 0.5 % slower than before at W = 256, twice (profiles/render_intake_refactor.txt)
  for (int wi = threadIdx.x; wi < ed.K * 22; wi += kT32) {
    const int p = wi / 22, i = wi - p * 22, ori = i >= 11, ii = ori ? i - 11 : i;
    WarpEnt w{0.0f, 0.0f, 1.0f, 1.0f, 0.0f, 0.0f};
    if (ii == 0) {
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
  const int tid = threadIdx.x, lane = tid & 63, b = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * kRowTile;
  const float* P = A_.params;
  const int nt0 = 2 * wave;
  if (tid < kRowTile) {
    float y, x;
    row_coord<CM>(A_.coords, A_.src, row0 + tid, y, x);         // (0, 0) for a pixel not in view
    sY[tid] = y;
    sX[tid] = x;
  }
  wg_barrier();

  // the 22 warped coordinates of proposal p -> sV (the same arithmetic as the bf16 chain's gen_warp)
  auto gen_warp = [&](int p) {
    const float y = sY[lane], x = sX[lane];
    for (int i = wave; i < 22; i += kT32 / 64) {
      const WarpEnt w = tWarp[p * 22 + i];
      const float t = __fadd_rn(__fmul_rn(y, w.cs), __fmul_rn(x, w.sn));
      const float qf = floorf(t * w.inv_per);
      float r = fmaf(-qf, w.per, t);
      r = r < 0.0f ? r + w.per : r;
      r = r >= w.per ? r - w.per : r;
      const float sv = __builtin_amdgcn_sinf(fmaf(r, w.inv_per, w.phase));
      sV[i * kRowTile + lane] = w.lin != 0.0f ? t - 1.0f : sv;
    }
  };

  const wrsrc_t rsrc = make_wrsrc(A_.w32, d32.total16);
  const ActSrc32 act{R + ((4 * h) * kRowTile + b) * 4};
  const EmbSrc32 emb{sV + b, ed.freq_rev, h};
  auto w32 = [&](int l) -> uint32_t { return (uint32_t)d32.off16[l]; };
  constexpr int GA = kW / 8;                       // 32 groups per 256 activation features
  constexpr int GE = 58;                           // 232 k-steps per proposal
  constexpr uint32_t U = kNT * 64;                 // 16-byte units per k-step group of a 256-wide layer

  f32x16 acc[2][kNB];
  // ---- L0
  // STASH: the 22 warped coordinates of proposal p (complete in sV behind a barrier) -> stash rows kS32V + 22 p + i
  auto stash_warp = [&](int p) {
    for (int i = tid; i < 22 * kRowTile; i += kT32)
      A_.stash[(int64_t)(kS32V + 22 * p + i / kRowTile) * A_.Bp + row0 + (i % kRowTile)] = sV[i];
  };
  auto stash_z = [&](const f32x16 (&t)[2][kNB], int frow0) { stash32_tiles<2>(t, A_.stash, frow0, A_.Bp, row0, nt0, b, h); };
  gen_warp(0);
  bias32(acc, P + d.b_off[L0], nt0, h);
  wg_barrier();
  if (STASH) stash_warp(0);
  part32<2, kNT>(acc, rsrc, w32(L0), GE, nt0, lane, emb);
  if (STASH) stash_z(acc, 0);
  epi32<true, 2>(acc, R, nt0, b, h);               // nobody reads R yet
  wg_barrier();
  // ---- L1..L4 (in place: read R, barrier, write R)
#pragma unroll 1
  for (int l = L1; l <= L4; ++l) {
    bias32(acc, P + d.b_off[l], nt0, h);
    part32<2, kNT>(acc, rsrc, w32(l), GA, nt0, lane, act);
    if (STASH) stash_z(acc, l * kW);
    wg_barrier();
    epi32<true, 2>(acc, R, nt0, b, h);
    wg_barrier();
  }
  // ---- L5 = [emb(p0), h]   (sV still holds proposal 0)
  bias32(acc, P + d.b_off[L5], nt0, h);
  part32<2, kNT>(acc, rsrc, w32(L5), GE, nt0, lane, emb);
  part32<2, kNT>(acc, rsrc, w32(L5) + GE * U, GA, nt0, lane, act);
  if (STASH) stash_z(acc, L5 * kW);
  wg_barrier();
  epi32<true, 2>(acc, R, nt0, b, h);
  wg_barrier();
#pragma unroll 1
  for (int l = L6; l <= L7; ++l) {
    bias32(acc, P + d.b_off[l], nt0, h);
    part32<2, kNT>(acc, rsrc, w32(l), GA, nt0, lane, act);
    if (STASH) stash_z(acc, l * kW);
    wg_barrier();
    epi32<true, 2>(acc, R, nt0, b, h);
    wg_barrier();
  }
  // ---- F1 (linear); its tiles stay in registers: P needs f1 again after S / F2 have recycled the region
  f32x16 f1[2][kNB];
  bias32(f1, P + d.b_off[LF1], nt0, h);
  part32<2, kNT>(f1, rsrc, w32(LF1), GA, nt0, lane, act);
  if (STASH) stash_z(f1, kS32F1);
  wg_barrier();
  epi32<false, 2>(f1, R, nt0, b, h);
  wg_barrier();

  f32x16 accp[1][kNB];
  if (MULTI) {
    // ---- S = [f1 (R), emb(p1..)]
    bias32(acc, P + d.b_off[LS], nt0, h);
    part32<2, kNT>(acc, rsrc, w32(LS), GA, nt0, lane, act);
    for (int p = 1; p < d.K; ++p) {
      wg_barrier();                                // every wave is done with the previous proposal's sV
      gen_warp(p);
      wg_barrier();
      if (STASH) stash_warp(p);
      part32<2, kNT>(acc, rsrc, w32(LS) + (uint32_t)(GA + (p - 1) * GE) * U, GE, nt0, lane, emb);
    }
    if (STASH) stash_z(acc, kS32ZS);
    wg_barrier();
    epi32<true, 2>(acc, R, nt0, b, h);             // a_s
    wg_barrier();
    // ---- F2 (linear) -> R (in place)
    bias32(acc, P + d.b_off[LF2], nt0, h);
    part32<2, kNT>(acc, rsrc, w32(LF2), GA, nt0, lane, act);
    if (STASH) stash_z(acc, kS32F2);
    wg_barrier();
    epi32<false, 2>(acc, R, nt0, b, h);            // f2
    wg_barrier();
    // ---- P = [f1, f2] -> 128: one neuron tile per wave; pack order: the f2 k-steps first, then f1
    bias32(accp, P + d.b_off[LP], wave, h);
    part32<1, kNT / 2>(accp, rsrc, w32(LP), GA, wave, lane, act);
    wg_barrier();
    epi32<false, 2>(f1, R, nt0, b, h);             // f1 back into the region
    wg_barrier();
    part32<1, kNT / 2>(accp, rsrc, w32(LP) + GA * (U / 2), GA, wave, lane, act);
  } else {
    bias32(accp, P + d.b_off[LP], wave, h);
    part32<1, kNT / 2>(accp, rsrc, w32(LP), GA, wave, lane, act);
  }
  if (STASH) stash32_tiles<1>(accp, A_.stash, kS32ZP, A_.Bp, row0, wave, b, h);
  epi32<true, 1>(accp, nullptr, wave, b, h);       // a_p stays in registers

  // ---- rgb_linear 128 -> 3 + output activation (models/helpers.py:55-58)
  wg_barrier();
  float* sRGB = (float*)R;                         // [4 waves][64 rows][3]
  float* sStage = sRGB + (kNT / 2) * kRowTile * 3; // the SS modes: kStageWords behind it (the region is free by now)
  static_assert(((kNT / 2) * kRowTile * 3 + kStageWords) * 4 <= kRegion32, "LDS");
  {
    const float* Wr = P + d.w_off[LRGB];
    float part[kNB][3];
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt)
#pragma unroll
      for (int c = 0; c < 3; ++c) part[bt][c] = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = wave * 32 + acc_row(r, h);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float w = Wr[c * (kW / 2) + k];
#pragma unroll
        for (int bt = 0; bt < kNB; ++bt) part[bt][c] = fmaf(w, accp[0][bt][r], part[bt][c]);
      }
    }
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = part[bt][c] + __shfl_xor(part[bt][c], 32, 64);
        if (h == 0) sRGB[(wave * kRowTile + bt * 32 + b) * 3 + c] = v;
      }
  }
  wg_barrier();
  if (tid < kRowTile * 3) {
    const int row = tid / 3, c = tid - row * 3;
    float z = P[d.b_off[LRGB] + c];
#pragma unroll
    for (int w = 0; w < kNT / 2; ++w) z += sRGB[(w * kRowTile + row) * 3 + c];
    const float o = A_.out_act == 1 ? 1.0f / (1.0f + expf(-z)) : (A_.out_act == 2 ? tanhf(z) : z);
    store_rgb<CM>(A_.src, A_.pred, row0 + row, c, o, sStage);
  }
  if (coord_is_ss(CM)) {                             // the ss x ss samples of a pixel -> their ordered mean (npp_coord.h)
    wg_barrier();
    average_rgb<CM>(A_.src, A_.pred, row0, tid, sStage);
  }
}

// fp32 pack: unit u (16 bytes) = [layer][k-step group g][neuron tile nt][lane]: element e = W[32 nt + (lane & 31)][col32(l, 4 g + e, lane >> 5)]
__global__ void pack32_kernel(const float* __restrict__ P, float* __restrict__ out, NetDesc d, Desc32 d32) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= d32.total16) return;
  int l = 0;
  for (int q = 0; q < kNumLayers; ++q)
    if (d32.present[q] && u >= d32.off16[q]) l = q;
  const int64_t r = u - d32.off16[l];
  const int lane = (int)(r & 63);
  const int nt = (int)((r >> 6) % d32.nt[l]);
  const int g = (int)((r >> 6) / d32.nt[l]);
  const int row = nt * 32 + (lane & 31), h = lane >> 5;
  f32x4_t o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int col = col32(d.K, l, 4 * g + e, h);
    o[e] = col < 0 ? 0.0f : P[d.w_off[l] + (int64_t)row * d.n_in[l] + col];
  }
  ((f32x4_t*)out)[u] = o;
}

}  // namespace npp

using namespace npp;

extern "C" int64_t npp_pack32_bytes(int K, int width) {
  if (K < 1 || K > NPP_MAX_K || width != NPP_WIDTH) { set_error("npp_pack32_bytes: K=%d width=%d", K, width); return -1; }
  return make_desc32(K).total16 * 16;
}

extern "C" int npp_pack_weights32(const float* d_params, void* d_w32, int K, int width, void* stream) {
  if (K < 1 || K > NPP_MAX_K || width != NPP_WIDTH || !d_params || !d_w32) { set_error("npp_pack_weights32: bad argument"); return NPP_ERR_ARG; }
  const Desc32 d32 = make_desc32(K);
  hipLaunchKernelGGL(pack32_kernel, dim3((unsigned)((d32.total16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_params,
                     (float*)d_w32, make_desc(K), d32);
  return check_launch("npp_pack_weights32");
}

template <int CM, bool STASH = false>
static int fwd32_launch(const Fwd32Args& A, const npp_embed_cfg* cfg, void* stream, const char* who) {
  const EmbedDev e = make_embed_dev(*cfg);
  const NetDesc d = make_desc(cfg->K);
  const Desc32 d32 = make_desc32(cfg->K);
  const dim3 grid((unsigned)(A.Bp / kRowTile)), block(kT32);
  const hipStream_t s = (hipStream_t)stream;
  return cfg->K > 1 ? launch_lds<mlp_fwd32_kernel<true, CM, STASH>>(who, grid, block, kSmem32, kSmem32, s, A, e, d, d32)
                    : launch_lds<mlp_fwd32_kernel<false, CM, STASH>>(who, grid, block, kSmem32, kSmem32, s, A, e, d, d32);
}

// The arguments every launch of the chain shares; n rows are computed in whole 64-row tiles
static Fwd32Args fwd32_args(int64_t n, const void* d_w32, const float* d_params, float* d_out, int out_act) {
  Fwd32Args A{};
  A.Bp = (n + kRowTile - 1) / kRowTile * kRowTile; A.w32 = (const float*)d_w32; A.params = d_params; A.pred = d_out; A.out_act = out_act;
  return A;
}

extern "C" int npp_mlp_fwd32(const int32_t* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_w32,
                             const float* d_params, float* d_out, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32";
  const int rc = fwd_entry_check(who, cfg, width, Bp, false, d_coords_yx, d_w32, d_params, d_out, out_act);
  if (rc) return rc;
  Fwd32Args A = fwd32_args(Bp, d_w32, d_params, d_out, out_act);
  A.coords = d_coords_yx;
  return fwd32_launch<kCoordI32>(A, cfg, stream, who);
}

extern "C" int npp_mlp_fwd32_coordf(const float* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_w32,
                                    const float* d_params, float* d_out, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32_coordf";
  const int rc = fwd_entry_check(who, cfg, width, Bp, false, d_coords_yx, d_w32, d_params, d_out, out_act);
  if (rc) return rc;
  Fwd32Args A = fwd32_args(Bp, d_w32, d_params, d_out, out_act);
  A.src.coordsf = d_coords_yx;
  return fwd32_launch<kCoordF32>(A, cfg, stream, who);
}

extern "C" int npp_mlp_fwd32_grid(const npp_grid* grid, const npp_embed_cfg* cfg, int width, const void* d_w32, const float* d_params,
                                  float* d_out, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32_grid";
  int rc = check_grid(grid, who);
  if (rc || (rc = fwd_entry_check(who, cfg, width, grid->n, true, nullptr, d_w32, d_params, d_out, out_act)) || grid->n == 0) return rc;
  Fwd32Args A = fwd32_args(grid->n, d_w32, d_params, d_out, out_act);
  A.src.g = *grid;
  return fwd32_launch<kCoordGrid>(A, cfg, stream, who);
}

extern "C" int npp_mlp_fwd32_view(const npp_view* view, const npp_embed_cfg* cfg, int width, const void* d_w32, const float* d_params,
                                  float* d_out, uint8_t* d_inside, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32_view";
  int rc = check_view(view, who);
  if (rc || (rc = fwd_entry_check(who, cfg, width, view->n, true, nullptr, d_w32, d_params, d_out, out_act)) || view->n == 0) return rc;
  Fwd32Args A = fwd32_args(view->n, d_w32, d_params, d_out, out_act);
  A.src.view.v = *view; A.src.view.inside = d_inside; A.src.view.H = cfg->H; A.src.view.W = cfg->W;
  return fwd32_launch<kCoordView>(A, cfg, stream, who);
}

// ss x ss samples per canvas pixel, averaged in the store epilogue (include/npp_hip.h "supersampled launches"): n ss^2 rows, n stored
extern "C" int npp_mlp_fwd32_grid_ss(const npp_grid* grid, int ss, const npp_embed_cfg* cfg, int width, const void* d_w32,
                                     const float* d_params, float* d_out, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32_grid_ss";
  if (ss == 1) return npp_mlp_fwd32_grid(grid, cfg, width, d_w32, d_params, d_out, out_act, stream);
  int rc = check_grid(grid, who);
  if (rc || (rc = check_ss(ss, grid->start, grid->n, grid->width, who)) ||
      (rc = fwd_entry_check(who, cfg, width, grid->n, true, nullptr, d_w32, d_params, d_out, out_act)) || grid->n == 0) return rc;
  Fwd32Args A = fwd32_args(grid->n * ss * ss, d_w32, d_params, d_out, out_act);
  A.src.g = *grid; A.src.ss = ss;
  return fwd32_launch<kCoordGridSS>(A, cfg, stream, who);
}

extern "C" int npp_mlp_fwd32_view_ss(const npp_view* view, int ss, const npp_embed_cfg* cfg, int width, const void* d_w32,
                                     const float* d_params, float* d_out, uint8_t* d_inside, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32_view_ss";
  if (ss == 1) return npp_mlp_fwd32_view(view, cfg, width, d_w32, d_params, d_out, d_inside, out_act, stream);
  int rc = check_view(view, who);
  if (rc || (rc = check_ss(ss, view->start, view->n, view->width, who)) ||
      (rc = fwd_entry_check(who, cfg, width, view->n, true, nullptr, d_w32, d_params, d_out, out_act)) || view->n == 0) return rc;
  Fwd32Args A = fwd32_args(view->n * ss * ss, d_w32, d_params, d_out, out_act);
  A.src.view.v = *view; A.src.view.inside = d_inside; A.src.view.H = cfg->H; A.src.view.W = cfg->W; A.src.ss = ss;
  return fwd32_launch<kCoordViewSS>(A, cfg, stream, who);
}

// npp_mlp_fwd32_view_ss over the n_list listed pixels of the window (include/npp_hip.h "listed launches"): n_list ss^2 rows; ss = 1 too
// runs the listed mode (its store keeps the point launch's bits)
extern "C" int npp_mlp_fwd32_view_list(const npp_view* view, int ss, const int64_t* d_pix, int64_t n_list, const npp_embed_cfg* cfg,
                                       int width, const void* d_w32, const float* d_params, float* d_out, uint8_t* d_inside, int out_act,
                                       void* stream) {
  const char* who = "npp_mlp_fwd32_view_list";
  int rc = check_view(view, who);
  if (rc || (rc = check_ss(ss, view->start, view->n, view->width, who)) || (rc = check_list(ss, d_pix, n_list, who)) ||
      (rc = fwd_entry_check(who, cfg, width, view->n, true, nullptr, d_w32, d_params, d_out, out_act)) || view->n == 0 || n_list == 0)
    return rc;
  Fwd32Args A = fwd32_args(n_list * ss * ss, d_w32, d_params, d_out, out_act);
  A.src.view.v = *view; A.src.view.inside = d_inside; A.src.view.H = cfg->H; A.src.view.W = cfg->W; A.src.ss = ss;
  A.src.pix = d_pix; A.src.n_list = n_list;
  return fwd32_launch<kCoordViewList>(A, cfg, stream, who);
}

// The forward of the exact-fp32 fit: npp_mlp_fwd32 plus the stash (d_stash: sizes[1] of npp_train_workspace32)
extern "C" int npp_mlp_fwd32_train(const int32_t* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_w32,
                                   const float* d_params, float* d_pred, void* d_stash, int out_act, void* stream) {
  const char* who = "npp_mlp_fwd32_train";
  const int rc = fwd_entry_check(who, cfg, width, Bp, false, d_coords_yx, d_w32, d_params, d_pred, out_act);
  if (rc) return rc;
  if (!d_stash) { set_error("%s: null stash", who); return NPP_ERR_ARG; }
  Fwd32Args A = fwd32_args(Bp, d_w32, d_params, d_pred, out_act);
  A.coords = d_coords_yx; A.stash = (float*)d_stash;
  return fwd32_launch<kCoordI32, true>(A, cfg, stream, who);
}
