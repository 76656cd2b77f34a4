// npp_light_common.h -- what the two forms of NPP_Net_light's fused training chains share (csrc/npp_light.hip: exact fp32;
// csrc/npp_light16.hip: bf16 operands): the order of the packed layers and their place in npp_light_desc, the topology test, the pixel
// loss folded into the head of the backward chains, and the latent column + step scalars of the Adam launches.
#pragma once
#include <math.h>

#include "npp_adam.h"
#include "npp_robust.h"
#include "npp_light_layout.h"

namespace npp {

// packed weights of one candidate: the forward pack's entries, then the transposed pack's of the backward chain
enum { LF_L0 = 0, LF_L1, LF_L2, LF_L3, LF_F1, LF_POS, LF_N };
enum { LB_POS = 0, LB_F1, LB_L3, LB_L2, LB_L1, LB_N };
// pack entry <-> npp_light_desc index li: periodic 0..3, pos (4), feature1 (5), rgb (6: read from the blob by the chains, never packed)
__host__ __device__ inline int light_fwd_layer(int l) { return l < 4 ? l : (l == LF_F1 ? 5 : 4); }
__host__ __device__ inline int light_bwd_layer(int l) { return l == LB_POS ? 4 : (l == LB_F1 ? 5 : 5 - l); }
__host__ __device__ inline int light_fwd_entry(int li) { return li < 4 ? LF_L0 + li : (li == 4 ? LF_POS : LF_F1); }
__host__ __device__ inline int light_bwd_entry(int li) { return li == 4 ? LB_POS : (li == 5 ? LB_F1 : 5 - li); }      // li = 1 .. 5
static_assert(LB_L3 == 2 && LB_L1 == 4, "light_bwd_layer / light_bwd_entry count the hidden layers down from LB_L3");

// the one network both chains are built for
static inline int light_topology_check(const npp_light_desc* L, const char* who) {
  const int n_out[7] = {kLW, kLW, kLW, kLW, kLPosOut, kLW, 3}, n_in[7] = {kLPer, kLW, kLW, kLW, kLW + kLPos, kLW, kLPosOut};
  for (int i = 0; i < 7; ++i)
    if (L->n_out[i] != n_out[i] || L->n_in[i] != n_in[i] || L->ld[i] < n_in[i] || L->w_off[i] < 0 || L->b_off[i] < 0) {
      set_error("%s: layer %d is %d x %d (ld %d): this build fuses NPP_Net_light(D=4, W=256) with 20 / 42 input columns only", who, i,
                L->n_out[i], L->n_in[i], L->ld[i]);
      return NPP_ERR_UNSUPPORTED;
    }
  return NPP_OK;
}

// ---- the pixel loss folded into the backward chains ---------------------------------------------------------------------------------
struct LightLossArgs {
  const float* gt;                              // targets (B, 3) ... (null: d pred is an input)
  const float* latents; const float* spline; int n_knots; float x_scale;      // ... its adaptive-loss latents (C, 6) and spline table
  float* loss; float* dlatent;                  // ... and where the loss words (C) / latent gradients (C, 6) accumulate (float atomics)
  float* part;                                  // the _det forms: (C, blocks, 8) -- every block leaves its seven sums here instead (no atomics)
  int64_t gt_cs;                                // "multi" forms (candidate = one IMAGE's fit with its own targets): elements per candidate, 0 = shared
};

// Head of a backward chain, whole workgroup (THREADS threads own ROWS pixel rows of candidate c from row0 on; the block is number `slot` of
// the candidate's n_slots): d raw = d pred * pred (1 - pred) for thread tid's element (row tid / 3, channel tid % 3) goes to
// store(g, d raw), g = the element's index in (C, B, 3).  With the pixel loss folded in (lo.gt): d pred = d img2mse(robust_loss_adaptive)
// / d pred right here (models/mse_calculator.py:13-27 without a mask: the arithmetic of pixel_loss_body, npp_robust.h); the loss and
// the latent gradients by atomics, or (lo.part) per block in a fixed order.  Ends behind a workgroup barrier that follows every store().
template <int THREADS, int ROWS, class Store>
__device__ __forceinline__ void light_loss_head(const LightLossArgs& lo, const float* __restrict__ pred, const float* __restrict__ dpred, int c,
                                                int64_t B, int64_t row0, int slot, int n_slots, Store&& store) {
  __shared__ ChanParams cp[3];
  __shared__ float sred[7];
  __shared__ float swv[THREADS / 64][7];
  const int tid = threadIdx.x;
  if (lo.gt) {
    if (tid < 3) cp[tid] = chan_params(lo.latents[c * 6 + tid], lo.latents[c * 6 + 3 + tid], lo.spline, lo.n_knots, lo.x_scale);
    if (tid < 7) sred[tid] = 0.0f;
    wg_barrier();
  }
  float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;                 // this thread's loss term and latent-gradient terms (channel tid % 3)
  if (tid < ROWS * 3) {
    const int64_t g = ((int64_t)c * B + row0) * 3 + tid;
    const float p = pred[g];
    float dp;
    if (lo.gt) {
      const int ch = tid % 3;
      const ChanParams q = cp[ch];
      const float inv = 1.0f / (3.0f * (float)B);
      const float x = p - lo.gt[(int64_t)c * lo.gt_cs + row0 * 3 + tid];
      const float xs = x / q.c, ssx = xs * xs;
      const float u = ssx / q.beta + 1.0f, e = 0.5f * q.alpha, lnu = logf(u);
      const float ue = expf(e * lnu), ue1 = ue / u;
      dp = inv * (x / (q.c * q.c)) * ue1;
      t0 = (q.beta / q.alpha) * (ue - 1.0f) + q.logc_plus_logz;
      t1 = -(2.0f / (q.alpha * q.alpha)) * (ue - 1.0f) + (q.beta / q.alpha) * ue * (0.5f * lnu + e * ssx / (q.beta * q.beta * u)) + q.dlogz;
      t2 = -(x * x) / (q.c * q.c * q.c) * ue1 + 1.0f / q.c;
      if (!lo.part) {
        atomicAdd(&sred[0], t0);
        atomicAdd(&sred[1 + ch], t1);
        atomicAdd(&sred[4 + ch], t2);
      }
    } else {
      dp = dpred[g];
    }
    store(g, dp * p * (1.0f - p));
  }
  if (lo.gt && lo.part) {
    // deterministic form (every wave, whole: threads past the 3 ROWS values carry zeros): the seven sums of a wave by shuffle
    // butterflies -- a fixed tree, masked-out lanes add exact zeros -- then the waves' results in wave order
    const int ch = tid % 3;
    const float v7[7] = {t0, ch == 0 ? t1 : 0.0f, ch == 1 ? t1 : 0.0f, ch == 2 ? t1 : 0.0f, ch == 0 ? t2 : 0.0f, ch == 1 ? t2 : 0.0f, ch == 2 ? t2 : 0.0f};
#pragma unroll
    for (int k7 = 0; k7 < 7; ++k7) {
      float v = v7[k7];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((tid & 63) == 0) swv[tid >> 6][k7] = v;
    }
  }
  wg_barrier();
  if (lo.gt && tid < 7) {
    const float inv = 1.0f / (3.0f * (float)B);
    if (lo.part) {
      float v = 0.0f;
#pragma unroll
      for (int w_ = 0; w_ < THREADS / 64; ++w_) v += swv[w_][tid];                          // wave order
      const float o = tid == 0 ? v * inv : (tid < 4 ? inv * v * cp[tid - 1].dalpha_dl : inv * v * cp[tid - 4].dc_dl);
      lo.part[((int64_t)c * n_slots + slot) * 8 + tid] = o;                                 // summed in block order by light_latent_step
    } else {
      const float v = sred[tid];
      if (tid == 0) atomicAdd(lo.loss + c, v * inv);
      else if (tid < 4) atomicAdd(lo.dlatent + c * 6 + (tid - 1), inv * v * cp[tid - 1].dalpha_dl);
      else atomicAdd(lo.dlatent + c * 6 + 3 + (tid - 4), inv * v * cp[tid - 4].dc_dl);
    }
  }
}

// ---- the latent column of the Adam launches (blockIdx.x == gridDim.x - 1) -----------------------------------------------------------------
struct LightLatentArgs {
  float *lat, *lat_m, *lat_v, *dlat, *zero;               // (C, 6) x 4, (C)
  float step_size, b1, b2, inv_sqrt_bc2, eps;             // torch.optim.Adam's single-tensor maths (adam_update, npp_adam.h): the weights' too
  const float* part; int32_t n_part; float* loss_cur;     // the _det forms: the blocks' partial sums of light_loss_head, added here in block order
};
// Adam's step-dependent scalars: adam_words (npp_adam.h), as in npp_adam_step
static inline LightLatentArgs light_latent_args(float* d_lat, float* d_lat_m, float* d_lat_v, float* d_dlat, float* d_zero, float lr, float beta1,
                                         float beta2, float eps, int step, const float* d_part, int n_part, float* d_loss_cur) {
  const AdamWords w = adam_words(lr, beta1, beta2, step);
  return LightLatentArgs{d_lat, d_lat_m, d_lat_v, d_dlat, d_zero, w.step_size, beta1, beta2, w.inv_sqrt_bc2, eps, d_part, n_part, d_loss_cur};
}
// steps candidate c's six adaptive-loss latents and clears one loss word
__device__ __forceinline__ void light_latent_step(const LightLatentArgs& a, int c) {
  const int t = threadIdx.x;
  if (t < 6) {
    const int i = c * 6 + t;
    float g = a.dlat[i];
    if (a.part)                                             // fixed order: bit-reproducible latent gradients
      for (int b = 0; b < a.n_part; ++b) g += a.part[((int64_t)c * a.n_part + b) * 8 + 1 + t];
    float m = a.lat_m[i], v = a.lat_v[i];
    a.lat[i] = adam_update(a.lat[i], m, v, g, a.step_size, a.b1, a.b2, a.inv_sqrt_bc2, a.eps);
    a.lat_m[i] = m; a.lat_v[i] = v; a.dlat[i] = 0.0f;
  } else if (t == 6 && a.zero) a.zero[c] = 0.0f;
  else if (t == 64 && a.part && a.loss_cur) {               // (another wave: the two sums run side by side)
    float l = 0.0f;
    for (int b = 0; b < a.n_part; ++b) l += a.part[((int64_t)c * a.n_part + b) * 8];
    a.loss_cur[c] += l;
  }
}

}  // namespace npp
