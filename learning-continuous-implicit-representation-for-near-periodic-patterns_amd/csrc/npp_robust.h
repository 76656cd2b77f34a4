// npp_robust.h -- the adaptive robust pixel loss: the per-channel quantities derived from its latents, the loss body that
// npp_pixel_loss and the fused patch-in launch share, and the fixed-order cross-block reduction of one launch.  Included by
// npp_loss_adam.hip, npp_conv.hip, npp_conv_pair.hip, npp_light_common.h (the loss folded into the candidate-ranking backward
// chains), npp_linear.hip, npp_lpips.hip and npp_cx.hip (the ordered reduction).
#pragma once
#include "npp_adam.h"       // kPixelLossScratch: the partial sums are handed to the Adam launch (AdamTail::pl_part)

namespace npp {

// ---- adaptive robust loss: per-channel quantities derived from the latents --------------
// adaptive.py:146-181, distribution.py:90-114,143-169, cubic_spline.py:65-97 (see npp_loss_adam.hip)
struct ChanParams {   // per-channel quantities derived from the latents
  float alpha, c, beta, logc_plus_logz, dlogz, dalpha_dl, dc_dl;
};

__device__ inline ChanParams chan_params(float latent_alpha, float latent_scale, const float* spline,
                                         int n_knots, float x_scale) {
  ChanParams p;
  // adaptive.py:146-164 + util.py:64-72: alpha = sigmoid(l)*(hi-lo)+lo, lo=.001, hi=1.999
  const float sg = 1.0f / (1.0f + expf(-latent_alpha));
  p.alpha = sg * (1.999f - 0.001f) + 0.001f;
  p.dalpha_dl = sg * (1.0f - sg) * (1.999f - 0.001f);
  // adaptive.py:166-181 + util.py:86-95: c = (1-1e-5)*softplus(l + log(e-1)) + 1e-5
  const float xs = latent_scale + 0.54132485f;   // log(expm1(1))
  const float sp = xs > 20.0f ? xs : log1pf(expf(xs));
  p.c = (1.0f - 1e-5f) * sp + 1e-5f;
  p.dc_dl = (1.0f - 1e-5f) / (1.0f + expf(-xs));
  p.beta = fmaxf(1.1920929e-07f, fabsf(p.alpha - 2.0f));
  // distribution.py:90-114 partition_spline_curve (alpha < 4 branch)
  const float den = fabsf(p.alpha - 2.0f) + 0.25f;
  const float xc = (2.25f * p.alpha - 4.5f) / den + p.alpha + 2.0f;
  const float dxc = 0.5625f / (den * den) + 1.0f;
  // cubic_spline.py:65-97
  const float xq = xc * x_scale;
  const float* vals = spline;
  const float* tans = spline + n_knots;
  const int lo = (int)floorf(fminf(fmaxf(xq, 0.0f), (float)(n_knots - 2)));
  const float t = xq - (float)lo, t2 = t * t, t3 = t * t2;
  const float h01 = -2.0f * t3 + 3.0f * t2, h00 = 1.0f - h01, h11 = t3 - t2, h10 = h11 - t2 + t;
  const float v0 = vals[lo], v1 = vals[lo + 1], m0 = tans[lo], m1 = tans[lo + 1];
  float val = v0 * h00 + v1 * h01 + m0 * h10 + m1 * h11;
  const float dh01 = -6.0f * t2 + 6.0f * t, dh11 = 3.0f * t2 - 2.0f * t, dh10 = dh11 - 2.0f * t + 1.0f;
  float dval = (v1 - v0) * dh01 + m0 * dh10 + m1 * dh11;
  if (t < 0.0f) { val = tans[0] * t + vals[0]; dval = tans[0]; }
  else if (t > 1.0f) { val = tans[n_knots - 1] * (t - 1.0f) + vals[n_knots - 1]; dval = tans[n_knots - 1]; }
  p.logc_plus_logz = logf(p.c) + val;
  p.dlogz = dval * x_scale * dxc;
  return p;
}

// ---- a8: adaptive robust pixel loss, forward + gradients (mse_calculator.py:13-27, robust_loss_pytorch) -----------------
// One thread per row (3 channels), block-stride over `nb` blocks of 256 threads; block reduction via wave shuffles, then
// one atomicAdd per block per output (7 floats).  Shared by npp_pixel_loss and the fused patch-in launch.
struct PixelLossArgs {
  const float* pred; const float* gt; const float* mask; int64_t N;
  const float* latents; const float* spline; int n_knots; float x_scale, weight;
  float* loss_out; float* dpred; float* dlatent;
  float* scratch;      // nullable: kPixelLossScratch floats.  Given: the launch leaves its per-block partial sums there (loss_out /
                       // dlatent untouched) for the Adam launch of the iteration to add in block order (AdamTail::pl_part)
  float quad;          // 0: robust_loss_adaptive.  > 0: the non-adaptive switches of models/mse_calculator.py:19-23, both quadratic:
                       // loss = quad * mean(x^2) -- 'l2' (quad = 1) and 'robust_loss' = lossfun(x, alpha = 2, scale = 0.1) = 0.5 (x / 0.1)^2
                       // (quad = 50); latents / spline unused (may be null), no latent gradient
};
// Cross-block reduction in a FIXED order inside one launch: every block publishes its partials, the block that draws the last
// ticket sums them.  cdna_hip_programming.md Guideline 16, form R1 without fences: the (few, small) partials are written with
// relaxed agent-scope atomic stores (share_store: write-through, visible from every XCD once the storing wave's vmcnt has drained)
// and read back with relaxed agent-scope atomic loads (share_load: past this CU's L1 and this XCD's L2) -- an agent-scope release
// fence would write back the XCD's whole L2.  Call from every thread of every block after its share_store()s; true in the whole
// block that arrived last (which re-arms the counter).  The counter must be zero before the first launch that uses it.
// (Where the consumer of a sum is a LATER launch, leave the partials to it instead: AdamTail::pl_part.)
__device__ __forceinline__ void share_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float share_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool block_last_arriver(unsigned* counter, int nb) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave: its partials have left for memory
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == (unsigned)nb - 1u;
    if (s_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return s_last != 0;
}
inline int pixel_loss_blocks(int64_t N) { const int64_t b = (N + 255) / 256; return (int)(b > 1024 ? 1024 : b); }
__device__ __forceinline__ void pixel_loss_body(const PixelLossArgs& a, int bid, int nb) {
  const float* __restrict__ pred = a.pred;
  const float* __restrict__ gt = a.gt;
  const float* __restrict__ mask = a.mask;
  float* __restrict__ dpred = a.dpred;
  const int64_t N = a.N;
  const float weight = a.weight;
  __shared__ ChanParams cp[3];
  __shared__ float red[4][7];
  const float quad = a.quad;
  if (threadIdx.x < 3) {
    if (quad > 0.0f) cp[threadIdx.x] = ChanParams{2.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    else cp[threadIdx.x] = chan_params(a.latents[threadIdx.x], a.latents[3 + threadIdx.x], a.spline, a.n_knots, a.x_scale);
  }
  __syncthreads();
  const float inv = 1.0f / (3.0f * (float)N);
  float acc[7] = {0, 0, 0, 0, 0, 0, 0};   // loss, dalpha[3], dc[3]
  for (int64_t r = (int64_t)bid * blockDim.x + threadIdx.x; r < N; r += (int64_t)nb * blockDim.x) {
    const float m = mask ? mask[r] : 1.0f;
    const float w = m + (1.0f - m) * 0.3f;          // mse_calculator.py:17
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const ChanParams p = cp[ch];
      const float d0 = pred[r * 3 + ch] - gt[r * 3 + ch];
      const float x = mask ? d0 * m + (1.0f - m) * d0 * 0.3f : d0;
      if (quad > 0.0f) {                            // (uniform branch) mse_calculator.py:19-23: 'l2' / 'robust_loss'
        acc[0] += quad * x * x;
        dpred[r * 3 + ch] = weight * inv * w * 2.0f * quad * x;
        continue;
      }
      const float xs = x / p.c, ssx = xs * xs;
      const float u = ssx / p.beta + 1.0f;
      const float e = 0.5f * p.alpha;
      const float lnu = logf(u);
      const float ue = expf(e * lnu);               // pow(u, e), u >= 1
      const float ue1 = ue / u;
      const float rho = (p.beta / p.alpha) * (ue - 1.0f);
      acc[0] += rho + p.logc_plus_logz;
      dpred[r * 3 + ch] = weight * inv * w * (x / (p.c * p.c)) * ue1;
      acc[1 + ch] += -(2.0f / (p.alpha * p.alpha)) * (ue - 1.0f) +
                     (p.beta / p.alpha) * ue * (0.5f * lnu + e * ssx / (p.beta * p.beta * u)) + p.dlogz;
      acc[4 + ch] += -(x * x) / (p.c * p.c * p.c) * ue1 + 1.0f / p.c;
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    float v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (a.scratch) {
    // deterministic form: this block's seven sums, scaled as they enter the totals, for the Adam launch to add in block order
    if (threadIdx.x < 7) {
      const int k = threadIdx.x;
      const float v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
      a.scratch[bid * 8 + k] = k == 0 ? weight * v * inv : k < 4 ? weight * inv * v * cp[k - 1].dalpha_dl : weight * inv * v * cp[k - 4].dc_dl;
    }
    if (bid == 0 && threadIdx.x == 8) a.scratch[kPixelLossScratch - 1] = __uint_as_float((unsigned)nb);
    return;
  }
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    float v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    if (k == 0) atomicAdd(a.loss_out, weight * v * inv);      // the term as it enters the total (train.py:195-198: `loss = 0` under --no_pix_loss)
    else if (quad > 0.0f) {}                                  // (no latents in the quadratic forms)
    else if (k < 4) atomicAdd(a.dlatent + (k - 1), weight * inv * v * cp[k - 1].dalpha_dl);
    else atomicAdd(a.dlatent + 3 + (k - 4), weight * inv * v * cp[k - 4].dc_dl);
  }
}

}  // namespace npp
