// npp_adam.h -- the one statement of torch.optim.Adam's update, of its step-dependent scalars and of the split-K slab sum that
// feeds it.  Included by npp_loss_adam.hip (npp_adam_step), npp_api.hip (the fused Adam + re-pack launch) and npp_light_common.h
// (the Adam launches of the candidate-ranking fits).
#pragma once
#include "npp_common.h"

namespace npp {

// ---- K8: torch.optim.Adam single-tensor maths (helpers.py:164), shared by npp_loss_adam.hip and the fused Adam + re-pack
// launch of npp_api.hip.  tail (optional, handled by one extra block): a second small parameter group -- the adaptive-loss
// latents, whose gradient accumulator is consumed and cleared -- and an accumulator to clear for the next iteration, so
// that one launch replaces optimizer.step() over both groups plus zero_grad().
struct AdamTail {
  float *p, *m, *v, *g;
  int n;
  float* zero;
  int n_zero;
  // round 4: the pixel loss of the iteration left its per-block partial sums in `pl_part` (PixelLossArgs::scratch) instead of
  // adding them to g / the loss word by atomics in arrival order; this block -- the consumer of g, one launch boundary later --
  // sums them in block order: bit-reproducible and free (no ticket, no fence, no extra launch).  Nullable.
  float* pl_part;
  float* loss_cur;      // the iteration's pixel-loss accumulator (+= the partial losses), nullable
};
constexpr int kPixelLossScratch = 1024 * 8 + 8;       // [block][8] partials (7 used) + the block count in the last word
// The one statement of the update: every Adam kernel of the library goes through it.
__device__ __forceinline__ float adam_update(float p, float& m, float& v, float g, float step_size, float b1, float b2,
                                             float inv_sqrt_bc2, float eps) {
  m = b1 * m + (1.0f - b1) * g;
  v = b2 * v + (1.0f - b2) * g * g;
  return p - step_size * (m / (sqrtf(v) * inv_sqrt_bc2 + eps));
}
// The step-dependent scalars of a launch, from the host: the only place the bias corrections are computed (npp_adam_words
// exports it; ops.adam_words is its Python twin).  The float arguments are widened, the results rounded once.
struct AdamWords { float step_size, inv_sqrt_bc2; };
inline AdamWords adam_words(float lr, float beta1, float beta2, int step) {
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  return AdamWords{(float)((double)lr / bc1), (float)(1.0 / sqrt(bc2))};
}
// The gradient of a parameter is the sum of its split-K slabs, in slab order (npp_mlp_wgrad): four slab loads in flight before
// the order-preserving summation, then the remainder.  T = float: one element; T = adam_f4: four consecutive ones (16-byte aligned).
typedef float adam_f4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T slab_sum(const float* __restrict__ g, int n_slabs, int64_t slab_stride) {
  auto ld = [&](int sl) { return *(const T*)(g + (int64_t)sl * slab_stride); };
  T gi = (T)(0.0f);
  int sl = 0;
  for (; sl + 4 <= n_slabs; sl += 4) {
    const T a0 = ld(sl), a1 = ld(sl + 1), a2 = ld(sl + 2), a3 = ld(sl + 3);
    gi += a0; gi += a1; gi += a2; gi += a3;
  }
  for (; sl < n_slabs; ++sl) gi += ld(sl);
  return gi;
}
// Elements i .. i + cnt - 1 (cnt = 4: one 16-byte access per array; cnt < 4: the last n % 4 parameters, element by element) of
// the blob: slab sum, update, store.  pn: the new parameters, for a caller that goes on with them (the re-pack scatter).
__device__ __forceinline__ void adam_quad(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                          const float* __restrict__ g, int64_t i, int cnt, int n_slabs, int64_t slab_stride,
                                          float step_size, float b1, float b2, float inv_sqrt_bc2, float eps, float pn[4]) {
  if (cnt == 4) {
    const adam_f4 gi = slab_sum<adam_f4>(g + i, n_slabs, slab_stride);
    adam_f4 mi = *(const adam_f4*)(m + i), vi = *(const adam_f4*)(v + i), pi = *(const adam_f4*)(p + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mi[e], ve = vi[e];
      pi[e] = pn[e] = adam_update(pi[e], me, ve, gi[e], step_size, b1, b2, inv_sqrt_bc2, eps);
      mi[e] = me;
      vi[e] = ve;
    }
    *(adam_f4*)(m + i) = mi;
    *(adam_f4*)(v + i) = vi;
    *(adam_f4*)(p + i) = pi;
  } else {
    for (int e = 0; e < cnt; ++e) {
      const float ge = slab_sum<float>(g + i + e, n_slabs, slab_stride);
      float me = m[i + e], ve = v[i + e];
      pn[e] = adam_update(p[i + e], me, ve, ge, step_size, b1, b2, inv_sqrt_bc2, eps);
      m[i + e] = me;
      v[i + e] = ve;
      p[i + e] = pn[e];
    }
  }
}
__device__ __forceinline__ void adam_tail_block(const AdamTail& tail, float step_size, float b1, float b2, float inv_sqrt_bc2,
                                                float eps) {
  const int t = threadIdx.x;
  int nb = 0;
  if (tail.pl_part) nb = (int)__float_as_uint(tail.pl_part[kPixelLossScratch - 1]);
  for (int i = t; i < tail.n; i += blockDim.x) {
    float gi = tail.g[i];
    if (i < 6)
      for (int b = 0; b < nb; ++b) gi += tail.pl_part[b * 8 + 1 + i];          // block order
    float mi = tail.m[i], vi = tail.v[i];
    const float pi = adam_update(tail.p[i], mi, vi, gi, step_size, b1, b2, inv_sqrt_bc2, eps);
    tail.m[i] = mi;
    tail.v[i] = vi;
    tail.p[i] = pi;
    tail.g[i] = 0.0f;
  }
  if (nb > 0 && t == 64) {                               // (another wave than the latents': the two sums run side by side)
    float l = 0.0f;
    for (int b = 0; b < nb; ++b) l += tail.pl_part[b * 8];
    if (tail.loss_cur) tail.loss_cur[0] += l;
  }
  for (int i = t; i < tail.n_zero; i += blockDim.x) tail.zero[i] = 0.0f;
  __syncthreads();
  if (nb > 0 && t == 0) tail.pl_part[kPixelLossScratch - 1] = 0.0f;          // consumed
}

}  // namespace npp
