// npp_dev_sampler.h -- the draw arithmetic of rng_mode="device", shared by the kernels of npp_dev_sampler.hip and their host
// twins (the npp_pack_scatter_host precedent: one definition, compiled for both sides, so the CPU suite checks the arithmetic the
// GPU runs).  What is drawn: the decisions of models/sampler.py:242-354 (patch source :324-331, fake-patch centres :260, lattice
// candidates + unknown-pixel filter + k nearest :148-214) and the N_rand pixel rows of NPP_completion/train.py:172 -- from a
// counter-based generator instead of np.random's stream, so a draw is a pure function of (seed, draw index t, inputs).
#pragma once
#include <math.h>
#include <stdint.h>

#include "npp_hip.h"

#if defined(__HIPCC__)
#define NPP_HD __host__ __device__ inline
#else
#define NPP_HD inline
#endif

namespace npp {
namespace devs {

struct U4 {
  uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32_R(10, ...)).
NPP_HD U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    U4 n;
    n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
    n.y = (uint32_t)p1;
    n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
    n.w = (uint32_t)p0;
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// Patch source of draw t (sampler.py:324-331 on u = word 0 of counter (0, 0, t, 0) times 2^-32): 0 'val', 1 'train', 2 'same'.
NPP_HD int patch_source(uint32_t t, uint32_t k0, uint32_t k1) {
  const U4 c = {0u, 0u, t, 0u};
  const double u = (double)philox4x32_10(c, k0, k1).x * (1.0 / 4294967296.0);
  if (u < 0.5) return NPP_DEV_SRC_VAL;
  if (0.5 < u && u < 0.8) return NPP_DEV_SRC_TRAIN;
  return NPP_DEV_SRC_SAME;
}

// Position i of the keyed permutation of [0, N) for (t, stream): a balanced Feistel network of eight rounds on the smallest
// even-width domain (at least 2 bits) that holds N - 1, walked along its cycle until it lands in range.  Positions 0..n-1 are n
// draws without replacement: no population-sized shuffle, no state, any position on its own.  1 <= N <= 2^32, 0 <= i < N.
NPP_HD int64_t perm_index(int64_t N, int64_t i, uint32_t t, uint32_t stream, uint32_t k0, uint32_t k1) {
  int bits = 0;
  for (uint64_t v = (uint64_t)(N - 1); v; v >>= 1) ++bits;
  if (bits < 2) bits = 2;
  bits += bits & 1;
  const int b = bits / 2;
  const uint32_t mask = (uint32_t)((1ull << b) - 1ull);
  uint64_t x = (uint64_t)i;
  do {
    uint32_t L = (uint32_t)(x >> b), R = (uint32_t)x & mask;
    for (uint32_t r = 0; r < 8; ++r) {
      const U4 c = {R, r, t, stream};
      const uint32_t F = philox4x32_10(c, k0, k1).x & mask;
      const uint32_t nR = L ^ F;
      L = R;
      R = nR;
    }
    x = ((uint64_t)L << b) | R;
  } while (x >= (uint64_t)N);
  return (int64_t)x;
}

constexpr int kCand = 400;         // the 20 x 20 lattice neighbourhood a, b in [-10, 10) (sampler.py:90-93)
constexpr int kNoCand = 0x7fffffff;

// Lattice candidate idx (a = idx / 20 - 10 outer, b = idx % 20 - 10 inner) of the fake patch at (cy, cx): cen + a s0 + b s1 in
// float64, left to right, NOT contracted to FMA (a fused product would move half-integer ties of the rint below).
NPP_HD void cand_pos(int cy, int cx, const double* s, int idx, double* y, double* x) {
#pragma clang fp contract(off)
  const double a = (double)(idx / 20 - 10), b = (double)(idx % 20 - 10);
  const double ay = a * s[0], ax = a * s[1], by = b * s[2], bx = b * s[3];
  const double y1 = (double)cy + ay, x1 = (double)cx + ax;
  *y = y1 + by;
  *x = x1 + bx;
}

NPP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// -> the candidate's selection key dist * 512 + idx (a stable order by distance, then by candidate index, is the order of the
// keys), or kNoCand when it fails the bounds test (sampler.py:161-164) or has more than P P invalid_ratio unknown pixels (:181;
// counted from the summed-area table of the known mask at rint of the position, out-of-image pixels unknown).
NPP_HD int cand_key(const npp_dev_image& im, int cy, int cx, int idx) {
#pragma clang fp contract(off)
  double y, x;
  cand_pos(cy, cx, im.shifts, idx, &y, &x);
  if (!(y > 0.0 && y < (double)(im.H - 1) && x > 0.0 && x < (double)(im.W - 1))) return kNoCand;
  const int ry = (int)rint(y), rx = (int)rint(x), h = im.P / 2;
  const int y0 = clampi(ry - h, 0, im.H), y1 = clampi(ry + h, 0, im.H);
  const int x0 = clampi(rx - h, 0, im.W), x1 = clampi(rx + h, 0, im.W);
  const int64_t ld = im.W + 1;
  const int known = im.sat[y1 * ld + x1] - im.sat[y0 * ld + x1] - im.sat[y1 * ld + x0] + im.sat[y0 * ld + x0];
  const int unknown = im.P * im.P - known;
  if ((double)unknown > (double)(im.P * im.P) * im.invalid_ratio) return kNoCand;
  const int a = idx / 20 - 10, b = idx % 20 - 10;
  int d = (a < 0 ? -a : a) + (b < 0 ? -b : b);
  if (d == 0) d = 10000;                                       // sampler.py:197
  return d * 512 + idx;
}

// Record of one image's draw (int32 words): [0] source, [1] k (0: no valid real patch, the iteration is skipped; -1: the pool
// holds fewer than n_p pixels), [2] n_p, [3] t; then the centres (row, col) of the n_p fake patches followed by the n_p k real
// ones (the order of GridPatchSampler.centres_i32); then, at word 4 + 2 n_p (1 + topk), the n_p k weights as float.
NPP_HD int64_t record_words(int n_p, int topk) { return 4 + 2 * (int64_t)n_p * (1 + topk) + (int64_t)n_p * topk; }
NPP_HD int64_t record_weights_at(int n_p, int topk) { return 4 + 2 * (int64_t)n_p * (1 + topk); }

// Fake-patch centre i of the draw: position i of the stream-1 permutation of the source's bounds-filtered pool.
NPP_HD void fake_centre(const npp_dev_image& im, int source, int i, uint32_t t, int* cy, int* cx) {
  const int32_t* pool = source == NPP_DEV_SRC_VAL ? im.pool_val : im.pool_train;
  const int64_t N = source == NPP_DEV_SRC_VAL ? im.n_pool_val : im.n_pool_train;
  const int64_t j = perm_index(N, i, t, 1u, im.seed_lo, im.seed_hi);
  *cy = pool[2 * j];
  *cx = pool[2 * j + 1];
}

// The real half of fake patch p once every patch's selection is known: sel = the keys of the topk best candidates per patch in
// order (kNoCand where there are fewer), cnt = candidates that passed the tests.  GridPatchSampler.draw() normalises patch p's
// weights over the running minimum k_p = min_{j <= p} min(cnt_j - 1, topk) and truncates to the final minimum k afterwards.
NPP_HD void write_real(const npp_dev_image& im, const int* sel, const int* cnt, int n_p, int topk, int k, int p, int cy, int cx,
                       int32_t* rec) {
#pragma clang fp contract(off)
  int kp = topk;
  for (int j = 0; j <= p; ++j) {
    const int kj = cnt[j] - 1 < topk ? cnt[j] - 1 : topk;
    kp = kj < kp ? kj : kp;
  }
  double sum = 0.0;
  for (int r = 0; r < kp; ++r) sum += 1.0 / (double)(sel[p * topk + r] >> 9);
  int32_t* cen = rec + 4 + 2 * ((int64_t)n_p + (int64_t)p * k);
  float* w = (float*)(rec + record_weights_at(n_p, topk)) + (int64_t)p * k;
  for (int r = 0; r < k; ++r) {
    const int key = sel[p * topk + r];
    double y, x;
    cand_pos(cy, cx, im.shifts, key & 511, &y, &x);
    cen[2 * r] = (int32_t)rint(y);
    cen[2 * r + 1] = (int32_t)rint(x);
    w[r] = (float)((1.0 / (double)(key >> 9)) / sum);
  }
}

NPP_HD int final_k(const int* cnt, int n_p, int topk) {
  int k = topk;
  for (int j = 0; j < n_p; ++j) {
    const int kj = cnt[j] - 1 < topk ? cnt[j] - 1 : topk;
    k = kj < k ? kj : k;
  }
  return k < 0 ? 0 : k;
}

}  // namespace devs
}  // namespace npp
