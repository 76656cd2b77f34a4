// npp_dev_sampler.hip -- rng_mode="device": the sampler's decisions on the GPU (include/npp_hip.h "rng_mode=device").
//
// The reference draws, per iteration and on a host core, the patch source, the fake-patch centres and the real patches of the
// lattice (models/sampler.py:242-354) and the N_rand pixel rows (NPP_completion/train.py:172: np.random.choice over i_train,
// a shuffle of the whole population).  Here the same decisions come from two launches that serve M images at once and read no
// state: every number is Philox4x32-10 of (seed, draw index t, position), the arithmetic is csrc/npp_dev_sampler.h, which the
// *_host twins below run unchanged on the CPU.  No float atomics; the output depends on (seed, t, inputs) only.
#include "npp_common.h"
#include "npp_dev_sampler.h"

namespace npp {

using namespace devs;

struct DevTs {
  uint32_t t[NPP_DEV_MAX_IMAGES];
};

constexpr int kDecideThreads = 256;

// One workgroup per image.  Phase 0: the source and the n_p fake centres.  Phase 1: one wave per fake patch in turn walks the
// 400 candidates (7 per lane) and selects the topk smallest keys (dist * 512 + idx: stable by distance, then index) by topk
// wave-wide minima.  Phase 2, behind the barrier: k = min over the patches, then the compact centre list and the weights.
// LDS (dynamic): cnt[n_p] | sel[n_p topk] | cen[2 n_p] ints.
__global__ __launch_bounds__(kDecideThreads) void dev_decide_kernel(const npp_dev_image* __restrict__ imgs, DevTs ts, int n_p,
                                                                    int topk, int32_t* __restrict__ recs, int64_t rec_stride) {
  extern __shared__ int s_mem[];
  int* s_cnt = s_mem;
  int* s_sel = s_mem + n_p;
  int* s_cen = s_sel + n_p * topk;
  const int m = blockIdx.x, tid = threadIdx.x;
  const npp_dev_image im = imgs[m];
  const uint32_t t = ts.t[m];
  int32_t* rec = recs + (int64_t)m * rec_stride;
  const int source = patch_source(t, im.seed_lo, im.seed_hi);
  const int64_t N = source == NPP_DEV_SRC_VAL ? im.n_pool_val : im.n_pool_train;
  if (tid == 0) {
    rec[0] = source;
    rec[2] = n_p;
    rec[3] = (int32_t)t;
  }
  if (N < n_p) {                                           // (uniform over the workgroup) np.random.choice raises: so does the host
    if (tid == 0) rec[1] = -1;
    return;
  }
  for (int i = tid; i < n_p; i += kDecideThreads) {
    int cy, cx;
    fake_centre(im, source, i, t, &cy, &cx);
    s_cen[2 * i] = cy;
    s_cen[2 * i + 1] = cx;
    rec[4 + 2 * i] = cy;
    rec[4 + 2 * i + 1] = cx;
  }
  if (source == NPP_DEV_SRC_SAME) {                        // sampler.py:332-338: the fake patches are their own real ones
    float* w = (float*)(rec + record_weights_at(n_p, topk));
    for (int i = tid; i < n_p; i += kDecideThreads) w[i] = 1.0f;
    if (tid == 0) rec[1] = 1;
    return;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int p = wave; p < n_p; p += kDecideThreads / 64) {
    const int cy = s_cen[2 * p], cx = s_cen[2 * p + 1];
    int keys[7];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int idx = lane + 64 * j;
      keys[j] = idx < kCand ? cand_key(im, cy, cx, idx) : kNoCand;
      cnt += keys[j] != kNoCand;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    for (int r = 0; r < topk; ++r) {
      int mine = keys[0];
#pragma unroll
      for (int j = 1; j < 7; ++j) mine = keys[j] < mine ? keys[j] : mine;
      int best = mine;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
      }
      if (best != kNoCand) {                               // the keys are distinct: exactly one lane holds the minimum
#pragma unroll
        for (int j = 0; j < 7; ++j)
          if (keys[j] == best) keys[j] = kNoCand;
      }
      if (lane == 0) s_sel[p * topk + r] = best;
    }
    if (lane == 0) s_cnt[p] = cnt;
  }
  __syncthreads();
  const int k = final_k(s_cnt, n_p, topk);
  if (tid == 0) rec[1] = k;
  if (k <= 0) return;
  for (int p = tid; p < n_p; p += kDecideThreads) write_real(im, s_sel, s_cnt, n_p, topk, k, p, s_cen[2 * p], s_cen[2 * p + 1], rec);
}

__global__ __launch_bounds__(256) void dev_pixels_kernel(const npp_dev_image* __restrict__ imgs, DevTs ts, int64_t n_pix,
                                                         int64_t* __restrict__ pix, int64_t pix_stride) {
  const int m = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pix) return;
  const int64_t N = imgs[m].n_train;
  // (j >= N cannot be drawn without replacement: refused by the caller; never walk from outside the domain)
  pix[(int64_t)m * pix_stride + j] = j < N ? perm_index(N, j, ts.t[m], 2u, imgs[m].seed_lo, imgs[m].seed_hi) : 0;
}

// The serial twin of dev_decide_kernel for one image.
static void decide_host_one(const npp_dev_image& im, uint32_t t, int n_p, int topk, int32_t* rec, int* cnt, int* sel, int* cen) {
  const int source = patch_source(t, im.seed_lo, im.seed_hi);
  const int64_t N = source == NPP_DEV_SRC_VAL ? im.n_pool_val : im.n_pool_train;
  rec[0] = source;
  rec[2] = n_p;
  rec[3] = (int32_t)t;
  if (N < n_p) {
    rec[1] = -1;
    return;
  }
  for (int i = 0; i < n_p; ++i) {
    fake_centre(im, source, i, t, &cen[2 * i], &cen[2 * i + 1]);
    rec[4 + 2 * i] = cen[2 * i];
    rec[4 + 2 * i + 1] = cen[2 * i + 1];
  }
  if (source == NPP_DEV_SRC_SAME) {
    float* w = (float*)(rec + record_weights_at(n_p, topk));
    for (int i = 0; i < n_p; ++i) w[i] = 1.0f;
    rec[1] = 1;
    return;
  }
  for (int p = 0; p < n_p; ++p) {
    int keys[kCand];
    cnt[p] = 0;
    for (int idx = 0; idx < kCand; ++idx) {
      keys[idx] = cand_key(im, cen[2 * p], cen[2 * p + 1], idx);
      cnt[p] += keys[idx] != kNoCand;
    }
    for (int r = 0; r < topk; ++r) {
      int best = kNoCand, at = -1;
      for (int idx = 0; idx < kCand; ++idx)
        if (keys[idx] < best) best = keys[idx], at = idx;
      if (at >= 0) keys[at] = kNoCand;
      sel[p * topk + r] = best;
    }
  }
  const int k = final_k(cnt, n_p, topk);
  rec[1] = k;
  for (int p = 0; k > 0 && p < n_p; ++p) write_real(im, sel, cnt, n_p, topk, k, p, cen[2 * p], cen[2 * p + 1], rec);
}

static bool decide_args_ok(const void* imgs, int M, const uint32_t* t, int n_p, int topk, const void* rec, int64_t rec_stride,
                           const char* what) {
  // (the LDS of the launch: n_p (topk + 3) ints, kept under 32 KiB)
  if (!imgs || !t || !rec || M < 1 || n_p < 1 || topk < 1 || (int64_t)n_p * (topk + 3) > 8192 ||
      rec_stride < record_words(n_p, topk)) {
    set_error("%s: bad argument (M=%d n_p=%d topk=%d rec_stride=%lld, need >= %lld; n_p (topk + 3) <= 8192)", what, M, n_p, topk,
              (long long)rec_stride, (long long)record_words(n_p > 0 ? n_p : 0, topk > 0 ? topk : 0));
    return false;
  }
  return true;
}

}  // namespace npp

using namespace npp;

extern "C" int64_t npp_dev_sampler_record_words(int n_p, int topk) {
  return n_p < 0 || topk < 0 ? NPP_ERR_ARG : devs::record_words(n_p, topk);
}

extern "C" int npp_dev_sampler_decide(const npp_dev_image* d_imgs, int M, const uint32_t* h_t, int n_p, int topk, int32_t* d_rec,
                                      int64_t rec_stride, void* stream) {
  if (!decide_args_ok(d_imgs, M, h_t, n_p, topk, d_rec, rec_stride, "npp_dev_sampler_decide")) return NPP_ERR_ARG;
  const size_t lds = (size_t)n_p * (topk + 3) * sizeof(int);
  for (int m0 = 0; m0 < M; m0 += NPP_DEV_MAX_IMAGES) {
    const int mc = M - m0 < NPP_DEV_MAX_IMAGES ? M - m0 : NPP_DEV_MAX_IMAGES;
    DevTs ts = {};
    for (int i = 0; i < mc; ++i) ts.t[i] = h_t[m0 + i];
    hipLaunchKernelGGL(dev_decide_kernel, dim3((unsigned)mc), dim3(kDecideThreads), lds, (hipStream_t)stream, d_imgs + m0, ts, n_p,
                       topk, d_rec + (int64_t)m0 * rec_stride, rec_stride);
  }
  return check_launch("npp_dev_sampler_decide");
}

extern "C" int npp_dev_sampler_decide_host(const npp_dev_image* imgs, int M, const uint32_t* t, int n_p, int topk, int32_t* rec,
                                           int64_t rec_stride) {
  if (!decide_args_ok(imgs, M, t, n_p, topk, rec, rec_stride, "npp_dev_sampler_decide_host")) return NPP_ERR_ARG;
  int* tmp = new int[(size_t)n_p * (topk + 3)];
  for (int m = 0; m < M; ++m)
    decide_host_one(imgs[m], t[m], n_p, topk, rec + (int64_t)m * rec_stride, tmp, tmp + n_p, tmp + n_p + (size_t)n_p * topk);
  delete[] tmp;
  return NPP_OK;
}

extern "C" int npp_dev_sampler_pixels(const npp_dev_image* d_imgs, int M, const uint32_t* h_t, int64_t n_pix, int64_t* d_pix,
                                      int64_t pix_stride, void* stream) {
  if (!d_imgs || !h_t || !d_pix || M < 1 || n_pix < 1 || pix_stride < n_pix || n_pix > ((int64_t)1 << 31)) {
    set_error("npp_dev_sampler_pixels: bad argument (M=%d n_pix=%lld pix_stride=%lld)", M, (long long)n_pix, (long long)pix_stride);
    return NPP_ERR_ARG;
  }
  for (int m0 = 0; m0 < M; m0 += NPP_DEV_MAX_IMAGES) {
    const int mc = M - m0 < NPP_DEV_MAX_IMAGES ? M - m0 : NPP_DEV_MAX_IMAGES;
    DevTs ts = {};
    for (int i = 0; i < mc; ++i) ts.t[i] = h_t[m0 + i];
    hipLaunchKernelGGL(dev_pixels_kernel, dim3((unsigned)((n_pix + 255) / 256), (unsigned)mc), dim3(256), 0, (hipStream_t)stream,
                       d_imgs + m0, ts, n_pix, d_pix + (int64_t)m0 * pix_stride, pix_stride);
  }
  return check_launch("npp_dev_sampler_pixels");
}

extern "C" int npp_dev_sampler_pixels_host(const npp_dev_image* imgs, int M, const uint32_t* t, int64_t n_pix, int64_t* pix,
                                           int64_t pix_stride) {
  if (!imgs || !t || !pix || M < 1 || n_pix < 1 || pix_stride < n_pix) {
    set_error("npp_dev_sampler_pixels_host: bad argument (M=%d n_pix=%lld pix_stride=%lld)", M, (long long)n_pix, (long long)pix_stride);
    return NPP_ERR_ARG;
  }
  for (int m = 0; m < M; ++m) {
    if (n_pix > imgs[m].n_train) {
      set_error("npp_dev_sampler_pixels_host: image %d: cannot draw %lld of %lld without replacement", m, (long long)n_pix,
                (long long)imgs[m].n_train);
      return NPP_ERR_ARG;
    }
    for (int64_t j = 0; j < n_pix; ++j)
      pix[(int64_t)m * pix_stride + j] = devs::perm_index(imgs[m].n_train, j, t[m], 2u, imgs[m].seed_lo, imgs[m].seed_hi);
  }
  return NPP_OK;
}

extern "C" int npp_dev_philox4x32_10(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4) {
  if (!ctr4 || !key2 || !out4) {
    set_error("npp_dev_philox4x32_10: null argument");
    return NPP_ERR_ARG;
  }
  const devs::U4 r = devs::philox4x32_10(devs::U4{ctr4[0], ctr4[1], ctr4[2], ctr4[3]}, key2[0], key2[1]);
  out4[0] = r.x, out4[1] = r.y, out4[2] = r.z, out4[3] = r.w;
  return NPP_OK;
}

extern "C" int npp_dev_perm_host(uint64_t seed, uint32_t t, uint32_t stream, int64_t N, int64_t n, int64_t* out) {
  if (!out || N < 1 || N > ((int64_t)1 << 32) || n < 0 || n > N) {
    set_error("npp_dev_perm_host: bad argument (N=%lld n=%lld: 1 <= N <= 2^32, 0 <= n <= N)", (long long)N, (long long)n);
    return NPP_ERR_ARG;
  }
  for (int64_t j = 0; j < n; ++j) out[j] = devs::perm_index(N, j, t, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
  return NPP_OK;
}
