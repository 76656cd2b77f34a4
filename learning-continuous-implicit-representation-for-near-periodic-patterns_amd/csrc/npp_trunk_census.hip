// npp_trunk_census.hip -- census of a stored fp16 trunk tensor (include/npp_hip.h "trunk audit"): how many of
// the values a forward pass of the trunk kernels (npp_conv.hip, npp_conv_pair.hip) left in ONE flat padded activation tensor sit at
// the limits of fp16, and -- against the exact-fp32 trunk's tensor of the same layer (npp_conv32.hip) -- how many ReLU gates the two
// disagree on.  npp_conv.hip's numeric contract is what is counted: fp16 activations saturated at +-65504 without a flag, gates
// taken from the fp16 values.  A census never writes the tensor and the hot kernels carry no counters: it is a scan of what they left.
//
// Layout (npp_trunk_layout.h / npp_conv.hip): [C/8 chunks][nposp][8] fp16, position kConvGuard + img (H+2)(W+2) + y (W+2) + x with a
// one-pixel border per image, element j of chunk c8 = true channel conv_chan(c8, j).  The kernel walks a chunk's positions linearly
// and INVERTS that map (position -> image, y, x; interior or not); the host twin walks (image, channel, y, x) through the FORWARD
// map: the two check each other.
#include "npp_census.h"
#include "npp_trunk_layout.h"

namespace npp {

constexpr int kTcWords = NPP_TRUNK_CENSUS_WORDS;

// bit j: element j of chunk c8 is one of the c_real true channels (the trunk input x0 carries 3 of its 16)
NPP_HD uint32_t trunk_census_jmask(int c8, int c_real) {
  uint32_t m = 0;
  for (int j = 0; j < 8; ++j) m |= (conv_chan(c8, j) < c_real ? 1u : 0u) << j;
  return m;
}
// (fp16 value > 0) from the code: positive sign, not zero, not NaN -- the gate the data-gradient launches take ([y > 0])
NPP_HD bool f16_code_positive(uint32_t c) { return !(c & 0x8000u) && (c & kFmtF16.mask) != 0u && (c & kFmtF16.mask) <= kFmtF16.nonfinite_from; }

struct TrunkCensusArgs {
  const u32x4* act;             // the flat tensor
  const float* ref;             // nullable: (>= n, c_real, H, W) fp32
  unsigned long long* rec;
  int64_t nposp;                // units per chunk
  int32_t n, c_real, H, W;
};

// grid: (x: slices of a chunk's positions, y: chunk); counted by CensusLane (npp_census.h), the two gate counters as its extra words
__global__ __launch_bounds__(kCensusThreads) void trunk16_census_kernel(TrunkCensusArgs A) {
  __shared__ CensusHist sHist[kCensusWaves];
  __shared__ uint32_t sPart[kCensusWaves][kTcWords];
  const int tid = threadIdx.x;
  const int c8 = blockIdx.y;
  const uint32_t jm = trunk_census_jmask(c8, A.c_real);
  if (!jm) return;                                                      // a chunk of padded channels only (uniform per workgroup)
  const uint32_t Wp = (uint32_t)A.W + 2u, S = ((uint32_t)A.H + 2u) * Wp;
  const uint32_t npos = (uint32_t)A.n * S;                             // (<= nposp < 2^21: the launcher's geometry check)
  const uint32_t stride = gridDim.x * kCensusThreads;
  if (blockIdx.x * kCensusThreads >= npos) return;
  const u32x4* base = A.act + (int64_t)c8 * A.nposp + kConvGuard;
  CensusLane L(sHist);
  L.clear();
  uint32_t gate[2] = {0, 0};                                            // NPP_TRUNK_CENSUS_GATE_ON, _GATE_FLIPS
  // position p of the image axis -> (image, y, x) of the padded image; 0 when it is a border position (or past the counted images)
  auto interior = [&](uint32_t p, uint32_t& img, uint32_t& y, uint32_t& x) -> bool {
    if (p >= npos) return false;
    img = p / S;
    const uint32_t r = p - img * S;
    y = r / Wp;
    x = r - y * Wp;
    return y >= 1u && y <= (uint32_t)A.H && x >= 1u && x <= (uint32_t)A.W;
  };
  auto count = [&](const u32x4& v, uint32_t img, uint32_t y, uint32_t x) {
    L.n_el += __popc(jm);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!((jm >> j) & 1u)) continue;                                  // (uniform: jm is the workgroup's)
      const uint32_t c = (v[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      const CensusClass k = census_classify(kFmtF16, c & kFmtF16.mask);
      L.n_zero += k.zero;
      L.n_max += k.at_max;
      L.add(k.bin);            // every code goes to the bin of its exponent field -- the non-finite ones (field 31) with it: finish()
      if (A.ref) {
        const float f = A.ref[(((int64_t)img * A.c_real + conv_chan(c8, j)) * A.H + (y - 1u)) * A.W + (x - 1u)];
        const bool on = f16_code_positive(c);
        gate[0] += on;
        gate[1] += on != (f > 0.0f);
      }
    }
  };
  for (uint32_t p = blockIdx.x * kCensusThreads + tid; p < npos; p += 2 * stride) {
    uint32_t i0 = 0, y0 = 0, x0 = 0, i1 = 0, y1 = 0, x1 = 0;
    const bool in0 = interior(p, i0, y0, x0), in1 = interior(p + stride, i1, y1, x1);
    u32x4 v0 = u32x4{0, 0, 0, 0}, v1 = v0;
    if (in0) v0 = base[p];                                              // both requested before either is counted
    if (in1) v1 = base[p + stride];
    if (in0) count(v0, i0, y0, x0);
    if (in1) count(v1, i1, y1, x1);
  }
  L.finish<2>(sHist, sPart, false, gate, A.rec);
}

// plain C++ twin on host copies: (image, chunk, element, y, x) through the FORWARD map of the layout
static void trunk16_census_host(const uint16_t* act, int n, int C, int c_real, int H, int W, int64_t nposp, const float* ref,
                                int64_t* rec) {
  for (int i = 0; i < kTcWords; ++i) rec[i] = 0;
  const int64_t S = (int64_t)(H + 2) * (W + 2);
  for (int img = 0; img < n; ++img)
    for (int c8 = 0; c8 < C / 8; ++c8)
      for (int j = 0; j < 8; ++j) {
        const int ch = conv_chan(c8, j);
        if (ch >= c_real) continue;
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            const int64_t pos = kConvGuard + img * S + (int64_t)(y + 1) * (W + 2) + (x + 1);
            const uint32_t c = act[((int64_t)c8 * nposp + pos) * 8 + j];
            if (ref) {
              const bool on = f16_code_positive(c);
              rec[NPP_TRUNK_CENSUS_GATE_ON] += on;
              rec[NPP_TRUNK_CENSUS_GATE_FLIPS] += on != (ref[(((int64_t)img * c_real + ch) * H + y) * W + x] > 0.0f);
            }
            census_tally(kFmtF16, c & kFmtF16.mask, rec);
          }
      }
}

}  // namespace npp

using namespace npp;

static int trunk_census_check(const char* who, const void* act, int N_total, int n, int C, int c_real, int H, int W, const float* ref,
                              const void* rec) {
  if (N_total < 1 || H < 1 || W < 1 || W + 3 > kConvGuard || conv_nposp(N_total, H, W) * 16 * 64 > 0x7fffffffLL) {
    set_error("%s: bad geometry N=%d H=%d W=%d (W <= %d, one launch's tensor size)", who, N_total, H, W, kConvGuard - 3);
    return NPP_ERR_ARG;
  }
  if (n < 1 || n > N_total || C < 16 || C % 16 || c_real < 1 || c_real > C) {
    set_error("%s: bad n=%d (1..N_total=%d) / C=%d (a multiple of 16) / c_real=%d (1..C)", who, n, N_total, C, c_real);
    return NPP_ERR_ARG;
  }
  if (!act || !rec || ((uintptr_t)act & 15) || ((uintptr_t)rec & 7) || ((uintptr_t)ref & 3)) {
    set_error("%s: null or misaligned pointer (tensor 16-byte, record 8-byte, fp32 partner 4-byte aligned)", who);
    return NPP_ERR_ARG;
  }
  return NPP_OK;
}

extern "C" int64_t npp_trunk16_census_words(void) { return kTcWords; }

extern "C" int npp_trunk16_census(const void* d_act, int N_total, int n, int C, int c_real, int H, int W, const float* d_ref32,
                                  int64_t* d_record, void* stream) {
  int rc = trunk_census_check("npp_trunk16_census", d_act, N_total, n, C, c_real, H, W, d_ref32, d_record);
  if (rc) return rc;
  TrunkCensusArgs A{};
  A.act = (const u32x4*)d_act; A.ref = d_ref32; A.rec = (unsigned long long*)d_record;
  A.nposp = conv_nposp(N_total, H, W);
  A.n = n; A.c_real = c_real; A.H = H; A.W = W;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_record, 0, (size_t)kTcWords * 8, s);
  if (e != hipSuccess) { set_error("npp_trunk16_census: hipMemsetAsync: %s", hipGetErrorString(e)); return NPP_ERR_LAUNCH; }
  // two 16-byte units in flight per lane and pass; about 2048 workgroups at most over the chunks (few atomics per counter)
  const int chunks = C / 8;
  const int64_t npos = (int64_t)n * (H + 2) * (W + 2);
  const int64_t want = (npos + 2 * kCensusThreads - 1) / (2 * kCensusThreads), cap = 2048 / chunks > 1 ? 2048 / chunks : 1;
  const unsigned gx = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
  hipLaunchKernelGGL(trunk16_census_kernel, dim3(gx, (unsigned)chunks), dim3(kCensusThreads), 0, s, A);
  return check_launch("npp_trunk16_census");
}

extern "C" int npp_trunk16_census_host(const void* act, int N_total, int n, int C, int c_real, int H, int W, const float* ref32,
                                       int64_t* record) {
  int rc = trunk_census_check("npp_trunk16_census_host", act, N_total, n, C, c_real, H, W, ref32, record);
  if (rc) return rc;
  trunk16_census_host((const uint16_t*)act, n, C, c_real, H, W, conv_nposp(N_total, H, W), ref32, record);
  return NPP_OK;
}
