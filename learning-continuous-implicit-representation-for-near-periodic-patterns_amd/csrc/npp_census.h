// npp_census.h -- the census core of the audits (DESIGN.md section 6j "census core"): what one entry of a census record counts --
// NPP_CENSUS_ELEMENTS .. NPP_CENSUS_NONFINITE, then NPP_CENSUS_BINS exponent bins -- for a format given as a CensusFmt, and how a
// workgroup counts it.  npp_stash_census.h (e4m3, e5m2) and npp_trunk_census.hip (fp16) keep their own walks over the data.
#pragma once
#include "npp_common.h"

namespace npp {

constexpr int kCensusThreads = 256, kCensusWaves = kCensusThreads / 64;
constexpr int kCensusEntry = NPP_CENSUS_ENTRY_WORDS, kCensusHist = NPP_CENSUS_HIST, kCensusBins = NPP_CENSUS_BINS;

// a format, sign dropped: mantissa bits, the largest finite code, the first non-finite code, the mask that drops the sign
struct CensusFmt { uint32_t mbits, max_code, nonfinite_from, mask; };
constexpr CensusFmt kFmtE4M3{3u, 0x7Eu, 0x7Fu, 0x7Fu};              // OCP: 0x7E = 448, 0x7F NaN, no infinity
constexpr CensusFmt kFmtE5M2{2u, 0x7Bu, 0x7Cu, 0x7Fu};              // 0x7B = 57344, 0x7C infinity, 0x7D..0x7F NaN
constexpr CensusFmt kFmtF16{10u, 0x7BFFu, 0x7C00u, 0x7FFFu};        // 0x7BFF = 65504, 0x7C00 infinity, above it NaN

// the classes of one sign-dropped code; bin is its exponent field (a non-finite code has one too: e4m3's 15, the others' 31)
struct CensusClass { bool nonfinite, zero, subnormal, at_max; uint32_t bin; };
NPP_HD CensusClass census_classify(const CensusFmt& F, uint32_t c) {
  const uint32_t bin = c >> F.mbits;
  return CensusClass{c >= F.nonfinite_from, c == 0u, c != 0u && bin == 0u, c == F.max_code, bin};
}

// the host twins' step: one counted code into the entry r (a non-finite code is in no bin)
inline void census_tally(const CensusFmt& F, uint32_t c, int64_t* r) {
  const CensusClass k = census_classify(F, c);
  ++r[NPP_CENSUS_ELEMENTS];
  if (k.nonfinite) { ++r[NPP_CENSUS_NONFINITE]; return; }
  r[NPP_CENSUS_ZERO] += k.zero; r[NPP_CENSUS_SUBNORMAL] += k.subnormal; r[NPP_CENSUS_AT_MAX] += k.at_max;
  ++r[kCensusHist + k.bin];
}

using CensusHist = uint32_t[kCensusBins][64];
// One lane's share of a workgroup's census.  Every lane counts in a column of its own (registers + 32 LDS words [bin][lane]: its bank
// is its lane, no conflict whatever the data), finish() sums the columns per wave and the waves in LDS, and the workgroup issues one
// 64-bit integer atomic per non-zero word.  sHist: kCensusWaves CensusHist.
struct CensusLane {
  uint32_t* col;
  uint32_t n_el = 0, n_zero = 0, n_max = 0, n_nf = 0, n_nan = 0;    // n_nan: non-finite codes that add() put into bin 15 (e4m3)

  __device__ explicit CensusLane(CensusHist* sHist) : col(&sHist[threadIdx.x >> 6][0][threadIdx.x & 63]) {}
  __device__ void clear() {
#pragma unroll
    for (int b = 0; b < kCensusBins; ++b) col[b * 64] = 0;
  }
  __device__ void add(uint32_t bin) {                                 // (no other lane adds here)
    __hip_atomic_fetch_add(col + bin * 64, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  // Behind the counting loop, by the whole workgroup.  The non-finite codes that went into the histogram leave it: those of bin 15
  // by their count n_nan (nan15, e4m3), else all of bin 31 (e5m2, fp16: nothing finite is there).  extra: kExtra more lane counters,
  // summed and flushed as the words behind the entry.  sPart: kCensusWaves rows of kCensusEntry + kExtra words; rec: the entry.
  template <int kExtra>
  __device__ void finish(const CensusHist* sHist, uint32_t (*sPart)[kCensusEntry + kExtra], bool nan15, uint32_t* extra,
                         unsigned long long* rec) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __syncthreads();
    // the wave's 64 columns -> 32 bin totals: lane l sums bin l & 31 over half the columns, skewed so that the 64 lanes read 64 banks
    uint32_t s = 0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) s += sHist[wave][lane & 31][(lane >> 5) * 32 + ((k + lane) & 31)];
    s += __shfl_xor(s, 32, 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      n_el += __shfl_xor(n_el, off, 64); n_zero += __shfl_xor(n_zero, off, 64); n_max += __shfl_xor(n_max, off, 64);
      n_nf += __shfl_xor(n_nf, off, 64); n_nan += __shfl_xor(n_nan, off, 64);
#pragma unroll
      for (int i = 0; i < kExtra; ++i) extra[i] += __shfl_xor(extra[i], off, 64);
    }
    if (nan15) {
      n_nf += n_nan;
      if ((lane & 31) == 15) s -= n_nan;
    } else {
      n_nf += __shfl(s, 31, 64);
      if ((lane & 31) == 31) s = 0;
    }
    if (lane < kCensusBins) sPart[wave][kCensusHist + lane] = s;
    if (lane == 0) {
      sPart[wave][NPP_CENSUS_ELEMENTS] = n_el; sPart[wave][NPP_CENSUS_ZERO] = n_zero; sPart[wave][NPP_CENSUS_SUBNORMAL] = 0;
      sPart[wave][NPP_CENSUS_AT_MAX] = n_max; sPart[wave][NPP_CENSUS_NONFINITE] = n_nf;
#pragma unroll
      for (int i = 0; i < kExtra; ++i) sPart[wave][kCensusEntry + i] = extra[i];
    }
    __syncthreads();
    if (tid < kCensusEntry + kExtra) {
      unsigned long long t = 0;                       // exponent field 0 holds the zeros and the subnormals: subnormal = that bin - zero
      for (int w = 0; w < kCensusWaves; ++w) t += tid == NPP_CENSUS_SUBNORMAL ? sPart[w][kCensusHist] - sPart[w][NPP_CENSUS_ZERO] : sPart[w][tid];
      if (t) atomicAdd(rec + tid, t);
    }
  }
};

}  // namespace npp
