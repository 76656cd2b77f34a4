// npp_stash_census.h -- census of the 8-bit training stash (include/npp_hip.h "stash audit"): how many of the
// bytes an iteration left in actF's W8 region and in dzF's bf8 arrays sit at the limits of their format.  Included by npp_api.hip
// only: the array table depends on NPP_WIDTH, and that source is compiled once per width.
//
// The table is derived from the layout's own k-step offsets (npp_layout.h kAct* / kDz*) and make_desc(K).present -- the arrays
// npp_mlp_fwd / npp_mlp_bwd write for this K, in the order they lie in memory.  A census never writes the stash and the hot
// kernels carry no counters: it is a scan of what they left.
#pragma once
#include "npp_census.h"

namespace npp {

enum CensusKind : int { kCensusAll = 0, kCensusEmb, kCensusRgb };   // which of an array's 16 nks feature slots are real
constexpr int kCensusMaxArrays = 12 + NPP_MAX_K + 13;

struct CensusArray {
  int32_t side;       // 0: actF's W8 region (fp8 e4m3), 1: dzF (bf8 e5m2) -- the side fixes the format
  int32_t ks0, nks;   // k-step offset and length (array base = wfmt8_array_base(ks0, n_wg))
  int32_t kind;       // CensusKind
  int32_t features;   // real features per row
};
struct CensusDesc {
  int32_t n;
  CensusArray a[kCensusMaxArrays];
};

// names[i] (optional): at least 12 chars each
inline CensusDesc make_census_desc(int K, char (*names)[12] = nullptr) {
  const NetDesc d = make_desc(K);
  CensusDesc c{};
  auto add = [&](int present, int side, int ks0, int nks, int kind, int features, const char* fmt, int idx) {
    if (!present) return;
    if (names) snprintf(names[c.n], 12, fmt, idx);
    c.a[c.n++] = CensusArray{side, ks0, nks, kind, features};
  };
  for (int l = L0; l <= L7; ++l) add(d.present[l], 0, l * kKSAct, kKSAct, kCensusAll, kW, "a%d", l);        // snake(z_l): the next layer's input
  add(d.present[LF1], 0, kActF1 * kKSAct, kKSAct, kCensusAll, kW, "f1", 0);
  add(d.present[LS], 0, kActAS * kKSAct, kKSAct, kCensusAll, kW, "a_s", 0);
  add(d.present[LF2], 0, kActF2 * kKSAct, kKSAct, kCensusAll, kW, "f2", 0);
  add(d.present[LP], 0, kActKsAP, kKSAct / 2, kCensusAll, kW / 2, "a_p", 0);
  for (int p = 0; p < K; ++p) add(1, 0, kActKsEmb0 + p * kKSEmb, kKSEmb, kCensusEmb, kE, "emb%d", p);
  for (int l = L0; l <= L7; ++l) add(d.present[l], 1, l * kKSAct, kKSAct, kCensusAll, kW, "dz%d", l);
  add(d.present[LF1], 1, kDzF1 * kKSAct, kKSAct, kCensusAll, kW, "dz_f1", 0);
  add(d.present[LS], 1, kDzS * kKSAct, kKSAct, kCensusAll, kW, "dz_s", 0);
  add(d.present[LF2], 1, kDzF2 * kKSAct, kKSAct, kCensusAll, kW, "dz_f2", 0);
  add(d.present[LP], 1, kDzKsP, kKSAct / 2, kCensusAll, kW / 2, "dz_p", 0);
  add(d.present[LRGB], 1, kDzKsRgb, 2, kCensusRgb, 3, "dz_rgb", 0);
  return c;
}

// bit j: element j of unit (ks, hh) is a real feature of the array
NPP_HD uint32_t census_jmask(int kind, int ks, int hh) {
  if (kind == kCensusAll) return 0xffu;
  if (kind == kCensusRgb) return (ks == 0 && hh == 0) ? 0x07u : 0u;      // npp_mlp_bwd.hip: dL/draw in elements 0..2 of the first unit
  uint32_t m = 0;
  for (int j = 0; j < 8; ++j) m |= (emb_col(ks, hh, j) >= 0 ? 1u : 0u) << j;
  return m;
}

NPP_HD CensusFmt census_fmt(int side) { return side ? kFmtE5M2 : kFmtE4M3; }

struct CensusArgs {
  const uint8_t* act8;          // actF + act8_region_base(K, n_wg)
  const uint8_t* dz8;           // dzF
  int64_t n_wg, n_rows;
  unsigned long long* rec;
  CensusDesc d;
};

// grid: (x: slices of an array's 16-byte pieces, y: array; y == d.n: the tile scale words); counted by CensusLane (npp_census.h)
__global__ __launch_bounds__(kCensusThreads) void stash8_census_kernel(CensusArgs A) {
  __shared__ CensusHist sHist[kCensusWaves];
  __shared__ uint32_t sPart[kCensusWaves][kCensusEntry];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int a = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * kCensusThreads;
  if (a == A.d.n) {                                                     // ---- dzF's per-tile scale words (tiles with a real row)
    const int32_t* sc = (const int32_t*)(A.dz8 + dz8_scale_base(A.n_wg));
    const int64_t tiles = (A.n_rows + kRowTile - 1) / kRowTile;
    uint32_t cnt = 0;
    int mn = 255, mx = 0;
    for (int64_t g = (int64_t)blockIdx.x * kCensusThreads + tid; g < tiles; g += stride) {
      const int s = sc[g] & 255;
      ++cnt; mn = min(mn, s); mx = max(mx, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      cnt += __shfl_xor(cnt, off, 64); mn = min(mn, __shfl_xor(mn, off, 64)); mx = max(mx, __shfl_xor(mx, off, 64));
    }
    if (lane == 0) { sPart[wave][0] = cnt; sPart[wave][1] = (uint32_t)mn; sPart[wave][2] = (uint32_t)mx; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long c = 0;
      int lo = 255, hi = 0;
      for (int w = 0; w < kCensusWaves; ++w) { c += sPart[w][0]; lo = min(lo, (int)sPart[w][1]); hi = max(hi, (int)sPart[w][2]); }
      if (c) {
        long long* t = (long long*)(A.rec + (int64_t)A.d.n * kCensusEntry);
        atomicAdd((unsigned long long*)t + NPP_CENSUS_TILES, c);
        atomicMin(t + NPP_CENSUS_SCALE_MIN, (long long)lo);
        atomicMax(t + NPP_CENSUS_SCALE_MAX, (long long)hi);
      }
    }
    return;
  }
  const CensusArray ar = A.d.a[a];
  const int64_t nq = (int64_t)ar.nks * A.n_wg * 64;                    // 16-byte pieces of the array (1 KiB per k-step and tile)
  if ((int64_t)blockIdx.x * kCensusThreads >= nq) return;
  const uint8_t* base = (ar.side ? A.dz8 : A.act8) + wfmt8_array_base(ar.ks0, A.n_wg);
  const CensusFmt F = census_fmt(ar.side);
  CensusLane L(sHist);
  L.clear();
  // the bytes of piece q that count: rows < n_rows, real features (wfmt8_unit16_decode: two rows x the 8 elements of one unit)
  auto valid = [&](int64_t q) -> uint32_t {
    if (q >= nq) return 0u;
    int64_t wg; int ks, row64, hh;
    wfmt8_unit16_decode(ar.nks, q, wg, ks, row64, hh);
    const int64_t row = wg * kRowTile + row64;
    const uint32_t jm = census_jmask(ar.kind, ks, hh);
    return (row < A.n_rows ? jm : 0u) | (row + 1 < A.n_rows ? jm << 8 : 0u);
  };
  // a piece with only some of its bytes counted (the ragged last rows, embedding padding, dz_rgb): byte by byte
  auto count = [&](const u32x4& v, uint32_t vm) {
    L.n_el += __popc(vm);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if ((vm >> i) & 1u) {
        const CensusClass k = census_classify(F, (v[i >> 2] >> (8 * (i & 3))) & F.mask);
        L.n_zero += k.zero;
        L.n_max += k.at_max;
        if (k.nonfinite) ++L.n_nf;
        else L.add(k.bin);
      }
    }
  };
  // a whole piece (nearly all of them), without a branch: every byte goes to the bin of its exponent field (one bit-field extract,
  // one LDS add) -- the non-finite codes with it, taken out again below: e5m2's fill bin 31 and nothing else does, e4m3's NaN sits
  // in bin 15 and is counted here -- and zero / at_max / NaN are counted four bytes at a time: (x & 0x7f..) + 0x7f.. sets bit 7 of a
  // byte exactly when its low seven bits are not all zero (0x7f + 0x7f does not carry)
  const uint32_t max4 = F.max_code * 0x01010101u;
  const uint32_t ebits = 7u - F.mbits;
  auto zero_bytes = [](uint32_t x7) -> uint32_t { return 4u - __popc((x7 + 0x7f7f7f7fu) & 0x80808080u); };
  auto count_all = [&](const u32x4& v) {
    L.n_el += 16u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t x = v[w], x7 = x & 0x7f7f7f7fu;
      L.n_zero += zero_bytes(x7);
      L.n_max += zero_bytes(x7 ^ max4);
      if (ar.side == 0) L.n_nan += zero_bytes(x7 ^ 0x7f7f7f7fu);
#pragma unroll
      for (int k = 0; k < 4; ++k) L.add(__builtin_amdgcn_ubfe(x, 8u * k + F.mbits, ebits));
    }
  };
  for (int64_t q = (int64_t)blockIdx.x * kCensusThreads + tid; q < nq; q += 2 * stride) {
    const uint32_t vm0 = valid(q), vm1 = valid(q + stride);
    u32x4 v0 = u32x4{0, 0, 0, 0}, v1 = v0;
    if (vm0) v0 = *(const u32x4*)(base + q * 16);                        // both requested before either is counted
    if (vm1) v1 = *(const u32x4*)(base + (q + stride) * 16);
    if (vm0 == 0xffffu) count_all(v0); else if (vm0) count(v0, vm0);
    if (vm1 == 0xffffu) count_all(v1); else if (vm1) count(v1, vm1);
  }
  L.finish<0>(sHist, sPart, ar.side == 0, nullptr, A.rec + (int64_t)a * kCensusEntry);
}

inline int64_t census_words(int K) { return (int64_t)make_census_desc(K).n * kCensusEntry + NPP_CENSUS_TILE_WORDS; }

// plain C++ twin on host copies of the same bytes: walks (row, k-step, lane half, element) through the FORWARD map wfmt8_unit
inline void stash8_census_host(const uint8_t* act8, const uint8_t* dz8, int64_t n_wg, int64_t n_rows, int K, int64_t* rec) {
  const CensusDesc d = make_census_desc(K);
  for (int64_t i = 0; i < (int64_t)d.n * kCensusEntry + NPP_CENSUS_TILE_WORDS; ++i) rec[i] = 0;
  for (int a = 0; a < d.n; ++a) {
    const CensusArray& ar = d.a[a];
    const CensusFmt F = census_fmt(ar.side);
    const uint8_t* base = (ar.side ? dz8 : act8) + wfmt8_array_base(ar.ks0, n_wg);
    int64_t* r = rec + (int64_t)a * kCensusEntry;
    for (int64_t row = 0; row < n_rows; ++row)
      for (int ks = 0; ks < ar.nks; ++ks)
        for (int hh = 0; hh < 2; ++hh) {
          const uint32_t jm = census_jmask(ar.kind, ks, hh);
          const uint8_t* u = base + wfmt8_unit(ar.nks, row / kRowTile, ks, (int)(row % kRowTile), hh);
          for (int j = 0; j < 8; ++j)
            if ((jm >> j) & 1u) census_tally(F, u[j] & F.mask, r);
        }
  }
  int64_t* t = rec + (int64_t)d.n * kCensusEntry;
  const int32_t* sc = (const int32_t*)(dz8 + dz8_scale_base(n_wg));
  const int64_t tiles = (n_rows + kRowTile - 1) / kRowTile;
  t[NPP_CENSUS_TILES] = tiles;
  t[NPP_CENSUS_SCALE_MIN] = 255; t[NPP_CENSUS_SCALE_MAX] = 0;
  for (int64_t g = 0; g < tiles; ++g) {
    const int64_t s = sc[g] & 255;
    if (s < t[NPP_CENSUS_SCALE_MIN]) t[NPP_CENSUS_SCALE_MIN] = s;
    if (s > t[NPP_CENSUS_SCALE_MAX]) t[NPP_CENSUS_SCALE_MAX] = s;
  }
}

}  // namespace npp
