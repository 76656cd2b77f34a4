// npp_chain16.h -- the building blocks of the fused 16-bit chains (v_mfma_f32_32x32x16_bf16, fp32 accumulation), the counterpart of
// npp_chain32.h.  GEMMs are transposed (Z^T = W X^T): the weights are the A operand, the activations the B operand.
//   fragment     16 bytes per lane = 8 bf16 features of one pixel row: lane (b, h) of k-step ks holds features 16 ks + perm16(h, j)
//                of row b -- an accumulator tile converted to bf16 (pack_acc) IS two fragments of the next layer
//   region       the B operands of one layer in LDS: [k-step][batch tile of 32 rows][lane] fragments (lds_frag / lds_store_frag)
//   ring slot    the A fragments of one k-step for a wave's NTW neuron tiles, in registers; kRD slots roll over the packed weights
//                [k-step][neuron tile][lane] of a part and on into the next part's (WRing, mma_ring)
//   W-format unit  a fragment's place in a stash array in global memory (npp_layout.h wfmt_unit; 8-byte W8 units: wfmt8_unit), laid out
//                so that npp_mlp_wgrad copies tiles linearly into LDS and reads them transposed (wfrag_offset / wfrag_read)
// Included by npp_mlp_fwd.hip, npp_mlp_bwd.hip, npp_mlp_wgrad.hip (the main loop's coordinate MLP), npp_light16.hip (NPP_Net_light's
// training chains) and npp_api.hip (the MFMA self-test and the pack kernels).
#pragma once
#include "npp_common.h"

namespace npp {

__device__ __forceinline__ bf16x8 pack_acc(const f32x16& acc, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)acc[8 * s + j];
  return r;
}

__device__ __forceinline__ f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// Streaming store of a 16-byte fragment to a stash array: written once, read once by a later
// kernel, so it should not displace the L2-resident weight packs (NPP_STASH_NT=0 to compare).
#ifndef NPP_STASH_NT
#define NPP_STASH_NT 1
#endif
__device__ __forceinline__ void stash_store(void* p, const bf16x8& v) {
#if NPP_STASH_NT
  __builtin_nontemporal_store(v, (bf16x8*)p);
#else
  *(bf16x8*)p = v;
#endif
}
// Pre-activation gradients (npp_mlp_bwd -> npp_mlp_wgrad, the next launch): NPP_DZ_NT=0 lets them allocate in the caches
#ifndef NPP_DZ_NT
#define NPP_DZ_NT NPP_STASH_NT
#endif
__device__ __forceinline__ void dz_store(void* p, const bf16x8& v) {
#if NPP_DZ_NT
  __builtin_nontemporal_store(v, (bf16x8*)p);
#else
  *(bf16x8*)p = v;
#endif
}
// ---- 8-bit stash helpers (npp_layout.h "W8-format") --------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(8))) int i32x8;
// v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 turn a finite value beyond the format's range into NaN / infinity unless MODE.FP16_OVFL is
// set, in which case they saturate (0x7e = 448 / 0x7b = 57344; tools/micro/fp8_probe.hip, round 6).  Kernels that write the 8-bit
// stash set the bit once at entry (it also makes the fp16 z stash saturate instead of overflowing to infinity).
__device__ __forceinline__ void set_fp16_ovfl() { asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1"); }
// 8 consecutive accumulator registers (or any 8 floats) -> the 8 bytes of a W8 unit
__device__ __forceinline__ u32x2 pack8_fp8(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(v2, v3, lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v4, v5, 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(v6, v7, hi, true);
  return u32x2{(uint32_t)lo, (uint32_t)hi};
}
__device__ __forceinline__ u32x2 pack8_bf8(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
  int lo = __builtin_amdgcn_cvt_pk_bf8_f32(v0, v1, 0, false);
  lo = __builtin_amdgcn_cvt_pk_bf8_f32(v2, v3, lo, true);
  int hi = __builtin_amdgcn_cvt_pk_bf8_f32(v4, v5, 0, false);
  hi = __builtin_amdgcn_cvt_pk_bf8_f32(v6, v7, hi, true);
  return u32x2{(uint32_t)lo, (uint32_t)hi};
}
__device__ __forceinline__ u32x2 pack8_bf8_acc(const f32x16& a, int s) {
  return pack8_bf8(a[8 * s], a[8 * s + 1], a[8 * s + 2], a[8 * s + 3], a[8 * s + 4], a[8 * s + 5], a[8 * s + 6], a[8 * s + 7]);
}
__device__ __forceinline__ u32x2 pack8_fp8_bf16(const bf16x8& f) {
  return pack8_fp8((float)f[0], (float)f[1], (float)f[2], (float)f[3], (float)f[4], (float)f[5], (float)f[6], (float)f[7]);
}
// snake'(z) = 1 + sin 2z in [0, 2] as one unsigned byte: u = round(127.5 * snake'(z)) (error <= 1 / 255, the size of the bf16
// rounding of the operand it multiplies); what the backward chain reads in stash8 mode instead of the fp16 pre-activation.
// v_cvt_pk_u8_f32 rounds to nearest even and saturates to [0, 255] (NaN -> 0): measured on gfx950, round 6.
constexpr float kSd8Scale = 127.5f, kSd8Inv = 1.0f / 127.5f;
__device__ __forceinline__ uint32_t pack4_u8(float v0, float v1, float v2, float v3) {
  uint32_t x = __builtin_amdgcn_cvt_pk_u8_f32(v0, 0u, 0u);
  x = __builtin_amdgcn_cvt_pk_u8_f32(v1, 1u, x);
  x = __builtin_amdgcn_cvt_pk_u8_f32(v2, 2u, x);
  return __builtin_amdgcn_cvt_pk_u8_f32(v3, 3u, x);
}
__device__ __forceinline__ float u8_byte_f32(uint32_t w, int j) {       // byte j of w as a float (v_cvt_f32_ubyteN)
  return (float)((w >> (8 * j)) & 255u);
}
__device__ __forceinline__ void stash8_store(void* p, const u32x2& v) {
#if NPP_STASH_NT
  __builtin_nontemporal_store(v, (u32x2*)p);
#else
  *(u32x2*)p = v;
#endif
}
// Pre-activations of the snake layers are stashed as fp16 (|z| is O(10); 11 significand bits):
// the backward chain derives snake'(z) = 1 + sin 2z from them and npp_mlp_wgrad derives the layer
// input snake(z) while staging -- ONE 16-bit array per layer instead of two.
__device__ __forceinline__ f16x8 pack_acc_f16(const f32x16& acc, int s) {
  f16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (_Float16)acc[8 * s + j];
  return r;
}
__device__ __forceinline__ void stash_store(void* p, const f16x8& v) {
#if NPP_STASH_NT
  __builtin_nontemporal_store(v, (f16x8*)p);
#else
  *(f16x8*)p = v;
#endif
}

// ---- W-format operand tiles in LDS (npp_layout.h wfmt_unit) ---------------------------
// A 16-KiB tile = 4 k-step pairs (128 features) x 2 batch tiles x 2 KiB of one 64-row
// workgroup tile, copied linearly from global memory.  wfrag_offset() is the byte offset of
// the first of the two ds_read_b64_tr_b16 that build, for this lane, the MFMA operand
// fragment "feature (lane & 31) of 32-feature tile tt, batch rows 16 t + 8 (lane >> 5) + 0..7"
// (t = 0..3 indexes the four 16-row k-steps of the 64 rows); the second read is 256 B on.
// Lane 4q+p of each 16-lane group addresses row q, feature quad p (cdna_hip_programming.md
// T10); within a 32-lane half the 32 addresses tile one 256-byte line: conflict-free.
__device__ __forceinline__ int wfrag_offset(int tt, int t, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, h = g >> 1;
  return ((tt * 2 + (t >> 1)) * 8 + 4 * (t & 1) + 2 * h) * 256 + (g & 1) * 128 + (p & 1) * 64 + q * 16 + (p >> 1) * 8;
}
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
__device__ __forceinline__ bf16x8 wfrag_read(const char* tile, int off) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(tile + off));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(tile + off + 256));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// ---- shared pieces of the fused chains -------------------------------------------------
struct Lane {
  int tid, wave, lane, b, h;
  int n_wg;             // 64-row workgroup tiles of THIS image's batch (gridDim.x of a plain launch): the W-format array geometry
  int xslot, xcount;    // this workgroup's index among / the number of the image's workgroups on its XCD (weight-pack requests)
};
__device__ __forceinline__ bf16x8 lds_frag(const char* region, int ks, int bt, int lane) {
  return *(const bf16x8*)(region + ((ks * kNB + bt) * 64 + lane) * 16);
}
__device__ __forceinline__ void lds_store_frag(char* region, int ks, int bt, int lane, const bf16x8& v) {
  *(bf16x8*)(region + ((ks * kNB + bt) * 64 + lane) * 16) = v;
}

// ---- weight stream: a rolling register ring of 4 k-steps --------------------------------
// With only Bp/64 workgroups in flight the kernel is latency-bound unless the L2 -> register
// weight stream runs ahead of the MFMAs.  Each wave keeps the weight fragments of the next
// 4 k-steps in a ring; right after the MFMAs of k-step ks have been issued, their slot is
// refilled with k-step ks+4 (16 MFMAs = 512+ cycles ahead).  The ring runs across part and
// layer boundaries (next_wp), so loads also fly under the epilogue and the barrier; START
// is the (compile-time) slot of this part's first k-step.
#ifndef NPP_RING_DEPTH
#define NPP_RING_DEPTH 4
#endif
constexpr int kRD = NPP_RING_DEPTH;     // k-steps of weight fragments in flight per wave
// The packed weights are addressed through ONE buffer descriptor (SGPRs, npp_common.h make_wrsrc) per kernel: a part of a
// layer is a wave-uniform offset into the pack (wptr_t, 16-byte units), the lane supplies only
// its constant 16-byte voffset, so a refill costs no vector ALU work at all (flat loads needed a
// 64-bit VALU add per k-step: ~1.2k of the ~9.6k VALU instructions a wave issued per tile).
using wptr_t = uint32_t;
constexpr wptr_t kNoW = 0xffffffffu;      // "no next part": the ring is not refilled past this part
template <int NTW>
struct WRing {
  bf16x8 w[kRD][NTW];
  wrsrc_t rsrc;
};

template <int NTW, int NT>
__device__ __forceinline__ void wslot_load(WRing<NTW>& r, int slot, wptr_t wp, int ks, int nt0, int lane) {
  typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const u32x4_t raw = __builtin_amdgcn_raw_buffer_load_b128(r.rsrc, lane * 16, (int)((wp + (uint32_t)((ks * NT + nt0 + nt) * 64)) * 16u), 0);
    r.w[slot][nt] = __builtin_bit_cast(bf16x8, raw);
  }
}
// fresh fill of the ring with k-steps 0..3 of wp (START = 0 for the consumer)
template <int NTW, int NT>
__device__ __forceinline__ void wring_fill(WRing<NTW>& r, wptr_t wp, int nt0, int lane) {
#pragma unroll
  for (int q = 0; q < kRD; ++q) wslot_load<NTW, NT>(r, q, wp, q, nt0, lane);
}

// Ring schedule positions [KS0, KS1) of a part with KSREAL real k-steps (weights at wp) padded
// to KSTOT (a multiple of 4) schedule positions, so that every part starts at ring slot 0:
// positions >= KSREAL issue no MFMA and load nothing, they only keep the refill cadence.
// Activation fragments of k-step ks sit at LDS k-step (ks - KS0 + ks_lds0) of `region`.
#ifndef NPP_SLICE_VALU_PER_GAP
#define NPP_SLICE_VALU_PER_GAP 4
#endif
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};
// `hook(ks - KS0)` is called once per schedule position, between the activation-fragment reads
// and the MFMAs: independent VALU / LDS work placed there (the embedding generator) issues in
// the shadow of the MFMAs of the same wave.
// SLICED: the hook emits a small, branch-free slice per position (a handful of VALU / LDS instructions); the scheduler is
// then told to place it INSIDE the position's MFMA run -- one MFMA, a share of the slice, one MFMA, ... -- instead of the
// blob-after-four-MFMAs it produces by itself (MI355X_MICROARCH.md: <= 5 single-issue instructions hide per MFMA gap).
template <int KS0, int KS1, int KSREAL, int KSTOT, int NTW, int NT, typename Hook = NoHook, bool SLICED = false>
__device__ __forceinline__ void mma_ring(f32x16 (&acc)[NTW][kNB], const char* region, int ks_lds0,
                                         wptr_t wp, wptr_t next_wp, int nt0,
                                         const Lane& L, WRing<NTW>& ring, const Hook& hook = Hook()) {
  static_assert(KSTOT % kRD == 0 && KSREAL <= KSTOT && KS1 <= KSTOT, "ring schedule");
  // activation fragments are read one k-step ahead of the MFMAs that use them (LDS latency
  // ~130+ cycles would otherwise serialise every k-step behind its own reads)
  constexpr int KSE = KS1 < KSREAL ? KS1 : KSREAL;       // real k-steps end
  bf16x8 xn[kNB];
  if (KS0 < KSE) {
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt) xn[bt] = lds_frag(region, ks_lds0, bt, L.lane);
  }
#pragma unroll
  for (int ks = KS0; ks < KS1; ++ks) {
    const int slot = ks % kRD;
    if (ks < KSREAL) {
      bf16x8 x[kNB];
#pragma unroll
      for (int bt = 0; bt < kNB; ++bt) x[bt] = xn[bt];
      if (ks + 1 < KSE) {
#pragma unroll
        for (int bt = 0; bt < kNB; ++bt) xn[bt] = lds_frag(region, ks_lds0 + ks + 1 - KS0, bt, L.lane);
      }
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int bt = 0; bt < kNB; ++bt) acc[nt][bt] = mfma_bf16(ring.w[slot][nt], x[bt], acc[nt][bt]);
    }
    hook(ks - KS0);
    if (ks + kRD < KSREAL) wslot_load<NTW, NT>(ring, slot, wp, ks + kRD, nt0, L.lane);
    else if (ks + kRD >= KSTOT && next_wp != kNoW) wslot_load<NTW, NT>(ring, slot, next_wp, ks + kRD - KSTOT, nt0, L.lane);
    if (SLICED && ks < KSREAL) {
#pragma unroll
      for (int g = 0; g < NTW * kNB; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, NPP_SLICE_VALU_PER_GAP, 0);   // its share of the slice's VALU work
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                        // and of the LDS reads (slice + next fragments)
      }
    }
    asm volatile("" ::: "memory");   // pin the refill here: no hoisting of later loads
  }
}

// ---- forward: the bias as the initial accumulator ------------------------------------------------------------------------------
// Neuron (within the wave's 32-neuron tile) of accumulator element idx for this lane: the 32x32x16 map (npp_layout.h acc_row) or,
// M16, that of the four 16 x 16 tiles npp_mlp_fwd.hip's NPP_FWD_MFMA16 form keeps in the same registers.
template <bool M16>
__device__ __forceinline__ int acc_row_map(int idx, const Lane& L) {
  return M16 ? 16 * (idx >> 3) + 4 * (L.lane >> 4) + (idx & 3) : acc_row(idx, L.h);
}
// acc[nt][bt] <- bias of this wave's neuron tiles (row constants as the initial accumulator)
template <int NTW, bool M16 = false>
__device__ __forceinline__ void init_bias(f32x16 (&acc)[NTW][kNB], const float* __restrict__ bias, int nt0,
                                          const Lane& L) {
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    f32x16 bv;
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[r] = bias[(nt0 + nt) * 32 + acc_row_map<M16>(r, L)];
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt) acc[nt][bt] = bv;
  }
}

// The same in two halves: the NEXT layer's bias values are fetched before the current layer's epilogue (their L2 latency
// hides under it and the barrier) and moved into the accumulators where init_bias used to load them.
template <int NTW> struct BiasPre { float v[NTW][16]; };
template <int NTW, bool M16 = false>
__device__ __forceinline__ void bias_fetch(BiasPre<NTW>& bp, const float* __restrict__ bias, int nt0, const Lane& L) {
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) bp.v[nt][r] = bias[(nt0 + nt) * 32 + acc_row_map<M16>(r, L)];
}
template <int NTW>
__device__ __forceinline__ void bias_apply(f32x16 (&acc)[NTW][kNB], const BiasPre<NTW>& bp) {
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][bt][r] = bp.v[nt][r];
}

// ---- backward: data-gradient accumulators and their epilogue ------------------------------------------------------------------
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][kNB]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][bt][r] = 0.0f;
}

// The z fragments a layer's epilogue needs (stash, cold in HBM), fetched BEFORE the layer's MFMA loop so that their
// latency is covered by it instead of stalling every epilogue (32 VGPRs).
// S8 (stash8): the forward left snake'(z) itself, one unsigned byte per element in the W8-format (kSd8Scale): 8-byte
// units, no sine here
template <bool S8> struct ZPre { f16x8 z[2][kNB][2]; };
template <> struct ZPre<true> { u32x2 z[2][kNB][2]; };
template <bool S8>
__device__ __forceinline__ void z_prefetch(ZPre<S8>& zp, const char* z_array, int wg, int kt0, const Lane& L) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if constexpr (S8) zp.z[t][bt][s] = *(const u32x2*)(z_array + wfmt8_unit(kKSAct, wg, 2 * (kt0 + t) + s, 32 * bt + L.b, L.h));
        else zp.z[t][bt][s] = *(const f16x8*)(z_array + wfmt_unit(kKSAct, wg, 2 * (kt0 + t) + s, bt, L.b, L.h));
      }
}

// dz = acc (x stashed snake derivative); fragments -> LDS for the next dgrad, rows -> dzT.
template <bool HAS_S, bool S8>
__device__ __forceinline__ void bwd_epilogue(f32x16 (&acc)[2][kNB], char* out, const ZPre<S8>* zp, char* dz_array,
                                             int wg, int kt0, const Lane& L) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ntg = kt0 + t;
#pragma unroll
    for (int bt = 0; bt < kNB; ++bt) {
      f32x16 g = acc[t][bt];
      if (HAS_S) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if constexpr (S8) {
            const u32x2 sd = zp->z[t][bt][s];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[8 * s + j] *= u8_byte_f32(sd[j >> 2], j & 3) * kSd8Inv;
          } else {
            const f16x8 zf = zp->z[t][bt][s];
#pragma unroll
            for (int j = 0; j < 8; ++j)      // snake'(z) = 1 + sin 2z  (activations.py:29-35)
              g[8 * s + j] *= 1.0f + __builtin_amdgcn_sinf((float)zf[j] * (2.0f * kInv2Pi));
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 f = pack_acc(g, s);
        if (out) lds_store_frag(out, 2 * ntg + s, bt, L.lane, f);
        if (S8) stash8_store(dz_array + wfmt8_unit(kKSAct, wg, 2 * ntg + s, 32 * bt + L.b, L.h), pack8_bf8_acc(g, s));
        else dz_store(dz_array + wfmt_unit(kKSAct, wg, 2 * ntg + s, bt, L.b, L.h), f);
      }
    }
  }
}

}  // namespace npp
