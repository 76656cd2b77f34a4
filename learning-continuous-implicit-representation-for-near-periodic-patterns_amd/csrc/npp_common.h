// npp_common.h -- what every gfx950 translation unit may need: the vector types, the host error plumbing and THE launch of a
// dynamic-LDS kernel, the tunables, snake, the LDS-only workgroup barrier, the buffer descriptor of a packed weight stream and the
// work-item decode of the stacked launches.  By topic elsewhere: npp_chain16.h / npp_chain32.h (the fused 16-bit / exact-fp32
// chains), npp_adam.h, npp_robust.h (adaptive pixel loss, ordered reduction), npp_coord.h (embedder maths, coordinate intake).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "npp_layout.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

namespace npp {

// host-side error plumbing (npp_api.cpp)
void set_error(const char* fmt, ...);
int check_launch(const char* what);
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE setting of a kernel: SmemOnce remembers which devices of this
// process already have it (bit d of the mask), so a second GPU driven from the same process is set up as well.
struct SmemOnce { unsigned long long done = 0; };
bool smem_attr(SmemOnce& once, const void* fn, int bytes);

// THE launch of a kernel with dynamic LDS.  Kern is a template argument, so the once-flag below exists once per kernel
// instantiation, wherever it is launched from.  lds_limit is what the kernel's dynamic-LDS limit is raised to, once per device:
// the launch's own lds_bytes, or the largest any launch of Kern asks for where lds_bytes varies (the limit is set only once);
// 0 leaves the default 48 KiB alone (sites that raise it only above that pass `bytes > kLdsDefault ? limit : 0`).
// who: the entry point's name in the error text.  Returns check_launch(who).
constexpr int kLdsDefault = 48 * 1024;
template <auto Kern, typename... Args>
int launch_lds(const char* who, dim3 grid, dim3 block, size_t lds_bytes, int lds_limit, hipStream_t stream, const Args&... args) {
  static SmemOnce once;
  if (lds_limit && !smem_attr(once, (const void*)Kern, lds_limit)) { set_error("%s: smem attribute", who); return NPP_ERR_LAUNCH; }
  hipLaunchKernelGGL(Kern, grid, block, lds_bytes, stream, args...);
  return check_launch(who);
}

// Launch-time choices between kernel forms that compute the same result (npp_tune(); defaults = the measured-best forms).  Read
// with relaxed loads by the launchers; an environment variable of the upper-cased name prefixed NPP_ (NPP_CONV_WINK=0) sets the
// initial value, so that tools can A/B whole processes, and npp_tune() flips it inside one process (parity tests, probes).
struct Tunables {
  int conv_wink;      // 1: group-split window convolution on the channel-rich trunk layers; 0: never; 2: wherever feasible
  int conv_win;       // 1: window-staged convolution on conv1_1 / conv1_2 / conv2_1 forward; 0: never; 2: wherever feasible
  int conv_wstat;     // 1: weight-stationary block numbering where the pack outweighs the activations; 0: never
  int conv_pair;      // bit mask of the fused convolution pairs (conv a -> conv b -> pool) the trunks use: 1 = first block, 2 = second, 4 = the first block's data gradient, 8 = patch plumbing + pixel loss inside the first pair; 0: never
  int light_det;      // 1 (default): the proposal-ranking fits' fp32 weight-gradient launch does not split its contraction (no float atomics on the gradient path: bit-reproducible fits); 0: split-K by atomicAdd
  int stash8;         // 1 (default): the training stash that feeds the weight gradients is 8-bit (bf8 gradients with a per-tile power-of-two scale, fp8 layer inputs; npp_layout.h "W8-format") and npp_mlp_wgrad runs on v_mfma_scale_f32_32x32x64_f8f6f4; 0: the round-2..5 16-bit stash and bf16 weight-gradient launch.  Read by npp_mlp_fwd* / npp_mlp_bwd* / npp_mlp_wgrad* at launch: flip it only between complete iterations
};
extern Tunables g_tune;

constexpr float kInv2Pi = 0.15915494309189535f;

// ---- a6: snake and its derivative (models/activations.py:29-35, a = 1) -----------
__device__ __forceinline__ float snake_fast(float z) {
  const float s = __builtin_amdgcn_sinf(z * kInv2Pi);
  return fmaf(s, s, z);
}
__device__ __forceinline__ void snake_fast2(float z, float& a, float& da) {
  const float rev = z * kInv2Pi;
  const float s = __builtin_amdgcn_sinf(rev);
  const float c = __builtin_amdgcn_cosf(rev);
  a = fmaf(s, s, z);
  da = fmaf(2.0f * s, c, 1.0f);                    // 1 + sin(2z)
}

// Workgroup barrier for LDS hand-offs that leaves global memory traffic in flight.
// __syncthreads() makes hipcc emit s_waitcnt vmcnt(0) first, which drains every outstanding
// stash store and weight prefetch at each of the ~30 barriers of the fused kernels (measured:
// 54 % of wave time in SQ_WAIT_ANY).  Only LDS operations (lgkmcnt) need to have completed
// before the other waves may read what this wave wrote; loads into registers are still
// waited for by the compiler at their first use.
__device__ __forceinline__ void wg_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Packed weights (the fused chains, the trunk convolutions) are addressed through ONE buffer descriptor (SGPRs) per kernel: the
// lane supplies a constant voffset, the part of the pack is a wave-uniform offset, so a load costs no vector ALU work.
using wrsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ wrsrc_t make_wrsrc(const void* pack, int64_t units16) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(pack), 0, (int)(units16 * 16), 0x00020000);
}

// ---- stacked launches (round 4): M independent images of one shape in every launch -----------------------------------------
// The reference loops its images serially (run_completion.sh:8-14); their fits are independent (own weights, Adam state, RNG),
// so M of them ride in one launch sequence: every buffer of the single-image path gets a leading image dimension with a fixed
// stride, and what differs per image and per iteration (patch source, k, Adam step) sits in a small device array the host uploads
// once per iteration (npp_stack_iter, include/npp_hip.h).  Work items are numbered so that an image's workgroups stay on 8 / M of
// the 8 XCDs (workgroups go round-robin over the XCDs by linear id -- observed, speed only): each XCD's 4-MiB L2 then keeps ONE
// image's 3.9-MB weight pack, as in the single-image launch, instead of M of them.
struct StackIter {                 // == npp_stack_iter
  int32_t active, k, comp, with_lp;
  int32_t x0, nk, same, pad1;      // x0: first image of this fit's prediction half in the stacked trunk batch; nk = n_p * k
  float step_size, inv_sqrt_bc2, pad2, pad3;
};
static_assert(sizeof(StackIter) == 48, "npp_stack_iter layout");
struct Stack {
  int32_t M;                       // 0: a plain single-image launch (blockIdx.x = work item)
  int32_t g;                       // XCDs per image (8 / M for M in {1, 2, 4, 8}), 0: images back to back in launch order
  int32_t n_items;                 // work items per image
  int32_t pad;
  const StackIter* iter;           // nullable: every image active
};
inline Stack make_stack(int M, int n_items, const void* d_iter) {
  Stack S{};
  S.M = M; S.n_items = n_items; S.iter = (const StackIter*)d_iter;
  S.g = (M == 1 || M == 2 || M == 4 || M == 8) ? 8 / M : 0;
  return S;
}
inline unsigned stack_grid(const Stack& S) {
  return S.g ? 8u * (unsigned)((S.n_items + S.g - 1) / S.g) : (unsigned)S.M * (unsigned)S.n_items;
}
// (image, item) of this workgroup; false: surplus workgroup of the rounded-up grid or an image that sits the iteration out
__device__ __forceinline__ bool stack_decode(const Stack& S, int& img, int& item, int& xslot, int& xcount) {
  const int b = (int)blockIdx.x;
  if (S.M == 0) { img = 0; item = b; xslot = b >> 3; xcount = ((int)gridDim.x + 7) >> 3; return true; }
  if (S.g) {
    const int xcd = b & 7, slot = b >> 3;
    img = xcd / S.g;
    item = slot * S.g + xcd % S.g;
    xslot = slot; xcount = (S.n_items + S.g - 1) / S.g;
  } else {
    img = b / S.n_items;
    item = b - img * S.n_items;
    xslot = item >> 3; xcount = (S.n_items + 7) >> 3;
  }
  if (item >= S.n_items) return false;
  return S.iter == nullptr || S.iter[img].active != 0;
}

}  // namespace npp
