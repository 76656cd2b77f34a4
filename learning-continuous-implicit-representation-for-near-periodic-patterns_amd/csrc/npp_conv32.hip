// npp_conv32.hip -- the trunks of the patch losses in exact fp32 (trunk_precision = "fp32"): conv3x3 (padding 1, stride 1) as an
// implicit GEMM on v_mfma_f32_32x32x2_f32, MaxPool2d(2,2) forward / backward, all on plain fp32 NCHW tensors.
//
// The default trunks (npp_conv.hip) keep fp16 activations and bf16 gradients; this file is the diagnostic twin that runs the
// same stacks (externel_lib/contextual_loss/modules/vgg.py:30-36, externel_lib/lpips/pretrained_networks.py:119-134,
// models/style_loss.py:11-14) in the reference's own arithmetic: every product is rounded once and accumulated in fp32 in a
// fixed order (the MFMA is a k-ordered fmaf chain), no float atomics, and a workgroup only ever reads one image -- so results
// are bit-reproducible and an image's result does not depend on its batch.
//
// GEMM view of one launch: D[m][pixel] = sum_{kch, tap} A[m][kch, tap] * X[kch][pixel + tap], m = output channel.
//   A operand of lane l = A[m = l & 31][k = l >> 5]      (the weight pack, one float per lane)
//   B operand of lane l = B[k = l >> 5][pixel = l & 31]  (32 pixels of one (channel, tap) out of the LDS halo tile)
//   D: pixel = l & 31 on the lane, m = (r & 3) + 8 (r >> 2) + 4 (l >> 5) in the 16 registers.
// No column matrix exists anywhere: the nine taps are nine shifted reads of the same LDS tile.
//
// Tile: a workgroup of 4 waves owns 256 pixels of one image (8 groups of 32 pixels, two per wave; a group is 32 / TW rows of
// TW columns, TW = 32, 16 or 8 chosen from the image width) x 64 output channels (two 32-row A tiles; one for the 3-channel
// image gradient): four independent accumulators per wave.  K runs in chunks of 8 input channels: the (rows + 2) x (TW + 2)
// halo tile of the chunk and its 8 x 9 x 64 weights are staged in LDS, then 9 taps x 4 channel pairs x 4 MFMAs.
// Summation order per output element: channel chunk, tap (row-major), channel -- fixed by the code, the same for every launch.
#include "npp_common.h"

namespace npp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int C32_CK = 8;                 // input channels per K chunk
constexpr int C32_TILE_MAX = 340;         // halo tile floats per channel: 10 x 34 (TW 32), 18 x 18 (TW 16), 34 x 10 (TW 8)
constexpr int C32_WTILE = 9 * 4 * 2 * 32; // pack floats per (32 output channels, K chunk): [tap][channel pair][k][m]

struct conv32_args {
  const float* x; const float* pack; const float* bias; const float* in_gate; const float* gate; const float* add; float* y;
  int H, W, K, M;          // K input channels, M output channels of THIS launch (the data gradient swaps the layer's)
  int mode, ltw, tiles_x;  // log2(TW)
  int has_in_norm;
  float in_scale[3], in_shift[3], out_scale[3];
};

template <int NCT>
__global__ __launch_bounds__(256) void conv32_kernel(const conv32_args a) {
  __shared__ float lds_x[C32_CK * C32_TILE_MAX];
  __shared__ float lds_w[NCT * C32_WTILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int tw = 1 << a.ltw, rpg = 32 >> a.ltw;             // tile width, rows per pixel group
  const int bh = 8 * rpg, ldx = tw + 2, tile = (bh + 2) * ldx;
  const int ty0 = (blockIdx.x / a.tiles_x) * bh, tx0 = (blockIdx.x % a.tiles_x) * tw;
  const int mt0 = blockIdx.y * NCT;
  const int n = blockIdx.z;
  const int H = a.H, W = a.W, K = a.K, M = a.M;
  const int64_t hw = (int64_t)H * W;
  const int KC = (K + C32_CK - 1) / C32_CK;
  const float* xin = a.x + (int64_t)n * K * hw;
  const float* gin = a.in_gate ? a.in_gate + (int64_t)n * K * hw : nullptr;
  // this lane's pixel in the wave's two groups (tile coordinates)
  int py[2], px;
  px = j & (tw - 1);
  py[0] = (2 * wave) * rpg + (j >> a.ltw);
  py[1] = (2 * wave + 1) * rpg + (j >> a.ltw);
  f32x16 acc[NCT][2];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][g][r] = 0.0f;

  for (int kc = 0; kc < KC; ++kc) {
    __syncthreads();                                         // the previous chunk's MFMAs have read both tiles
    for (int c = 0; c < C32_CK; ++c) {
      const int ch = kc * C32_CK + c;
      for (int idx = tid; idx < tile; idx += 256) {
        const int yy = idx / ldx, xx = idx - yy * ldx;
        const int gy = ty0 + yy - 1, gx = tx0 + xx - 1;
        float v = 0.0f;                                      // zero padding of conv2d(padding=1), channels past K, tile overhang
        if (ch < K && gy >= 0 && gy < H && gx >= 0 && gx < W) {
          const int64_t off = (int64_t)ch * hw + (int64_t)gy * W + gx;
          v = xin[off];
          if (a.has_in_norm) v = v * a.in_scale[ch] + a.in_shift[ch];   // the NORMALISED image is what torch zero-pads
          if (gin) v = gin[off] > 0.0f ? v : 0.0f;           // ReLU gate of the tapped top layer
        }
        lds_x[c * tile + idx] = v;
      }
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const float4* src = reinterpret_cast<const float4*>(a.pack + ((int64_t)(mt0 + ct) * KC + kc) * C32_WTILE);
      float4* dst = reinterpret_cast<float4*>(lds_w + ct * C32_WTILE);
      for (int idx = tid; idx < C32_WTILE / 4; idx += 256) dst[idx] = src[idx];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = t / 3, dx = t % 3;
      const int o0 = (py[0] + dy) * ldx + px + dx, o1 = (py[1] + dy) * ldx + px + dx;
#pragma unroll
      for (int kp = 0; kp < 4; ++kp) {
        const float* xs = lds_x + (kp * 2 + h) * tile;
        const float b0 = xs[o0], b1 = xs[o1];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const float av = lds_w[ct * C32_WTILE + ((t * 4 + kp) * 2 + h) * 32 + j];
          acc[ct][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[ct][0], 0, 0, 0);
          acc[ct][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[ct][1], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: lane = pixel, registers = 16 output channels
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int gy = ty0 + py[g], gx = tx0 + px;
    if (gy >= H || gx >= W) continue;
    const int64_t pix = (int64_t)gy * W + gx;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (mt0 + ct) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m >= M) continue;
        const int64_t off = ((int64_t)n * M + m) * hw + pix;
        float v = acc[ct][g][r];
        if (a.mode == 0) {                                   // nn.Conv2d + nn.ReLU
          v += a.bias[m];
          v = v > 0.0f ? v : 0.0f;
        } else if (a.mode == 1) {                            // dL/d(pre-activation) of the layer below (or dL/d(pooled tensor))
          if (a.add) v += a.add[off];
          if (a.gate) v = a.gate[off] > 0.0f ? v : 0.0f;
        } else {                                             // dL/dimage: times the input scale
          v *= a.out_scale[m];
        }
        a.y[off] = v;
      }
    }
  }
}

// torch Conv2d weight (Cout, Cin, 3, 3) -> [M tiles of 32][K chunks of 8][tap][channel pair][k][m], zero padded.
// which = 0: M = Cout, K = Cin, tap t.  which = 1 (data gradient): M = Cin, K = Cout, tap 8 - t (transposed, flipped).
__global__ void conv32_pack_kernel(const float* __restrict__ w, int Cin, int Cout, int which, float* __restrict__ pack, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int M = which ? Cin : Cout, K = which ? Cout : Cin;
  const int KC = (K + C32_CK - 1) / C32_CK;
  const int i = (int)(e & 31), h = (int)((e >> 5) & 1), kp = (int)((e >> 6) & 3);
  const int64_t rest = e >> 8;                               // (mt * KC + kc) * 9 + t
  const int t = (int)(rest % 9);
  const int64_t mk = rest / 9;
  const int kc = (int)(mk % KC), mt = (int)(mk / KC);
  const int m = mt * 32 + i, kch = kc * C32_CK + kp * 2 + h;
  float v = 0.0f;
  if (m < M && kch < K) v = which ? w[((int64_t)kch * Cin + m) * 9 + (8 - t)] : w[((int64_t)m * Cin + kch) * 9 + t];
  pack[e] = v;
}

__global__ void maxpool2_fwd32_kernel(const float* __restrict__ x, int64_t total, int H, int W, int Ho, int Wo, float* __restrict__ y) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int xo = (int)(e % Wo), yo = (int)((e / Wo) % Ho);
  const int64_t nc = e / ((int64_t)Wo * Ho);
  const float* p = x + nc * H * W + (int64_t)(2 * yo) * W + 2 * xo;
  float best = p[0];
  if (p[1] > best) best = p[1];
  if (p[W] > best) best = p[W];
  if (p[W + 1] > best) best = p[W + 1];
  y[e] = best;
}

// one thread per element of the PRE-pool tensor: no two threads write one address, no atomics
__global__ void maxpool2_bwd32_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ add,
                                      int64_t total, int H, int W, int Ho, int Wo, int gate, float* __restrict__ dz) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int xi = (int)(e % W), yi = (int)((e / W) % H);
  const int64_t nc = e / ((int64_t)W * H);
  const int yo = yi >> 1, xo = xi >> 1;
  float v = 0.0f;
  if (yo < Ho && xo < Wo) {                                  // (odd sizes floor: the last row / column is in no window)
    const float* p = x + nc * H * W + (int64_t)(2 * yo) * W + 2 * xo;
    int arg = 0;                                             // first maximum in row-major window order
    float best = p[0];
    if (p[1] > best) { best = p[1]; arg = 1; }
    if (p[W] > best) { best = p[W]; arg = 2; }
    if (p[W + 1] > best) { best = p[W + 1]; arg = 3; }
    if (arg == (yi & 1) * 2 + (xi & 1)) v = dy[(nc * Ho + yo) * Wo + xo];
  }
  if (add) v += add[e];
  if (gate) v = x[e] > 0.0f ? v : 0.0f;
  dz[e] = v;
}

static bool conv32_channels_ok(int c) { return c == 3 || c == 64 || c == 128 || c == 256 || c == 512; }

static int64_t conv32_pack_floats(int Cin, int Cout, int which) {
  const int M = which ? Cin : Cout, K = which ? Cout : Cin;
  return (int64_t)((M + 31) / 32) * ((K + C32_CK - 1) / C32_CK) * C32_WTILE;
}

}  // namespace npp

using namespace npp;

extern "C" int64_t npp_conv32_pack_bytes(int Cin, int Cout, int which) {
  if (!conv32_channels_ok(Cin) || !conv32_channels_ok(Cout) || Cout == 3 || (which != 0 && which != 1)) {
    set_error("npp_conv32_pack_bytes: bad argument (Cin=%d Cout=%d which=%d)", Cin, Cout, which);
    return NPP_ERR_ARG;
  }
  return conv32_pack_floats(Cin, Cout, which) * (int64_t)sizeof(float);
}

extern "C" int npp_conv32_pack(const float* d_w, int Cin, int Cout, float* d_pack_fwd, float* d_pack_bwd, void* stream) {
  if (!d_w || (!d_pack_fwd && !d_pack_bwd) || !conv32_channels_ok(Cin) || !conv32_channels_ok(Cout) || Cout == 3) {
    set_error("npp_conv32_pack: bad argument (Cin=%d Cout=%d)", Cin, Cout);
    return NPP_ERR_ARG;
  }
  float* out[2] = {d_pack_fwd, d_pack_bwd};
  for (int which = 0; which < 2; ++which) {
    if (!out[which]) continue;
    const int64_t total = conv32_pack_floats(Cin, Cout, which);
    hipLaunchKernelGGL(conv32_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_w, Cin, Cout,
                       which, out[which], total);
    const int rc = check_launch("npp_conv32_pack");
    if (rc != NPP_OK) return rc;
  }
  return NPP_OK;
}

extern "C" int npp_conv32(const float* d_x, int N_total, int n_run, int H, int W, int Cin, int Cout, const float* d_pack, int mode,
                          const float* d_bias, const float in_scale[3], const float in_shift[3], const float* d_in_gate,
                          const float* d_gate, const float* d_add, const float out_scale[3], float* d_y, void* stream) {
  const bool chan_ok = mode == 0 ? (conv32_channels_ok(Cin) && conv32_channels_ok(Cout) && Cout != 3)
                     : mode == 1 ? (conv32_channels_ok(Cin) && conv32_channels_ok(Cout) && Cin != 3 && Cout != 3)
                                 : (conv32_channels_ok(Cin) && Cin != 3 && Cout == 3);
  if (!d_x || !d_pack || !d_y || mode < 0 || mode > 2 || !chan_ok || H < 1 || W < 1 || n_run < 0 || n_run > N_total ||
      n_run > 65535 || (mode == 0 && !d_bias) || (mode == 2 && !out_scale) || (mode != 0 && (in_scale || in_shift)) ||
      ((in_scale != nullptr) != (in_shift != nullptr)) || (in_scale && Cin != 3) || (mode != 1 && (d_gate || d_add)) ||
      (mode == 0 && d_in_gate)) {
    set_error("npp_conv32: bad argument (mode=%d N_total=%d n_run=%d H=%d W=%d Cin=%d Cout=%d)", mode, N_total, n_run, H, W, Cin, Cout);
    return NPP_ERR_ARG;
  }
  if (n_run == 0) return NPP_OK;
  conv32_args a;
  a.x = d_x; a.pack = d_pack; a.bias = d_bias; a.in_gate = d_in_gate; a.gate = d_gate; a.add = d_add; a.y = d_y;
  a.H = H; a.W = W; a.K = Cin; a.M = Cout; a.mode = mode;
  a.ltw = W > 16 ? 5 : (W > 8 ? 4 : 3);
  const int tw = 1 << a.ltw, bh = 8 * (32 >> a.ltw);
  a.tiles_x = (W + tw - 1) / tw;
  const int64_t tiles = (int64_t)a.tiles_x * ((H + bh - 1) / bh);
  if (tiles > 0x7fffffff) {
    set_error("npp_conv32: image too large (H=%d W=%d)", H, W);
    return NPP_ERR_ARG;
  }
  a.has_in_norm = in_scale != nullptr;
  for (int c = 0; c < 3; ++c) {
    a.in_scale[c] = in_scale ? in_scale[c] : 1.0f;
    a.in_shift[c] = in_shift ? in_shift[c] : 0.0f;
    a.out_scale[c] = out_scale ? out_scale[c] : 1.0f;
  }
  const int MT = (Cout + 31) / 32;
  if (MT % 2 == 0)
    hipLaunchKernelGGL(conv32_kernel<2>, dim3((unsigned)tiles, MT / 2, n_run), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(conv32_kernel<1>, dim3((unsigned)tiles, MT, n_run), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("npp_conv32");
}

extern "C" int npp_maxpool2_fwd32(const float* d_x, int N_total, int n_run, int H, int W, int C, float* d_y, void* stream) {
  if (!d_x || !d_y || H < 1 || W < 1 || C < 1 || n_run < 0 || n_run > N_total) {
    set_error("npp_maxpool2_fwd32: bad argument (N_total=%d n_run=%d H=%d W=%d C=%d)", N_total, n_run, H, W, C);
    return NPP_ERR_ARG;
  }
  const int Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)n_run * C * Ho * Wo;
  if (total == 0) return NPP_OK;
  if ((total + 255) / 256 > 0x7fffffff) {
    set_error("npp_maxpool2_fwd32: tensor too large");
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(maxpool2_fwd32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_x, total, H, W,
                     Ho, Wo, d_y);
  return check_launch("npp_maxpool2_fwd32");
}

extern "C" int npp_maxpool2_bwd32(const float* d_dy, const float* d_x, const float* d_add, int N_total, int n_run, int H, int W, int C,
                                  int gate, float* d_dz, void* stream) {
  if (!d_x || !d_dz || H < 1 || W < 1 || C < 1 || n_run < 0 || n_run > N_total || (!d_dy && H / 2 > 0 && W / 2 > 0)) {
    set_error("npp_maxpool2_bwd32: bad argument (N_total=%d n_run=%d H=%d W=%d C=%d)", N_total, n_run, H, W, C);
    return NPP_ERR_ARG;
  }
  const int64_t total = (int64_t)n_run * C * H * W;
  if (total == 0) return NPP_OK;
  if ((total + 255) / 256 > 0x7fffffff) {
    set_error("npp_maxpool2_bwd32: tensor too large");
    return NPP_ERR_ARG;
  }
  hipLaunchKernelGGL(maxpool2_bwd32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_dy, d_x, d_add,
                     total, H, W, H / 2, W / 2, gate, d_dz);
  return check_launch("npp_maxpool2_bwd32");
}
