/*
 * npp_hip.h -- C ABI of libnpp_hip.so: the MI355X (gfx950) implementation of the
 * per-image NPP-Net optimisation path.
 *
 * The reference (ArmastusChen/Learning-Continuous-Implicit-Representation-for-Near-
 * Periodic-Patterns) has no FFI or operator registry for this path: it is plain
 * Python calling PyTorch.  Each entry point below therefore replaces a Python call
 * site of the reference (cited as file:line relative to the reference root) and is
 * what a ctypes binding on the reference side would bind.
 *
 * Conventions
 *   - every function returns 0 (NPP_OK) or a negative npp_status; nothing throws;
 *     npp_last_error_string() describes the last failure on the calling thread;
 *   - every pointer named d_* is a DEVICE pointer owned by the caller; the library
 *     allocates no caller-visible memory and keeps no state between calls;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it and
 *     re-entrant across streams; nothing here synchronises the device;
 *   - coordinates are (row=y, col=x) int32 pairs;
 *   - parameters live in ONE fp32 blob in the reference's own tensor layout
 *     (torch nn.Linear: weight [out][in] row-major, then bias), tensors in the order
 *     npp_param_layout() reports, so it maps 1:1 onto the reference's state_dict.
 */
#ifndef NPP_HIP_H
#define NPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPP_MAX_K 5         /* proposals (options/arg_config.py:73 p_topk, BASELINE c5) */
#define NPP_N_OFF 5         /* options/arg_config.py:20 freq_offsets */
#define NPP_N_FREQ 10       /* options/arg_config.py:27 multires */
#define NPP_E 462           /* embedding width per proposal: 22 * (1 + 2*10) */
#ifndef NPP_WIDTH           /* MLP width this build of the fused chain is specialised for: 256 (BASELINE c2; libnpp_hip.so) */
#define NPP_WIDTH 256       /* or 512 (the reference's default --netwidth, options/arg_config.py:57; libnpp_hip_w512.so)  */
#endif
#define NPP_MAX_TENSORS 32
#define NPP_MAX_STACK 16      /* images per stacked launch (npp_*_stack) */
#ifndef NPP_ROW_TILE
#define NPP_ROW_TILE 64     /* rows per workgroup of the fused MLP kernels */
#endif

typedef enum {
  NPP_OK = 0,
  NPP_ERR_ARG = -1,         /* bad argument (null pointer, size, unsupported K/width) */
  NPP_ERR_LAUNCH = -2,      /* hipLaunchKernel / runtime error, see error string */
  NPP_ERR_UNSUPPORTED = -3,
  NPP_ERR_SELFTEST = -4
} npp_status;

/* models/embedder.py:60-90 get_embedder(...) arguments + :26 the Fourier freqs
 * (random in the reference; an explicit input here). */
typedef struct {
  int32_t K;                          /* number of periodicity proposals */
  int32_t H, W;                       /* res = (H, W), embedder.py:112-113 */
  float angles_deg[NPP_MAX_K][2];     /* selected_angles[k] (degrees) */
  float periods[NPP_MAX_K][2];        /* selected_periods[k] */
  float offsets[NPP_N_OFF];           /* freq_offsets, default 0,-1,1,.5,-.5 */
  float freqs[NPP_N_FREQ];            /* Embedder freq_bands (embedder.py:26) */
} npp_embed_cfg;

/* ---- meta ---------------------------------------------------------------- */
int npp_version(void);
const char* npp_last_error_string(void);
int npp_device_count(void);
/* Launch-time choice between kernel FORMS that compute the same result (the reference has no counterpart: torch / cuDNN pick
 * their algorithms internally).  Keys: "conv_wink" (group-split window convolution: 0 never, 1 where measured best, 2 wherever
 * feasible), "conv_win" (window-staged convolution, same values), "conv_wstat" (weight-stationary block numbering, 0 / 1),
 * "conv_pair" (fused convolution pairs: bit 0 the first VGG block, bit 1 the second, bit 2 the first block's data gradient, bit 3 the loop's patch plumbing + pixel loss inside the first pair; 0 never, default 15),
 * "light_det" (1 default / 0: the proposal-ranking fits' fp32 weight-gradient launch without / with split-K float atomics),
 * "stash8" (round 6; 1 default / 0): the FORMAT of the training stash between npp_mlp_fwd*, npp_mlp_bwd* and npp_mlp_wgrad* -- 1: 8-bit
 * (csrc/npp_layout.h "W8-format": per snake layer its output as fp8 e4m3 and snake'(z) as an unsigned byte, f1 / f2 / embedding slots
 * as fp8, the pre-activation gradients as bf8 e5m2 scaled per 64-row tile by a power of two derived from max |dL/draw| of the tile;
 * the weight gradients are contracted by v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulate); 0: the 16-bit stash of rounds 2-5 (fp16
 * z, bf16 gradients, bf16 MFMA).  Unlike the other keys this one changes operand ROUNDING (not the algorithm): forward values are
 * identical, weight gradients differ by the quantisation noise of bf8 x fp8 products (tests/test_gpu_parity.py states both
 * tolerances; every reference trajectory golden holds within 0.1 dB with either).  The three launches of an iteration must see the
 * same value: flip it between complete iterations only.  value < 0 only reads.  Returns the previous value, NPP_ERR_ARG for an unknown
 * key.  Initial values come from the environment (NPP_CONV_WINK=...), defaults are the measured-best forms. */
int npp_tune(const char* key, int value);

/* ---- parameters ---------------------------------------------------------- */
/* Tensor table of the fp32 parameter blob for NPP_Net (K>1, models/networks.py:40-49)
 * or NPP_Net_top1 (K==1, :128-140).  names[i] points at static strings with the
 * reference's state_dict names; offsets/rows/cols are in floats.  Returns the number
 * of tensors (>0) or a negative status.  *total = floats in the blob. */
int npp_param_layout(int K, int width, const char** names, int64_t* offsets,
                     int32_t* rows, int32_t* cols, int64_t* total);

/* Bytes of the bf16 MFMA-fragment-ordered weight packs the fused kernels read.
 * which = 0: forward pack, 1: backward (dgrad, transposed) pack. */
int64_t npp_pack_bytes(int K, int width, int which);

/* Re-pack the fp32 blob into both bf16 packs (run after every optimiser step). */
int npp_pack_weights(const float* d_params, void* d_wf, void* d_wb, int K, int width,
                     void* stream);
/* Same mapping evaluated on the HOST (no GPU needed): used by the CPU tests to check
 * the fragment maps against a NumPy model of the MFMA.  Buffers are host memory. */
int npp_pack_weights_host(const float* params, void* wf, void* wb, int K, int width);

/* ---- exact-fp32 fused forward (BASELINE config c4: "fp32"): the same function as npp_mlp_fwd on v_mfma_f32_32x32x2_f32
 * (f32 operands and accumulation, 157 TFLOP/s peak; no bf16 rounding anywhere) -- the reference's own arithmetic type
 * (models/networks.py:56-95 via F.linear, models/embedder.py:11-56,102-148).  The render of train.py:270-331; the exact-fp32 TRAINING
 * chain built on it follows below (npp_mlp_fwd32_train).
 * npp_pack32_bytes / npp_pack_weights32: the fp32 A-operand pack of the blob ([layer][group of 4 k-steps][tile][lane][4]).
 * out_act: 0 raw / 1 sigmoid / 2 tanh (models/helpers.py:55-58). */
int64_t npp_pack32_bytes(int K, int width);
int npp_pack_weights32(const float* d_params, void* d_w32, int K, int width, void* stream);
int npp_mlp_fwd32(const int32_t* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_w32,
                  const float* d_params, float* d_out, int out_act, void* stream);

/* ---- exact-fp32 training of the fused MLP (opt-in: NPPNet(precision="fp32"), python -m npp_amd.train --precision fp32) ----------
 * The fit's three MLP launches in the reference's own arithmetic (PyTorch fp32: NPP_completion/train.py:183-254 -- render(),
 * loss.backward(), optimizer.step()), so that a fit can be compared with the reference without the bf16 / 8-bit operand roundings
 * of the default chain.  Arrays (csrc/npp_layout.h "exact-fp32 TRAINING chain"): feature-major fp32 [row][Bp], nothing rounded.
 *
 * npp_train_workspace32: byte sizes for a padded batch of Bp rows -- sizes[0] 0, sizes[1] the fp32 stash (pre-activations of the
 *   snake layers, f1, z_s, f2, z_p and the 22 K warped coordinates: (11.5 W + 22 K) * 4 bytes per row; the 462 K embedding columns
 *   are formed again from the warped coordinates by the weight-gradient launch), sizes[2] the fp32 pre-activation gradients
 *   ((11.5 W + 4) * 4 bytes per row), sizes[3] the gradient slabs: the layout and stride of npp_train_workspace, so npp_adam_step_net
 *   and npp_grad_reduce take them unchanged. */
int npp_train_workspace32(int K, int width, int64_t Bp, int ksplit, int64_t sizes[4]);
/* The transposed fp32 pack the data-gradient chain streams (models/networks.py:56-95 backwards: W^T of pos_linears, feature_linear2,
 * the f1 columns of scale_linears, feature_linear1, layers 7..1 -- the h columns of the skip layer 5): bytes, and the pack launch. */
int64_t npp_pack32_bwd_bytes(int K, int width);
int npp_pack_weights32_bwd(const float* d_params, void* d_w32_bwd, int K, int width, void* stream);
/* render() of the training iteration (NPP_completion/train.py:183-189; models/helpers.py:41-62): npp_mlp_fwd32 on the same rows, bit
 * for bit, plus the stash the two launches below read. */
int npp_mlp_fwd32_train(const int32_t* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_w32,
                        const float* d_params, float* d_pred, void* d_stash, int out_act, void* stream);
/* loss.backward() through models/networks.py:56-95 / :145-173 (NPP_completion/train.py:252): d_dpred (Bp, 3) = dL/dpred (rows beyond
 * the real batch must be 0) -> the pre-activation gradients d_dz of every layer: sigmoid / tanh output (out_act as in npp_mlp_fwd32),
 * pos_linears, the K > 1 scale branch, feature_linear1/2, the eight snake layers and the skip at layer 4.  No gradient into the
 * embedding.  Deterministic: no atomics. */
int npp_mlp_bwd32(const float* d_dpred, const float* d_pred, int64_t Bp, int K, int width, const void* d_w32_bwd,
                  const float* d_params, const void* d_stash, void* d_dz, int out_act, void* stream);
/* The weight and bias gradients of that backward (what autograd accumulates into .grad of every nn.Linear, networks.py:40-49) as
 * ksplit slabs in the parameter-blob layout, contracted over the rows on the fp32 MFMA.  Row tile t of the T = Bp / 64 belongs to
 * slab s with s T / ksplit <= t < (s + 1) T / ksplit; every slab is written in full (a slab without rows holds zeros), by one
 * workgroup per output tile in row order: no float atomics, identical bits on every run.  cfg: the embedder of the forward (its
 * Fourier frequencies are needed to form the embedding columns again). */
int npp_mlp_wgrad32(const void* d_dz, const void* d_stash, const npp_embed_cfg* cfg, int64_t Bp, int K, int width, int ksplit,
                    float* d_gslabs, void* stream);

/* ---- a1+a2+a4: embedder -------------------------------------------------- */
/* Replaces Embedder_periodic.embed + Embedder.embed + cat (models/embedder.py:140-148,
 * :51-56; NPP_completion/train.py:93-105): coords (N,2) -> (N, K*462), row-major,
 * reference column order.  out_dtype 0 = fp32, 1 = bf16.  precise != 0 uses full-
 * range sinf/cosf (fp32 parity path), 0 uses the hardware v_sin/v_cos. */
int npp_embed_fwd(const int32_t* d_coords_yx, int64_t N, const npp_embed_cfg* cfg,
                  void* d_out, int out_dtype, int precise, void* stream);
/* The 22-vector stage alone (embedder.py:140-148): (N,2) -> (N, K*22) fp32. */
int npp_warp_fwd(const int32_t* d_coords_yx, int64_t N, const npp_embed_cfg* cfg,
                 float* d_out, void* stream);

/* ---- continuous coordinates: render a fitted network anywhere on the plane ----------------------------------------------
 * The network is a function of the fit's pixel frame (row y, col x as floats; res = (cfg->H, cfg->W) only scales the two linear
 * columns).  The _coordf forms take (N, 2) fp32 positions [y, x] instead of int32 pixel indices, with the same padding contract as
 * their int32 neighbours.  The _grid forms take no coordinate buffer: canvas pixel (i, j) of a canvas `width` pixels wide sits at
 *     y = y0 + i / sy,  x = x0 + j / sx
 * (an IEEE fp32 quotient, then a separate fp32 add; i and j converted to fp32 exactly), and a launch covers canvas pixels
 * [start, start + n) in row-major order, writing exactly n output rows (no padding: the surplus rows of the last 64-row tile
 * compute on the last pixel and are not stored).  So integer scales nest: at scale S, pixel (S i, S j) is bit for bit pixel (i, j)
 * of scale 1, and scale 1 at origin 0 is the int32 render of the full grid.  NPP_ERR_ARG (with a message) when sy or sx is not
 * finite or not > 0, the origin is not finite, width < 1, start < 0, n < 0, or a canvas row or column index would reach 2^24
 * (fp32 would no longer hold it exactly); n == 0 is a no-op. */
typedef struct {
  int64_t start, n;      /* first canvas pixel (row-major) and number of pixels of this launch */
  int32_t width;         /* canvas width in pixels */
  float y0, x0;          /* fit-frame position of canvas pixel (0, 0) */
  float sy, sx;          /* canvas pixels per fit pixel (2 = twice the density) */
} npp_grid;
/* npp_mlp_fwd_act (bf16 chain, inference: no stash) over a canvas grid: d_out (n, 3).  out_act: 0 raw / 1 sigmoid / 2 tanh. */
int npp_mlp_fwd_grid(const npp_grid* grid, const npp_embed_cfg* cfg, int width, const void* d_wf, const float* d_params,
                     float* d_out, int out_act, void* stream);
/* npp_mlp_fwd32 (exact fp32 chain) over a canvas grid: d_out (n, 3). */
int npp_mlp_fwd32_grid(const npp_grid* grid, const npp_embed_cfg* cfg, int width, const void* d_w32, const float* d_params,
                       float* d_out, int out_act, void* stream);
/* The _view forms are the _grid forms under a projective map: canvas pixel (i, j) sits at
 *     d = (m6 i + m7 j) + m8,  y = ((m0 i + m1 j) + m2) / d,  x = ((m3 i + m4 j) + m5) / d
 * in fp32, every product and sum rounded separately (no fma contraction) and an IEEE quotient; i and j converted exactly.  The same
 * launch contract: pixels [start, start + n) in row-major order, exactly n rows stored, n == 0 a no-op, indices below 2^24.  A pixel
 * is IN VIEW iff d > 0 and y and x are finite; a pixel not in view stores (0, 0, 0) and computes on the position (0, 0), so no
 * non-finite position enters the chain.  d_inside (n bytes, may be null): 0 not in view, 1 in view, 3 in view and inside the fit's
 * image rectangle, -0.5 <= y < cfg->H - 0.5 and -0.5 <= x < cfg->W - 0.5.  NPP_ERR_ARG (with a message) for a non-finite matrix
 * entry, width < 1, negative start or n, or an index that reaches 2^24.  The affine map [[1/sy, 0, y0], [0, 1/sx, x0], [0, 0, 1]]
 * with power-of-two scales is the grid launch at (y0, x0, sy, sx) bit for bit. */
typedef struct {
  int64_t start, n;      /* first canvas pixel (row-major) and number of pixels of this launch */
  int32_t width;         /* canvas width in pixels */
  float m[9];            /* row-major 3x3 map: canvas (row, col, 1) -> fit-frame (y, x) over d */
} npp_view;
/* npp_mlp_fwd_grid under a view: d_out (n, 3), d_inside (n) or null. */
int npp_mlp_fwd_view(const npp_view* view, const npp_embed_cfg* cfg, int width, const void* d_wf, const float* d_params,
                     float* d_out, uint8_t* d_inside, int out_act, void* stream);
/* npp_mlp_fwd32_grid under a view: d_out (n, 3), d_inside (n) or null. */
int npp_mlp_fwd32_view(const npp_view* view, const npp_embed_cfg* cfg, int width, const void* d_w32, const float* d_params,
                       float* d_out, uint8_t* d_inside, int out_act, void* stream);
/* The positions and inside bytes of such a launch by plain C++ on the host (the same rule, compiled without contraction): out_yx
 * (n, 2) [y, x] ((0, 0) for a pixel not in view), inside (n) or null; H, W: the fit's image size (cfg->H, cfg->W). */
int npp_view_coords_host(const npp_view* view, int H, int W, float* out_yx, uint8_t* inside);
/* ---- supersampled launches: ss x ss samples per canvas pixel, averaged in the kernel ----------------------------------------
 * The _grid_ss / _view_ss forms are the _grid / _view forms with ss in {1, 2, 4, 8} samples per canvas pixel in each direction and
 * their mean as the pixel's colour.  ss^2 divides the 64-row tile of both chains, so a tile holds 64 / ss^2 whole pixels and the
 * mean never crosses a workgroup: one launch, no atomics, no intermediate buffer.  The rule:
 *   offsets       off[a] = (2 a + 1) / (2 ss) - 0.5 for a = 0 .. ss - 1 (exact in fp32).
 *   sample order  sample s = a ss + b of canvas pixel (i, j) sits at the canvas position fi = (float)i + off[a], fj = (float)j +
 *                 off[b], one fp32 add each; with ss > 1 a canvas row or column index must stay below 2^20 so that this add is exact.
 *   grid form     y = y0 + fi / sy, x = x0 + fj / sx (IEEE quotient, then a separate add).
 *   view form     d, y, x from (fi, fj) in the operation order of the _view forms (no contraction).  A sample is in view iff d > 0
 *                 and y and x are finite; a sample not in view computes on (0, 0) and does not count.
 *   chain rows    row r of a launch is sample r % ss^2 of pixel start + min(r / ss^2, n - 1); a launch runs n ss^2 rows and stores
 *                 exactly n output rows.
 *   pixel colour  after the output nonlinearity: acc = +0.0f; for s = 0 .. ss^2 - 1 in that order acc = acc + o_s if the sample
 *                 counts (one rounded fp32 add each); colour = acc / (float)count (IEEE quotient).  In a grid launch every sample
 *                 counts and count = ss^2.
 *   inside byte   of a view launch: the byte the point launch writes for the pixel centre (i, j), unchanged, so masks do not depend
 *                 on ss.  Where that byte is 0, or where no sample counts, the pixel stores (0, 0, 0) and byte 0.
 *   ss = 1        is the _grid / _view launch bit for bit (these entry points forward to it).
 * NPP_ERR_ARG (with a message) for ss outside {1, 2, 4, 8}, for an index that reaches 2^20 with ss > 1, for n ss^2 rows beyond the
 * 2^31 - 1 tiles of a launch, and for everything the _grid / _view forms refuse; n == 0 stays a no-op. */
int npp_mlp_fwd_grid_ss(const npp_grid* grid, int ss, const npp_embed_cfg* cfg, int width, const void* d_wf, const float* d_params,
                        float* d_out, int out_act, void* stream);
int npp_mlp_fwd32_grid_ss(const npp_grid* grid, int ss, const npp_embed_cfg* cfg, int width, const void* d_w32, const float* d_params,
                          float* d_out, int out_act, void* stream);
int npp_mlp_fwd_view_ss(const npp_view* view, int ss, const npp_embed_cfg* cfg, int width, const void* d_wf, const float* d_params,
                        float* d_out, uint8_t* d_inside, int out_act, void* stream);
int npp_mlp_fwd32_view_ss(const npp_view* view, int ss, const npp_embed_cfg* cfg, int width, const void* d_w32, const float* d_params,
                          float* d_out, uint8_t* d_inside, int out_act, void* stream);
/* The same rule by plain C++ on the host: the (n ss^2, 2) fp32 positions [y, x] of such a launch in chain-row order ((0, 0) for a
 * sample not in view), sample_in_view (n ss^2 bytes, 0 / 1, may be null) and the per-pixel inside bytes (n, may be null). */
int npp_grid_samples_host(const npp_grid* grid, int ss, float* out_yx);
int npp_view_samples_host(const npp_view* view, int ss, int H, int W, float* out_yx, uint8_t* sample_in_view, uint8_t* inside);
/* ---- adaptive supersampling: a class per canvas pixel of a view, and launches over listed pixels --------------------------------
 * A view under perspective is coarse at its far end and fine near the camera, so one ss for the whole canvas pays the far end's
 * price everywhere.  The class launch gives every canvas pixel the ss its own footprint asks for; the listed launch is the _view_ss
 * launch over the pixels of one class.  Every pixel of the result is, bit for bit, what the uniform launch at that pixel's ss writes.
 * The class rule, for canvas pixel (i, j) of an npp_view with a .. k = m[0 .. 8] converted fp32 -> float64:
 *   class 0       iff the point launch's inside byte of the pixel centre is 0 (the fp32 rule of the _view forms, unchanged).
 *   otherwise     in float64, every operation rounded separately (no contraction), no square root and no quotient:
 *                   d    = |(g i + h j) + k|
 *                   t    = (d d) d
 *                   adet = |(a (e k - f h) - b (d1 k - f g)) + c (d1 h - e g)|,  d1 = m[3]: once per launch, on the host
 *                 the class is the smallest S in {1, 2, 4, 8} with adet <= (2.25 S^2) t, else 8; the constants 2.25, 9, 36, 144 are
 *                 exact and (2.25 S^2) t is one rounded product.
 * This is the uniform rule (S = the next of 1, 2, 4, 8 at or above density / 1.5) on density = sqrt|det J| at the pixel centre, with
 * |det J| = |det M| / |d|^3, rearranged so that NumPy, the host twin and the kernel agree byte for byte.
 * npp_view_ss_classes: one thread per pixel of [start, start + n): d_cls (n bytes: 0, 1, 2, 4 or 8) and, unless null, d_inside (n
 * bytes: the centre's inside byte for a fit of H x W).  _host: the same function in plain C++ on host memory.  NPP_ERR_ARG (with a
 * message) for everything the _view forms refuse in a view, H or W < 1, a null d_cls with n > 0; n == 0 is a no-op. */
int npp_view_ss_classes(const npp_view* view, int H, int W, uint8_t* d_cls, uint8_t* d_inside, void* stream);
int npp_view_ss_classes_host(const npp_view* view, int H, int W, uint8_t* cls, uint8_t* inside);
/* Listed launches: the _view_ss launch over a listed subset of the canvas window.  view->start, n, width name the window that d_out
 * (n, 3) and d_inside (n, may be null) cover; d_pix holds n_list absolute row-major canvas pixel indices.
 *   chain rows    row r of a launch is sample r % ss^2 of pixel d_pix[min(r / ss^2, n_list - 1)]: n_list ss^2 rows.
 *   per pixel     positions, counting, ordered mean and inside byte are those of _view_ss for that pixel p, stored at
 *                 d_out[(p - start) 3 + c] and d_inside[p - start].
 *   ss = 1        a listed pixel gets the point launch's bits, colour and byte (the one sample is stored as it is: +0 + o would
 *                 turn -0.0 into +0.0).
 *   nothing else  no other word changes: unlisted pixels are not touched, and an index outside [start, start + n) is skipped by the
 *                 kernel and stores nothing.  An index listed twice is written twice with the same bits.
 * n_list == 0 (or n == 0) is a no-op.  NPP_ERR_ARG (with a message) for everything _view_ss refuses, for n_list < 0, for a null list
 * with n_list > 0 and for n_list ss^2 rows beyond the 2^31 - 1 tiles of a launch. */
int npp_mlp_fwd_view_list(const npp_view* view, int ss, const int64_t* d_pix, int64_t n_list, const npp_embed_cfg* cfg, int width,
                          const void* d_wf, const float* d_params, float* d_out, uint8_t* d_inside, int out_act, void* stream);
int npp_mlp_fwd32_view_list(const npp_view* view, int ss, const int64_t* d_pix, int64_t n_list, const npp_embed_cfg* cfg, int width,
                            const void* d_w32, const float* d_params, float* d_out, uint8_t* d_inside, int out_act, void* stream);
/* npp_mlp_fwd_act (inference) on fp32 positions: coords (Bp, 2) -> d_pred (Bp, 3), Bp a multiple of NPP_ROW_TILE. */
int npp_mlp_fwd_coordf(const float* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_wf,
                       const float* d_params, float* d_pred, int out_act, void* stream);
/* npp_mlp_fwd32 on fp32 positions: coords (Bp, 2) -> d_out (Bp, 3), Bp a multiple of NPP_ROW_TILE. */
int npp_mlp_fwd32_coordf(const float* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_w32,
                         const float* d_params, float* d_out, int out_act, void* stream);
/* npp_warp_fwd on fp32 positions (the reference's Embedder_periodic.embed of a float tensor): (N, 2) -> (N, K*22), any N. */
int npp_warp_fwd_coordf(const float* d_coords_yx, int64_t N, const npp_embed_cfg* cfg, float* d_out, void* stream);
/* npp_embed_fwd on fp32 positions: (N, 2) -> (N, K*462), any N; out_dtype / precise as there. */
int npp_embed_fwd_coordf(const float* d_coords_yx, int64_t N, const npp_embed_cfg* cfg, void* d_out, int out_dtype, int precise,
                         void* stream);

/* ---- a5+a6+a7: fused coordinate MLP -------------------------------------- */
/* Workspace sizes (bytes) for a padded batch of Bp rows (multiple of NPP_ROW_TILE):
 *  sizes[0] 0 (reserved)
 *  sizes[1] actF   forward stash: the 16-bit W-format region (csrc/npp_layout.h: fp16 pre-activations of the snake layers, bf16
 *                  f1 / f2, bf16 embedding slots) followed by the 8-bit W8-format region of the same k-step table; with
 *                  npp_tune("stash8") = 1 the first region holds the snake'(z) bytes (at W8 size) and the second the fp8 arrays,
 *                  with 0 only the first is used -- one allocation serves both settings
 *  sizes[2] dzF    pre-activation gradients: bf16 fragments in W-format, or (stash8) bf8 units in W8-format + one int32 scale
 *                  word per 64-row tile behind them (fits the same allocation)
 *  sizes[3] grad slabs (ksplit * S * 4 bytes, S = the parameter count rounded up to a multiple of 4 floats: the slab stride) */
int npp_train_workspace(int K, int width, int64_t Bp, int ksplit, int64_t sizes[4]);

/* Replaces render() -> run_network -> NPP_Net.forward -> sigmoid
 * (models/helpers.py:41-62, models/networks.py:56-95 / :145-173) INCLUDING the
 * embedding lookup it is fed with (train.py:166-181): coords (Bp,2) -> pred (Bp,3).
 * d_wf: forward pack; d_params: fp32 blob (biases + rgb_linear are read from it).
 * d_actF may be NULL (inference / full-image render, train.py:277-309); when given, the
 * kernel also writes the stash npp_mlp_bwd / npp_mlp_wgrad need.
 * Bp must be a multiple of NPP_ROW_TILE (pad with any valid coordinate). */
int npp_mlp_fwd(const int32_t* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg,
                int width, const void* d_wf, const float* d_params, float* d_pred,
                void* d_actF, void* stream);
/* The same with render()'s output nonlinearity as an argument (models/helpers.py:55-60): out_act 1 = sigmoid (npp_mlp_fwd), 2 = tanh
 * (--normalize_type 2: images scaled to [-1, 1], loaders/loaders.py:56,111), 0 = the raw network output. */
int npp_mlp_fwd_act(const int32_t* d_coords_yx, int64_t Bp, const npp_embed_cfg* cfg, int width, const void* d_wf,
                    const float* d_params, float* d_pred, void* d_actT, int out_act, void* stream);

/* Backward of the same (what loss.backward() does through networks.py:56-95):
 * d_dpred (Bp,3) = dL/dpred (rows >= the real batch must be 0).  Reads actF, writes dzF. */
int npp_mlp_bwd(const float* d_dpred, const float* d_pred, int64_t Bp, int K, int width,
                const void* d_wb, const float* d_params, const void* d_actF,
                void* d_dzF, void* stream);

/* The same with the patch rows' dL/dpred formed inside the launch from the patch losses' image gradients (the sum
 * npp_patch_compose_bwd computes: NPP_completion/train.py:200-236 backwards) -- rows [row0, row0 + n_p*P*P) of d_dpred are
 * WRITTEN (so the buffer ends up as loss.backward() would leave it), all other rows are read as in npp_mlp_bwd. */
typedef struct {
  const float* dx_a;      /* (n_p*k, 3, P, P) dL/dx of the contextual branch */
  const float* dx_b;      /* same shape, second branch (LPIPS / style) or NULL */
  const float* fmask;     /* (n_p, P, P) */
  const float* rmask;     /* (n_p*k, P, P) */
  int64_t row0;           /* first patch row of the batch (= N_rand) */
  int32_t n_p, k, P, comp;
} npp_patch_grad;
int npp_mlp_bwd_patch(float* d_dpred, const float* d_pred, int64_t Bp, int K, int width,
                      const void* d_wb, const float* d_params, const void* d_actF,
                      void* d_dzF, const npp_patch_grad* patch, void* stream);
/* npp_mlp_bwd_patch behind out_act (see npp_mlp_fwd_act). */
int npp_mlp_bwd_patch_act(float* d_dpred, const float* d_pred, int64_t Bp, int K, int width, const void* d_wb,
                          const float* d_params, const void* d_actT, void* d_dzT, const npp_patch_grad* pg, int out_act,
                          void* stream);

/* Compatibility forms at the reference's module boundary.  NPP_Net(...).forward(None, x_periodic)
 * (models/networks.py:56-95, NPP_Net_top1 :134-173) receives a MATERIALISED embedding:
 * d_emb (Bp, ld >= K*462) fp32 row-major in the reference's column order (any embedder may have
 * produced it).  out_act selects what render() applies to the network output (models/helpers.py:55-60):
 * 0 = none (the module's own return value), 1 = sigmoid, 2 = tanh.  The backward of that forward
 * takes the same out_act.  These read 5.5 KB per row from HBM that npp_mlp_fwd never materialises. */
int npp_mlp_fwd_emb(const float* d_emb, int64_t ld, int64_t Bp, int K, int width, const void* d_wf,
                    const float* d_params, float* d_out, void* d_actF, int out_act, void* stream);
int npp_mlp_bwd_act(const float* d_dout, const float* d_out, int64_t Bp, int K, int width,
                    const void* d_wb, const float* d_params, const void* d_actF, void* d_dzF,
                    int out_act, void* stream);

/* Weight/bias gradients: ksplit partial slabs in the parameter-blob layout
 * (slab s at d_gslabs + s * S floats, S = sizes[3] / (4 * ksplit) of npp_train_workspace: 16-byte aligned slabs);
 * npp_adam_step sums them (pass S as its slab_stride). */
int npp_mlp_wgrad(const void* d_dzF, const void* d_actF, int64_t Bp, int K, int width,
                  int ksplit, float* d_gslabs, void* stream);

/* Output tiles (256 x 256) of the grouped weight-gradient launch for K proposals: the launch has
 * tiles x ksplit workgroups of one per CU, so ksplit = CUs / tiles fills the chip in one round
 * (K = 3: 21 tiles -> 12 on 256 CUs; K = 5: 25 -> 10; K = 1: 14 -> 18). */
int npp_mlp_wgrad_tiles(int K);

/* ---- stash audit: census of the 8-bit training stash (npp_tune "stash8" = 1) -----------------------------
 * The reference trains in fp32 and has nothing to count; the 8-bit stash converts with saturation (a value out of range becomes the
 * largest finite code, silently) and flushes what lies far below a tile's maximum.  The census scans what ONE iteration's
 * npp_mlp_fwd* / npp_mlp_bwd* left in actF's W8 region and in dzF's bf8 arrays and counts, per array the configuration writes
 * (rows < n_rows and real features only: 462 of an embedding's 480 slots, the 3 used features of dz_rgb, W / 2 of a_p / dz_p):
 *   record[offsets[i] + NPP_CENSUS_ELEMENTS]   bytes counted
 *                      NPP_CENSUS_ZERO         codes 0x00 / 0x80 (a flushed value and a true zero share them: an upper bound on flushes)
 *                      NPP_CENSUS_SUBNORMAL    exponent field 0, mantissa != 0
 *                      NPP_CENSUS_AT_MAX       |code| = the largest finite (e4m3 0x7E = 448, e5m2 0x7B = 57344): saturated, or exactly there
 *                      NPP_CENSUS_NONFINITE    e4m3 0x7F (NaN); e5m2 0x7C..0x7F (infinity, NaN)
 *                      NPP_CENSUS_HIST + e     finite codes by exponent field e (32 bins; e4m3 uses 16); bin 0 = zero + subnormal
 * so that elements = zero + subnormal + sum of bins 1.. + nonfinite, with at_max inside its bin.  Behind the arrays, at *tile_offset:
 * NPP_CENSUS_TILES (64-row tiles with a real row) and NPP_CENSUS_SCALE_MIN / _MAX, the smallest / largest E8M0 byte of their scale
 * words (stored gradient * 2^(byte - 127) = gradient).  All words are int64; integer sums: the record does not depend on the schedule.
 *
 * npp_stash8_census_words: int64 words of the record.  npp_stash8_census_layout: the table -- names[i] (static strings: a0..a7 the
 * snake layers' outputs, f1, a_s, f2, a_p, emb0.., dz0..dz7, dz_f1, dz_s, dz_f2, dz_p, dz_rgb; K = 1 has no a_s / f2 / dz_s / dz_f2),
 * formats[i] (0 = fp8 e4m3, 1 = bf8 e5m2), features[i] (real features per row), offsets[i] (words into the record); any output may be
 * NULL, arrays hold NPP_CENSUS_MAX_ARRAYS entries; returns the number of arrays.
 * npp_stash8_census: d_actF / d_dzF are the workspace arrays of npp_train_workspace(K, width, Bp) as the launches were given them
 * (a stacked workspace: the same entry on image m's offset pointers); 1 <= n_rows <= Bp.  Clears d_record itself (hipMemsetAsync),
 * then one launch; allocates nothing and writes nothing else.  npp_stash8_census_host: the same counts by plain C++ on HOST copies
 * of the same bytes (no GPU needed). */
#define NPP_CENSUS_ELEMENTS 0
#define NPP_CENSUS_ZERO 1
#define NPP_CENSUS_SUBNORMAL 2
#define NPP_CENSUS_AT_MAX 3
#define NPP_CENSUS_NONFINITE 4
#define NPP_CENSUS_HIST 5
#define NPP_CENSUS_BINS 32
#define NPP_CENSUS_ENTRY_WORDS (NPP_CENSUS_HIST + NPP_CENSUS_BINS)
#define NPP_CENSUS_TILES 0
#define NPP_CENSUS_SCALE_MIN 1
#define NPP_CENSUS_SCALE_MAX 2
#define NPP_CENSUS_TILE_WORDS 3
#define NPP_CENSUS_MAX_ARRAYS (12 + NPP_MAX_K + 13)
int64_t npp_stash8_census_words(int K, int width);
int npp_stash8_census_layout(int K, int width, const char** names, int32_t* formats, int32_t* features, int64_t* offsets,
                             int64_t* tile_offset);
int npp_stash8_census(const void* d_actF, const void* d_dzF, int64_t Bp, int64_t n_rows, int K, int width, int64_t* d_record,
                      void* stream);
int npp_stash8_census_host(const void* actF, const void* dzF, int64_t Bp, int64_t n_rows, int K, int width, int64_t* record);

/* d_grad[n] (+)= sum of the slabs: the parameter gradient as one blob, for optimisers other than
 * npp_adam_step (the reference hands model.parameters() to torch.optim.Adam, helpers.py:164). */
int npp_grad_reduce(const float* d_gslabs, int n_slabs, int64_t slab_stride, int64_t n,
                    float* d_grad, int accumulate, void* stream);

/* ---- a2 stand-alone: Embedder.embed (models/embedder.py:11-56) on any (N,d) fp32 input:
 * out (N, d*(2*n_freq + include_input)) = [x | sin(f0 x) | cos(f0 x) | ...]; freqs is a HOST array. */
int npp_fourier_fwd(const float* d_x, int64_t N, int d, const float* freqs, int n_freq,
                    int include_input, float* d_out, void* stream);

/* ---- a8: adaptive robust pixel loss -------------------------------------- */
/* Replaces img2mse(pred, gt, 'robust_loss_adaptive', adaptive_pix, mask)
 * (models/mse_calculator.py:13-27 -> robust_loss_pytorch/adaptive.py:183-204) and its
 * backward.  pred/gt (N,3), mask (N,1) or NULL.  latents: [alpha(3) | scale(3)].
 * spline: values[n_knots] then tangents[n_knots] fp32 (distribution.py:129-141).
 * Outputs: d_loss[0] += mean nll (caller zeroes), d_dpred (N,3) = weight * dL/dpred,
 * d_dlatent[6] += weight * dL/dlatents (caller zeroes). */
int npp_pixel_loss(const float* d_pred, const float* d_gt, const float* d_mask, int64_t N,
                   const float* d_latents, const float* d_spline, int n_knots,
                   float x_scale, float weight, float* d_loss, float* d_dpred,
                   float* d_dlatent, void* stream);

/* ---- a14: Adam ------------------------------------------------------------ */
/* torch.optim.Adam step (models/helpers.py:164; NPP_completion/train.py:253-254) over
 * n floats: g = sum of n_slabs slabs (slab stride = slab_stride floats).  `step` is
 * the 1-based step count used for bias correction. */
int npp_adam_step(float* d_p, float* d_m, float* d_v, const float* d_gslabs, int64_t n,
                  int n_slabs, int64_t slab_stride, float lr, float beta1, float beta2,
                  float eps, int step, void* stream);

/* One launch for optimizer.step() over the network blob AND the adaptive-loss latents
 * (create_npp_net puts both groups into one torch.optim.Adam, models/helpers.py:144-164), which
 * also performs the next optimizer.zero_grad() (train.py:192) of the small accumulators: the
 * latent gradient d_dlat[n_lat] is cleared after use and d_zero[n_zero] is cleared. */
int npp_adam_step_net(float* d_p, float* d_m, float* d_v, const float* d_gslabs, int64_t n,
                      int n_slabs, int64_t slab_stride, float* d_lat, float* d_lat_m,
                      float* d_lat_v, float* d_dlat, int n_lat, float* d_zero, int n_zero,
                      float lr, float beta1, float beta2, float eps, int step, void* stream);

/* npp_adam_step_net + npp_pack_weights in ONE launch: every updated weight is also written, as bf16, into the forward and
 * backward MFMA packs (which npp_pack_weights must have filled once: their padding elements are not rewritten).  Replaces
 * optimizer.step() (models/helpers.py:164; NPP_completion/train.py:253) followed by the re-pack the fused kernels need.
 * npp_pack_scatter_host: host twin of the scatter (inverse pack maps), for tests. */
int npp_adam_step_net_pack(float* d_p, float* d_m, float* d_v, const float* d_gslabs, int64_t n,
                           int n_slabs, int64_t slab_stride, float* d_lat, float* d_lat_m,
                           float* d_lat_v, float* d_dlat, int n_lat, float* d_zero, int n_zero,
                           float lr, float beta1, float beta2, float eps, int step, int K, int width,
                           void* d_wf, void* d_wb, float* d_pl_partials, float* d_loss_cur, void* stream);
/* (d_pl_partials, nullable: the scratch of the iteration's pixel-loss launch, npp_pixel_loss_args.scratch -- its per-block sums
 *  are added, in block order, to the latent gradients before the latents' step and to d_loss_cur[0], the iteration's pixel-loss
 *  accumulator.) */
int npp_pack_scatter_host(const float* params, void* wf, void* wb, int K, int width);

/* Host only, launches nothing: the two step-dependent scalars of every Adam entry of this library for 1-based step `step`,
 * out[0] = step_size = lr / (1 - beta1^step), out[1] = 1 / sqrt(1 - beta2^step) -- the float arguments widened to double,
 * pow / sqrt in double, each result rounded to float once.  These are the words the *_dev forms read from d_hp.
 * NPP_ERR_ARG for step < 1 or a null out. */
int npp_adam_words(float lr, float beta1, float beta2, int step, float out[2]);

/* Same step with step_size = lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) read from device memory
 * (d_hp[0], d_hp[1]): lets a captured HIP graph of one optimisation iteration be replayed. */
int npp_adam_step_dev(float* d_p, float* d_m, float* d_v, const float* d_gslabs, int64_t n,
                      int n_slabs, int64_t slab_stride, float beta1, float beta2, float eps,
                      const float* d_hp, void* stream);

/* npp_adam_step_net_pack with step_size = lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) read from device memory (d_hp[0], d_hp[1]):
 * optimizer.step() of NPP_completion/train.py:253 with the LR rule of :257-263 applied by whoever writes the two words (the
 * host, in the double arithmetic of npp_adam_step_net_pack) -- the form a captured HIP graph of one optimisation iteration
 * replays (fit.CompletionFit(graph_iteration=True)).  Same kernel, same bits as the argument form for equal words. */
int npp_adam_step_net_pack_dev(float* d_p, float* d_m, float* d_v, const float* d_gslabs, int64_t n,
                               int n_slabs, int64_t slab_stride, float* d_lat, float* d_lat_m,
                               float* d_lat_v, float* d_dlat, int n_lat, float* d_zero, int n_zero,
                               float beta1, float beta2, float eps, const float* d_hp, int K, int width,
                               void* d_wf, void* d_wb, float* d_pl_partials, float* d_loss_cur, void* stream);

/* ---- a9/a10: patch crops ---------------------------------------------------- */
/* Replaces extract_glimpse(..., mode='nearest', padding_mode='zeros', normalized=False,
 * centered=False) as models/sampler.py:171-178,284-291 calls it (utils/extract_glimpse.py:
 * 53-79): integer crops [c - P/2, c + P/2) of the (H,W,3) image and (H,W) mask at M centres
 * (row, col), zeros outside.  out_rgb (M,3,P,P), out_mask (M,1,P,P) or NULL. */
int npp_patch_gather(const float* d_img_hwc, const float* d_mask_hw, int H, int W,
                     const int32_t* d_centres_yx, int M, int P, float* d_out_rgb,
                     float* d_out_mask, void* stream);

/* The input rows of one loop iteration (NPP_completion/train.py:166-181) assembled in one launch: rows [0, n_pix) =
 * i_train[pix[t]] (the np.random.choice of :172-174), rows [n_pix, n_pix + n_p P^2) = the pixel coordinates of the fake
 * patches around centres `cen` (models/sampler.py:269-279), zero rows up to Bp; gt = img[row] and (optional, remapping)
 * pmask = pmask_img[row] of the pixel rows.  coords int32 (Bp, 2) (row, col); gt (n_pix, 3). */
int npp_batch_assemble(const int32_t* d_i_train, int64_t n_train, const int64_t* d_pix, int64_t n_pix,
                       const int32_t* d_cen, int n_p, int P, int64_t Bp, const float* d_img_hwc,
                       const float* d_pmask_hw, int H, int W, int32_t* d_coords, float* d_gt, float* d_pmask,
                       void* stream);

/* ---- a10: patch plumbing (NPP_completion/train.py:200-236) and its backward ------ */
/* d_pred_rows (n_p*P*P, 3): the predicted patch rows (row = (p*P + y)*P + x, train.py:178-181);
 * d_fake (n_p,3,P,P) / d_fmask (n_p,1,P,P): fake patch and its known mask (untiled; the reference
 * tiles them k times); d_real (n_p*k,3,P,P) / d_rmask (n_p*k,1,P,P).  comp != 0: 'val' compositing
 * (train.py:230-231).  d_xy (2*n_p*k, 3, P, P) = [x | y]: x = (comp ? fake*fmask + pred*(1-fmask)
 * : pred) * rmask, y = real * rmask -- the inputs of contextualLoss (and of percepLoss in 'same'
 * mode).  The backward sums dL/dx (two sources: d_dx_b nullable) over the k copies into
 * d_dpred_rows (n_p*P*P, 3) (overwritten). */
int npp_patch_compose_fwd(const float* d_pred_rows, const float* d_fake, const float* d_fmask,
                          const float* d_real, const float* d_rmask, int n_p, int k, int P,
                          int comp, float* d_xy, void* stream);
int npp_patch_compose_bwd(const float* d_dx_a, const float* d_dx_b, const float* d_fmask,
                          const float* d_rmask, int n_p, int k, int P, int comp,
                          float* d_dpred_rows, void* stream);

/* ---- a12: contextual loss core ------------------------------------------------ */
/* Replaces contextual_loss(x, y, band_width, weight, 'cosine') and its backward w.r.t. x
 * (externel_lib/contextual_loss/functional.py:9-63,127-163) on feature tensors (N,C,h*w) fp32
 * NCHW (C a multiple of 32).  d_loss[0] += scale * loss ; d_dfx (N,C,hw) = scale * dL/dx or
 * NULL for forward only.  d_weight: per-sample weights (functional.py:55-57) or NULL.  Any hw: the loop's
 * patches give hw <= 1600; the whole-image crops of the proposal ranking (NPP_proposal/search.py:180-197)
 * go through a column-chunked row pass (workspace = 2 N hw^2 floats + O(N hw)). */
int64_t npp_cx_workspace_bytes(int N, int C, int hw);
int npp_cx_fwd_bwd(const float* d_fx, const float* d_fy, int N, int C, int hw, float band_width,
                   const float* d_weight, float scale, float* d_loss, float* d_dfx,
                   void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- a13: LPIPS head (adaptive-robust variant), one VGG16 tap per call --------- */
/* Replaces, for tap kk, lpips.py:99-121 + :130 (normalize_tensor, per-channel robust NLL of
 * the difference, lin 1x1 conv, spatial mean) and its backward.  feats (N,C,hw) fp32 NCHW;
 * d_latents [alpha(C) | scale(C)]; d_loss[0] += scale * mean_n(...); d_df0 (N,C,hw) and
 * d_dlatent [2C] (accumulated) may both be NULL for forward only.  C in {16, 32, 64, 128, 192,
 * 256, 384, 512}.  d_workspace: npp_lpips_workspace_bytes(C) bytes, ZEROED once by the caller and owned by one
 * stream -- the latent gradients and the loss are then summed over the launch's blocks as fixed-point integers
 * (order-independent, bit-reproducible); NULL: float atomics in arrival order.  A grouped launch (npp_lpips_layers) with
 * workspaces adds the taps' totals to d_loss[0] in tap order, as ONE addend, from slots behind tap 0's accumulators.
 * d_latents == NULL: the PLAIN head, LPIPS.forward(use_robust=False) (lpips.py:108-109: diffs = (feats0 - feats1)^2) -- the in-loop
 * form under --use_adaptive_perceptual_loss off (train.py:241-251) -- with its gradient d_df0 (d_spline, d_dlatent NULL). */
int64_t npp_lpips_workspace_bytes(int C);
/* All taps of LPIPS.forward in ONE launch (lpips.py:99-133: the heads are independent, `val` is their sum): taps[i] = the per-tap
 * arguments of npp_lpips_layer (host array, n_taps <= 5); a tap's workspace must not be shared with another tap of the call. */
typedef struct {
  const float* f0; const float* f1; int32_t C, hw; const float* lin; const float* latents;
  float* df0; float* dlatent; void* workspace;
  /* optional: the gradient w.r.t. feats0 as bf16 in the trunk's flat layout (a zero-initialised npp_trunk_act buffer of geometry
   * (N_total, C, H, W), H * W == hw) INSTEAD of df0 (then NULL): what npp_trunk_grad_in(df0, NULL, ...) would produce in a launch of
   * its own -- the tap gradient npp_maxpool2_bwd / npp_conv3x3_dgrad_pool add in. */
  void* dflat; int32_t N_total, H, W;
  const void* yact;   /* optional with dflat: the tapped layer's own flat fp16 activation; the gradient is gated by [yact > 0]
                       * (= npp_trunk_grad_in(df0, yact, ...): dL/d(pre-activation) of the top tap's layer) */
} npp_lpips_tap;
int npp_lpips_layers(int n_taps, const npp_lpips_tap* taps, int N, const float* d_spline, int n_knots, float x_scale, float scale,
                     float* d_loss, void* stream);
int npp_lpips_layer(const float* d_f0, const float* d_f1, int N, int C, int hw,
                    const float* d_lin, const float* d_latents, const float* d_spline,
                    int n_knots, float x_scale, float scale, float* d_loss, float* d_df0,
                    float* d_dlatent, void* d_workspace, void* stream);

/* ---- a11 / a13 trunks: frozen VGG19[0:18] / VGG16 stacks ----------------------- */
/* Replace the torchvision/cuDNN convolution stacks the two patch losses run their inputs
 * through (externel_lib/contextual_loss/modules/vgg.py:16-21,30-36: features[0:18] up to
 * relu3_4; externel_lib/lpips/pretrained_networks.py:96-134: five VGG16 slices), forward and
 * data gradient (the weights are frozen: vgg.py:26-28, pretrained_networks.py:116-118).
 *
 * Between layers tensors stay in a "flat padded" 16-bit layout (csrc/npp_conv.hip): for a
 * logical (N, C, H, W) tensor, [C/8][npp_trunk_nposp(N,H,W)][8] with a zero one-pixel border
 * around every image, so conv2d(padding=1) needs no boundary handling.  Forward activations and
 * forward weight packs are fp16 (saturating; 11 significand bits = the TF32 class cuDNN runs the
 * reference's trunks in), gradient tensors and gradient packs are bf16; accumulation is fp32.  Buffers must be
 * ZERO-INITIALISED by the caller once (kernels rewrite only the position range they compute and
 * keep borders zero).  N_total fixes a buffer's geometry; n_run <= N_total restricts a backward
 * launch to the leading images (the ones that need a gradient).  Limits: W <= 1021 (the guard band of
 * the flat layout), 512 * npp_trunk_nposp * 16 bytes < 2 GiB per tensor; NPP_ERR_ARG beyond them. */
int64_t npp_trunk_nposp(int N, int H, int W);                /* 16-byte units per channel chunk */
int64_t npp_trunk_act_bytes(int N, int C, int H, int W);     /* bytes of a flat tensor (C padded to 16) */

/* Pack a torch Conv2d weight (Cout, Cin, 3, 3) fp32 into bf16 MFMA A-operand fragments:
 * which = 0 forward pack, 1 data-gradient pack (transposed, taps flipped).  in_natural != 0:
 * the layer's input channels are in natural order (the image layer, Cin = 3 padded to 16);
 * otherwise they are in the accumulator order the previous conv layer stored them in. */
int64_t npp_conv_pack_bytes(int Cin, int Cout, int which);
int npp_conv_pack(const float* d_w, int Cin, int Cout, int in_natural, void* d_pack_fwd,
                  void* d_pack_bwd, void* stream);

/* (N,3,H,W) fp32 image -> flat C=16 tensor of x*scale[c] + shift[c] (the reference's input
 * normalisations: contextual.py:56-61 (x-mean)/std; lpips.py:96-98,136-143 scaling layer). */
int npp_trunk_image_in(const float* d_img_nchw, int N, int H, int W, const float scale[3],
                       const float shift[3], void* d_x0, void* stream);

/* npp_patch_compose_fwd + npp_trunk_image_in in ONE launch (NPP_completion/train.py:200-236 followed by
 * contextual.py:56-61): the batch [x | y] of the patch plumbing is written straight into the flat
 * C=16 trunk input d_x0 (2*n_p*k images of P x P, value*scale[c] + shift[c]); d_xy (nullable) also
 * receives it as fp32 (2*n_p*k,3,P,P) for the other consumers of the iteration (LPIPS / style
 * trunks); d_zero[0..n_zero) (n_zero <= 256, nullable) is set to 0 -- the iteration's patch-loss
 * accumulator.  Bit-identical to the two separate calls.  which = 0: both halves (d_x0 holds
 * 2*n_p*k images); 1: only the prediction half x, 2: only the real half y (d_x0 holds n_p*k
 * images; d_xy, if given, is still the full [x | y] tensor and receives that half; the inputs
 * of the other half may be NULL) -- the two halves can then run through the trunk on two streams. */
int npp_trunk_patch_in(const float* d_pred_rows, const float* d_fake, const float* d_fmask,
                       const float* d_real, const float* d_rmask, int n_p, int k, int P, int comp,
                       const float scale[3], const float shift[3], void* d_x0, float* d_xy,
                       float* d_zero, int n_zero, int which, void* stream);
/* The same launch also computing npp_pixel_loss (the arguments of that entry point, in a struct): the two consumers of
 * the forward launch's prediction (train.py:195 and :200-236) are independent, so they share one launch. */
#define NPP_PIXEL_LOSS_SCRATCH_FLOATS (1024 * 8 + 8)
typedef struct {
  const float* pred; const float* gt; const float* mask; int64_t N;
  const float* latents; const float* spline; int32_t n_knots; float x_scale, weight;
  float* loss; float* dpred; float* dlatent;
  /* nullable.  NPP_PIXEL_LOSS_SCRATCH_FLOATS floats, ZEROED once by the caller and then owned by ONE stream.  Given: the launch
   * leaves its per-block partial sums there and does NOT touch loss / dlatent; the Adam launch of the iteration
   * (npp_adam_step_net_pack(_stack), d_pl_partials = this buffer) adds them in block order -- bit-reproducible, and the
   * reduction costs no ticket, fence or launch.  NULL: float atomics onto loss / dlatent in arrival order. */
  float* scratch;
  /* 0: robust_loss_adaptive (the reference's default).  > 0: the non-adaptive switches of models/mse_calculator.py:19-23, both of the
   * form quad * mean(x^2): --loss_type l2 (quad = 1) and robust_loss = lossfun(x, alpha = 2, scale = 0.1) (quad = 50); latents, spline
   * and dlatent are then unused (may be NULL). */
  float quad;
} npp_pixel_loss_args;
int npp_trunk_patch_in_loss(const float* d_pred_rows, const float* d_fake, const float* d_fmask,
                            const float* d_real, const float* d_rmask, int n_p, int k, int P, int comp,
                            const float scale[3], const float shift[3], void* d_x0, float* d_xy,
                            float* d_zero, int n_zero, int which, const npp_pixel_loss_args* loss,
                            void* stream);

/* One 3x3 / pad 1 convolution launch on flat tensors (Cin, Cout multiples of 16, <= 512):
 *  mode 0  y = relu(conv(x, w) + bias)                    nn.Conv2d + nn.ReLU
 *  mode 1  y = conv_transpose(x) * [mask > 0]             dL/d(pre-activation) of the layer below:
 *                                                         x = dL/d(pre-act) of this layer, d_pack its
 *                                                         gradient pack, d_mask the layer-below output
 *  mode 2  y = conv_transpose(x)                          the same without a ReLU gate (into a pooled
 *                                                         tensor or the image)
 * d_tap (nullable): additionally writes the result as plain fp32 (n, Ctap, H, W) for channels
 * < Ctap (times tap_scale[c], Ctap <= 4, when tap_scale is given): feature taps for
 * npp_cx_fwd_bwd / npp_lpips_layer, and the image gradient.  d_y may be NULL if d_tap is set. */
int npp_conv3x3(const void* d_x, int N_total, int n_run, int H, int W, int Cin, int Cout,
                const void* d_pack, const float* d_bias, int mode, const void* d_mask, void* d_y,
                float* d_tap, int Ctap, const float* tap_scale, void* stream);
/* The same, additionally requesting the weight pack of the launch that follows into L2 (d_next_pack may be NULL). */
int npp_conv3x3_pf(const void* d_x, int N_total, int n_run, int H, int W, int Cin, int Cout,
                const void* d_pack, const float* d_bias, int mode, const void* d_mask, void* d_y,
                float* d_tap, int Ctap, const float* tap_scale, const void* d_next_pack, int64_t next_pack_bytes,
                   void* stream);
/* Which kernel form the launch of these arguments takes, decided on the host alone (no GPU, no stream): the struct the launcher
 * itself launches from, under the current npp_tune("conv_wink" / "conv_win" / "conv_wstat") values and the once-read
 * NPP_CONV_TILE.  fold: 0 = npp_conv3x3 / npp_conv3x3_pf, 1 = npp_conv3x3_pool (mode 0, even H and W), 2 = npp_conv3x3_dgrad_pool
 * (mode 2).  Argument errors are the launcher's (bad mode, n_run, channels, geometry -> NPP_ERR_ARG).  out[NPP_CONV_PLAN_N]:
 *   FAMILY  0 = conv3x3_kernel (tile), 1 = conv3x3_win_kernel, 2 = conv3x3_wink_kernel
 *   CT, PT  32-channel and 32-position tiles of one workgroup (win: 2, 8; wink: 2, 4 NPT)
 *   S       waves (tile) or wave groups (wink: 2) the contraction is split over; win: 1
 *   NPT     wink only: position tiles per wave (1 or 2), else 0
 *   WSTAT   1: weight-stationary block numbering (tile family only; GRID_X then counts 8 x ceil(groups / 8) x position blocks)
 *   GRID_X, GRID_Y, LDS (dynamic LDS bytes of the launch) */
enum { NPP_CONV_PLAN_FAMILY = 0, NPP_CONV_PLAN_CT, NPP_CONV_PLAN_PT, NPP_CONV_PLAN_S, NPP_CONV_PLAN_NPT, NPP_CONV_PLAN_WSTAT,
       NPP_CONV_PLAN_GRID_X, NPP_CONV_PLAN_GRID_Y, NPP_CONV_PLAN_LDS, NPP_CONV_PLAN_N };
int npp_conv3x3_plan(int N_total, int n_run, int H, int W, int Cin, int Cout, int mode, int fold, int32_t out[]);

/* nn.MaxPool2d(2,2) on flat tensors, and its backward fused with the ReLU gate of the pooled
 * layer: dz = (route(dy) + addend) * [x > 0]; the gradient goes to the first maximum of each
 * window in scan order (torch semantics); d_addend (nullable) is a tap gradient on x. */
int npp_maxpool2_fwd(const void* d_x, int N, int H, int W, int C, void* d_y, void* stream);
int npp_maxpool2_bwd(const void* d_dy, const void* d_x, const void* d_addend, int N_total,
                     int n_run, int H, int W, int C, void* d_dz, void* stream);
/* npp_conv3x3 mode 2 INTO a pooled tensor followed by npp_maxpool2_bwd, as ONE launch (the pool's backward, the pre-pool
 * ReLU gate and the optional tap gradient ride in the convolution's epilogue; results bit-identical to the two launches).
 * H, W: the pooled geometry (= this convolution's); d_xpre (fp16 activation of the pre-pool layer), d_addend (nullable) and
 * d_dz: flat tensors of geometry (N_total, Cout, 2H, 2W); d_dz's border must be zero (npp_trunk_act buffers are) and is not
 * written.  Replaces the autograd nodes of nn.MaxPool2d + nn.ReLU in the reference's trunks
 * (externel_lib/contextual_loss/modules/vgg.py:20-27, externel_lib/lpips/pretrained_networks.py:96-130). */
/* npp_conv3x3 mode 0 followed by npp_maxpool2_fwd as ONE launch: d_y = relu(conv(x) + bias) (flat fp16, + the optional fp32
 * tap as in npp_conv3x3) and d_ypool = maxpool2x2(d_y), geometry (N_total, Cout, H/2, W/2); H, W even.  Only the n_run leading
 * images are computed / pooled; the borders of both outputs must be zero (npp_trunk_act buffers are) and are not written.
 * Bit-identical to the two launches. */
int npp_conv3x3_pool(const void* d_x, int N_total, int n_run, int H, int W, int Cin, int Cout,
                     const void* d_pack, const float* d_bias, void* d_y, void* d_ypool, float* d_tap, int Ctap,
                     const float* tap_scale, const void* d_next_pack, int64_t next_pack_bytes, void* stream);
/* TWO forward layers and the MaxPool2d(2,2) behind them in ONE launch (round 5): relu(conv a) -> relu(conv b) -> pool, the first
 * blocks of VGG19 / VGG16 (contextual_loss/modules/vgg.py:16-21, lpips/pretrained_networks.py:106-115: features[0:5], [5:10]).  A
 * workgroup owns a 16 x 16 tile of one image; the intermediate activation lives in LDS.  d_y_a / d_y_b (flat fp16, geometry
 * (N_total, Cmid | Cout, H, W)) are written for the first n_keep images only -- what the data-gradient pass reads (ReLU gates, the
 * pool's arg-max source); d_y_pool (geometry (N_total, Cout, H/2, W/2)) and the optional fp32 tap d_tap_b (n_run, Cout, H, W) for
 * all n_run images.  Borders of the outputs are not touched (they are zero from npp_trunk_alloc-style zero initialisation).
 * Bit-identical to npp_conv3x3 x 2 + npp_maxpool2_fwd.  npp_conv_pair_fwd_ok() != 0 says whether a shape is built. */
int npp_conv_pair_fwd_ok(int H, int W, int Cin, int Cmid, int Cout);
int npp_conv_pair_fwd(const void* d_x, int N_total, int n_run, int n_keep, int H, int W, int Cin, int Cmid, int Cout,
                      const void* d_pack_a, const float* d_bias_a, const void* d_pack_b, const float* d_bias_b,
                      void* d_y_a, void* d_y_b, void* d_y_pool, float* d_tap_b, void* stream);
/* npp_trunk_patch_in_loss + npp_conv_pair_fwd in ONE launch (first block; iterations that need no fp32 copy of the batch): the
 * 2 n_p k patches are composed inside the pair's input staging from the prediction rows and the sampler's crops
 * (NPP_completion/train.py:200-236; x * scale + shift), the flat trunk input is never written, and the launch's last blocks are the
 * adaptive pixel loss (`loss` as in npp_trunk_patch_in_loss; NULL: none).  d_zero / n_zero: accumulators cleared on the way.
 * Outputs as npp_conv_pair_fwd with N_total = n_run = 2 n_p k, H = W = P.  Bit-identical to the two launches. */
int npp_conv_pair_fwd_patch(const float* d_pred_rows, const float* d_fake, const float* d_fmask, const float* d_real,
                            const float* d_rmask, int n_p, int k, int P, int comp, const float scale[3], const float shift[3],
                            float* d_zero, int n_zero, const npp_pixel_loss_args* loss, int n_keep, int Cmid, int Cout,
                            const void* d_pack_a, const float* d_bias_a, const void* d_pack_b, const float* d_bias_b,
                            void* d_y_a, void* d_y_b, void* d_y_pool, float* d_tap_b, void* stream);
/* The data gradient of the first block in ONE launch: d_dz_b = dL/d(pre-activation of conv b) (flat bf16, Cmid channels) ->
 * conv b's data gradient -> ReLU gate of conv a (d_y_a: flat fp16 relu(conv a)) -> conv a's data gradient -> d_dimg fp32
 * (n_run, 3, H, W) times scale[c] -- npp_conv3x3 mode 1 (mask = d_y_a) + mode 2 with the fp32 tap, the gated intermediate gradient
 * in LDS (contextual_loss/modules/vgg.py:16-21 / lpips/pretrained_networks.py:106 under autograd).  Packs: the data-gradient packs
 * of npp_conv_pack.  Same arithmetic up to the fp32 summation order of the split-K forms it replaces. */
int npp_conv_pair_dgrad_ok(int H, int W, int Cmid);
int npp_conv_pair_dgrad(const void* d_dz_b, int N_total, int n_run, int H, int W, int Cmid, const void* d_pack_b_bwd,
                        const void* d_y_a, const void* d_pack_a_bwd, float* d_dimg, const float scale[3], void* stream);
int npp_conv3x3_dgrad_pool(const void* d_x, int N_total, int n_run, int H, int W, int Cin, int Cout,
                           const void* d_pack, const void* d_xpre, const void* d_addend, void* d_dz,
                           const void* d_next_pack, int64_t next_pack_bytes, void* stream);

/* Tap gradient (n_run, C, H, W) fp32 -> flat (bf16, or fp16 when as_f16), gated by [y > 0]
 * when the fp16 activation tensor d_y is given; accumulate != 0 adds it onto the gradient already in d_dz
 * (a tap on a tensor that also feeds the next layer).  Also the generic fp32 -> flat importer. */
int npp_trunk_grad_in(const float* d_df_nchw, const void* d_y, int N_total, int n_run, int C,
                      int H, int W, void* d_dz, int as_f16, int accumulate, void* stream);
/* the same, also requesting the weight pack of the data-gradient launch that follows into L2 (like npp_conv3x3_pf) */
int npp_trunk_grad_in_pf(const float* d_df_nchw, const void* d_y, int N_total, int n_run, int C,
                         int H, int W, void* d_dz, int as_f16, int accumulate, const void* d_next_pack,
                         int64_t next_pack_bytes, void* stream);
/* flat (fp16 activations when is_f16, else bf16 gradients) -> (n_run, C, H, W) fp32 */
int npp_trunk_export(const void* d_act, int N_total, int n_run, int C, int H, int W,
                     float* d_out_nchw, int is_f16, void* stream);

/* ---- trunk audit: census of a stored fp16 trunk tensor (csrc/npp_trunk_census.hip) --------------------
 * The numeric contract of csrc/npp_conv.hip: forward activations and weights are fp16, SATURATED at +-65504 (silently: the
 * epilogue clamps, nothing is flagged), gradients are bf16, ReLU gates are taken from the fp16 activations.  The reference runs
 * its trunks in fp32 and has nothing to count.  The census scans what a forward pass left in ONE flat padded fp16 tensor of
 * logical shape (N_total, C, H, W) -- [C/8 chunks][nposp][8], csrc/npp_trunk_layout.h -- and counts the INTERIOR positions
 * (y, x in 1..H, 1..W of the padded image) of images < n and the true channels conv_chan(chunk, j) < c_real; guard, border, tail
 * and padded-channel units are never counted, whatever they hold (the trunk input x0: C = 16, c_real = 3).  The record, int64:
 *   NPP_CENSUS_ELEMENTS, _ZERO (codes 0x0000 / 0x8000), _SUBNORMAL (exponent field 0, mantissa != 0), _AT_MAX (|code| = 0x7BFF =
 *   65504: saturated, or exactly there -- an upper bound on saturations), _NONFINITE (exponent field 0x1F), NPP_CENSUS_HIST + e
 *   (finite codes by exponent field e, 32 bins; bin 0 = zero + subnormal) -- the entry of npp_stash8_census, so that
 *   elements = zero + subnormal + sum of bins 1..30 + nonfinite with at_max inside bin 30 -- then, with d_ref32 given,
 *   NPP_TRUNK_CENSUS_GATE_ON    #(fp16 value > 0): the ReLU gates the data-gradient pass opens
 *   NPP_TRUNK_CENSUS_GATE_FLIPS #((fp16 value > 0) != (fp32 value > 0)), the fp32 partner d_ref32 a plain (>= n, c_real, H, W)
 *                               NCHW tensor (what the exact-fp32 trunk stored for the same layer); both 0 when d_ref32 is NULL.
 * Integer sums only: the record does not depend on the schedule.  npp_trunk16_census clears d_record itself (hipMemsetAsync),
 * then one launch; it allocates nothing and writes nothing else.  npp_trunk16_census_host: the same counts by plain C++ on HOST
 * copies (no GPU needed); it walks the layout's forward map where the kernel inverts it.  1 <= n <= N_total, C % 16 == 0,
 * 1 <= c_real <= C; d_act 16-byte, d_ref32 4-byte, d_record 8-byte aligned. */
#define NPP_TRUNK_CENSUS_GATE_ON NPP_CENSUS_ENTRY_WORDS
#define NPP_TRUNK_CENSUS_GATE_FLIPS (NPP_CENSUS_ENTRY_WORDS + 1)
#define NPP_TRUNK_CENSUS_WORDS (NPP_CENSUS_ENTRY_WORDS + 2)
int64_t npp_trunk16_census_words(void);
int npp_trunk16_census(const void* d_act, int N_total, int n, int C, int c_real, int H, int W, const float* d_ref32,
                       int64_t* d_record, void* stream);
int npp_trunk16_census_host(const void* act, int N_total, int n, int C, int c_real, int H, int W, const float* ref32,
                            int64_t* record);

/* ---- the same trunks in exact fp32 (trunk_precision = "fp32"; csrc/npp_conv32.hip) ------------------------------
 * The diagnostic twin of the launches above: the stacks of externel_lib/contextual_loss/modules/vgg.py:30-36,
 * externel_lib/lpips/pretrained_networks.py:119-134 and models/style_loss.py:11-14 in the arithmetic torch runs them in on
 * the reference's side -- fp32 operands, one rounding per product, fp32 accumulation (v_mfma_f32_32x32x2_f32: a k-ordered
 * fmaf chain).  All tensors are plain fp32 NCHW: a layer's stored output IS the feature tap the loss heads read
 * (npp_cx_fwd_bwd, npp_lpips_layers, npp_gram_fwd), its ReLU gate and the pool's arg-max source.  Implicit GEMM: no column
 * matrix is formed (npp_im2col + npp_linear_fwd would need 9 x the activation per layer and direction).  No float atomics and
 * a fixed summation order (channel chunks of 8, then tap, then channel): two runs give equal bits, and an image's result does
 * not depend on the other images of its batch.  N_total / n_run as in npp_conv3x3: only the leading n_run images are computed.
 * Channel counts: 3 (image layer only), 64, 128, 256, 512; any H, W >= 1.  No weight gradients (vgg.py:26-28). */

/* torch Conv2d weight (Cout, Cin, 3, 3) fp32 -> fp32 MFMA A-operand packs, zero padded to 32 output x 8 input channels:
 * which = 0 forward pack, 1 data-gradient pack (transposed, taps flipped).  Either output of npp_conv32_pack may be NULL. */
int64_t npp_conv32_pack_bytes(int Cin, int Cout, int which);
int npp_conv32_pack(const float* d_w, int Cin, int Cout, float* d_pack_fwd, float* d_pack_bwd, void* stream);

/* One 3x3 / pad 1 / stride 1 convolution launch, d_x (N_total, Cin, H, W) -> d_y (N_total, Cout, H, W):
 *  mode 0  y = relu(conv(x', w) + bias)          nn.Conv2d + nn.ReLU (vgg.py:30-36, pretrained_networks.py:119-134); with
 *                                                in_scale / in_shift (Cin = 3): x' = x * in_scale[c] + in_shift[c] applied on
 *                                                load, BEFORE the zero padding -- contextual.py:56-61, lpips.py:96-98,136-143
 *                                                (not folded into w and bias: torch pads the normalised image with zeros)
 *  mode 1  y = (conv_transpose(x') + add) * [gate > 0]   the autograd node of the same layer: x = dL/d(pre-activation) of this
 *                                                layer (Cin = its output channels), d_pack its data-gradient pack, d_gate the
 *                                                stored output of the layer below (NULL: none -- into a pooled tensor), d_add
 *                                                (nullable) a tap gradient on that tensor; both (N_total, Cout, H, W)
 *  mode 2  y = conv_transpose(x') * out_scale[c]  dL/dimage of the image layer (Cout = 3)
 * d_in_gate (modes 1 / 2, nullable): x' = x * [in_gate > 0] on load -- x is then dL/d(OUTPUT) of this layer and d_in_gate its
 * stored output (the tapped top layer's own ReLU). */
int npp_conv32(const float* d_x, int N_total, int n_run, int H, int W, int Cin, int Cout, const float* d_pack, int mode,
               const float* d_bias, const float in_scale[3], const float in_shift[3], const float* d_in_gate,
               const float* d_gate, const float* d_add, const float out_scale[3], float* d_y, void* stream);

/* nn.MaxPool2d(2, 2) on fp32 NCHW, (N_total, C, H, W) -> (N_total, C, H/2, W/2) (odd sizes floor like torch), and its backward
 * dz = (route(dy) + add) * [x > 0 if gate]: the gradient goes to the first maximum of each window in row-major order (as
 * npp_maxpool2_bwd); d_add (nullable) is a tap gradient on x; gate != 0 applies the ReLU gate of the pooled layer.  One thread
 * per element of x: no atomics.  models/style_loss.py:11-14 taps the pooled tensors themselves. */
int npp_maxpool2_fwd32(const float* d_x, int N_total, int n_run, int H, int W, int C, float* d_y, void* stream);
int npp_maxpool2_bwd32(const float* d_dy, const float* d_x, const float* d_add, int N_total, int n_run, int H, int W, int C,
                       int gate, float* d_dz, void* stream);

/* ---- stacked launches: M independent images of one shape in every launch (round 4) ---------------------------
 * The reference fits its images one after the other (run_completion.sh:8-14: one `python train.py` per directory);
 * the fits are independent -- own weights, own Adam state, own random stream -- so M of them can ride
 * in ONE launch sequence: BASELINE config c3 at fewer than 8 GPUs (8 / 4 / 2 images per GPU), and the cure for the
 * ~5 us every dependent launch of the single-image loop costs.  Every per-image buffer of the entry points above gets a
 * leading image dimension with a fixed stride; what differs per image AND per iteration sits in a device array of M
 * npp_stack_iter the caller uploads once per iteration.  All images share K, width, the row count Bp, n_p, P and the
 * known-pixel row count; an image whose sampler found no valid real patch (train.py:160-161) has active = 0 and is
 * skipped by every launch of that iteration (its Adam step count and LR clock do not advance).
 * Work items are numbered so that an image's workgroups stay on 8 / M of the 8 XCDs (M in {1, 2, 4, 8}): every L2 then
 * keeps one image's weight pack, as in the single-image launch. */
typedef struct {
  int32_t active;        /* 0: the image sits this iteration out */
  int32_t k;             /* real patches per fake patch (models/sampler.py:297-354), 1 on 'same' iterations */
  int32_t comp;          /* 'val' compositing (train.py:230-231) */
  int32_t with_lp;       /* 'same' iteration with the LPIPS term (train.py:241-251) */
  int32_t x0;            /* first image of this fit's prediction half in the stacked trunk batch [x_0..x_{M-1} | y_0..y_{M-1}] */
  int32_t nk;            /* n_p * k (0 when inactive) */
  int32_t same;          /* real patches := fake patches (sampler.py:338) */
  int32_t pad1;
  float step_size;       /* Adam: lr / (1 - beta1^t) of THIS image's step t */
  float inv_sqrt_bc2;    /* 1 / sqrt(1 - beta2^t) */
  float pad2, pad3;
} npp_stack_iter;

/* The embedder constants the fused kernels derive from npp_embed_cfg, as a device-memory blob (one per image of a stack):
 * npp_embed_dev_bytes() bytes each, built on the host by npp_embed_dev_build and uploaded by the caller once per fit. */
int npp_embed_dev_bytes(void);
int npp_embed_dev_build(const npp_embed_cfg* cfg, void* host_out);
/* npp_mlp_fwd over M images: coords (M, Bp, 2), pred (M, Bp, 3); image m's forward pack / parameter blob / stash at
 * + m * stride (bytes / floats / bytes).  d_iter nullable (all active). */
int npp_mlp_fwd_stack(const int32_t* d_coords_yx, int64_t Bp, const void* d_embed_dev, int M, int K, int width,
                      const void* d_wf, int64_t wf_stride_bytes, const float* d_params, int64_t params_stride,
                      float* d_pred, void* d_actF, int64_t act_stride_bytes, const void* d_iter, void* stream);
/* npp_trunk_patch_in_loss over M images.  d_crops (M, n_p + n_p*kmax, 3, P, P): per image [fake | real] as ONE
 * npp_patch_gather writes them; d_cmasks likewise (M, n_p + n_p*kmax, P, P).  The trunk batch is laid out
 * [x_0 .. x_{M-1} | y_0 .. y_{M-1}] (X = sum of the nk images each) inside a flat tensor of FIXED geometry N_total
 * (>= 2 X: 2 M n_p kmax), so the trunk launches run with n_run = 2 X (forward) / X (data gradient).  d_xy (M, 2 n_p kmax,
 * 3, P, P), nullable: fp32 [x | y] of the images with with_lp set.  d_zero: M patch-loss accumulators, cleared.
 * loss: the pixel-loss arguments of image 0; image m at pred / dpred + m Bp 3, gt + m gt_stride, latents / dlatent +
 * m lat_stride, loss + m loss_stride, scratch + m scratch_stride; loss->mask (nullable: per-pixel loss weights of the remapping
 * task, NPP_remapping/train.py:186-190) is (M, loss->N) contiguous. */
int npp_trunk_patch_in_loss_stack(const float* d_pred, int64_t Bp, int64_t row0, const float* d_crops, int64_t crop_stride,
                                  const float* d_cmasks, int64_t cmask_stride, int M, int n_p, int P, int X, int N_total,
                                  const float scale[3], const float shift[3], void* d_x0, float* d_xy, int64_t xy_stride,
                                  float* d_zero, const void* d_iter, const npp_pixel_loss_args* loss, int64_t gt_stride,
                                  int lat_stride, int loss_stride, int64_t scratch_stride, void* stream);
/* npp_cx_fwd_bwd over sample groups (one per image): see csrc/npp_cx.hip. */
int npp_cx_fwd_bwd_groups(const float* d_fx, const float* d_fy, int N, int C, int hw, float band_width, float scale,
                          float* d_loss, int loss_stride, float* d_dfx, const void* d_iter, int M, void* d_workspace,
                          int64_t workspace_bytes, void* stream);
/* npp_cx_fwd_bwd(_groups) delivering dL/dx where the trunk's data-gradient pass reads it: the flat bf16 tensor d_dz (geometry
 * N_total x C x H x W, npp_trunk_act_bytes), gated by the ReLU of the tapped layer (d_yact: its flat fp16 output) -- one launch
 * instead of the core's last one + npp_trunk_grad_in.  d_scratch_dfx (N, C, H*W) fp32: workspace.  M = 0: one group. */
int npp_cx_fwd_bwd_flat(const float* d_fx, const float* d_fy, int N, int C, int H, int W, float band_width, float scale,
                        float* d_loss, int loss_stride, float* d_scratch_dfx, const void* d_yact, void* d_dz, int N_total,
                        const void* d_iter, int M, void* d_workspace, int64_t workspace_bytes, void* stream);
/* npp_mlp_bwd_patch over M images: d_dx_a = dL/d(trunk batch) (only the leading X images are read: image m's at x0),
 * d_dx_b (M, 2 n_p kmax, 3, P, P) nullable = the LPIPS branch's gradient of the images with with_lp set. */
int npp_mlp_bwd_patch_stack(float* d_dpred, const float* d_pred, int64_t Bp, int M, int K, int width, const void* d_wb,
                            int64_t wb_stride_bytes, const float* d_params, int64_t params_stride, const void* d_actF,
                            int64_t act_stride_bytes, void* d_dzF, int64_t dz_stride_bytes, const float* d_dx_a,
                            const float* d_dx_b, int64_t dxb_stride, const float* d_cmasks, int64_t cmask_stride,
                            int64_t row0, int n_p, int P, const void* d_iter, void* stream);
/* npp_mlp_wgrad over M images: image m's ksplit slabs at d_gslabs + m * slab_img_stride floats. */
int npp_mlp_wgrad_stack(const void* d_dzF, int64_t dz_stride_bytes, const void* d_actF, int64_t act_stride_bytes,
                        int64_t Bp, int M, int K, int width, int ksplit, float* d_gslabs, int64_t slab_img_stride,
                        const void* d_iter, void* stream);
/* npp_adam_step_net_pack over M images (step size / bias correction per image from d_iter). */
int npp_adam_step_net_pack_stack(float* d_p, float* d_m, float* d_v, int64_t blob_stride, const float* d_gslabs, int64_t n,
                                 int n_slabs, int64_t slab_stride, int64_t slab_img_stride, float* d_lat, float* d_lat_m,
                                 float* d_lat_v, float* d_dlat, int n_lat, int lat_stride, float* d_zero, int n_zero,
                                 int zero_stride, float beta1, float beta2, float eps, int M, int K, int width, void* d_wf,
                                 int64_t wf_stride_bytes, void* d_wb, int64_t wb_stride_bytes, float* d_pl_partials,
                                 int64_t pl_stride, float* d_loss_cur, const void* d_iter, void* stream);

/* ---- generic dense layers (exact fp32), SURVEY.md 8 f1 -------------------------- */
/* What F.linear + SnakeActivation (models/activations.py:29-35) and their autograd do for topologies the fused chain
 * kernels are not specialised for -- first user: NPP_Net_light of the proposal-ranking fits (models/networks.py:176-263,
 * NPP_proposal/search.py:85-205).  Row-major tensors with explicit leading dimensions (so a layer can write into / read
 * from a column block of a concatenated buffer, networks.py:247 torch.cat); w (out, in) like nn.Linear.
 *  fwd:        y = act(x w^T + b), act 0 none / 1 snake / 2 relu; d_z (nullable) receives the pre-activation
 *  bwd_data:   dx[:, :in_used] (+)= dz w[:, :in_used]
 *  bwd_weight: dw (+)= dz^T x ; db (+)= column sums of dz (d_db nullable)
 *  act_bwd:    dz = dy * act'(.), act 1 snake from z, 2 sigmoid from its output, 3 tanh from its output, 4 relu from z
 *  act_fwd:    y = sigmoid (2) / tanh (3) of x, elementwise (render, models/helpers.py:55-58) */
int npp_linear_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, int64_t B, int in,
                   int out, int act, float* d_y, int64_t ldy, float* d_z, int64_t ldz, void* stream);
int npp_linear_bwd_data(const float* d_dz, int64_t lddz, const float* d_w, int64_t B, int in, int out,
                        float* d_dx, int64_t lddx, int in_used, int accumulate, void* stream);
int npp_linear_bwd_weight(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, int64_t B, int in,
                          int out, float* d_dw, float* d_db, int accumulate, void* stream);
/* The same three forms over nbatch independent problems of ONE shape in one launch -- the proposal-ranking candidates of one
 * image (NPP_proposal/search.py:85-147: each candidate its own NPP_Net_light, all on the same pixel rows): s*b are the element
 * strides between the problems' arrays.  The weight-gradient form ACCUMULATES into d_dw / d_db (split contraction; caller clears).
 * The data-gradient form optionally applies the PREVIOUS layer's activation derivative on the way out (d_zy non-null: d_dx =
 * (d_dz w) * act'(d_zy), act / d_zy as npp_act_bwd takes them; not with accumulate): one launch instead of two per hidden layer. */
int npp_linear_fwd_batched(const float* d_x, int64_t ldx, int64_t sxb, const float* d_w, int64_t swb, const float* d_b,
                           int64_t sbb, int nbatch, int64_t B, int in, int out, int act, float* d_y, int64_t ldy,
                           int64_t syb, float* d_z, int64_t ldz, int64_t szb, void* stream);
int npp_linear_bwd_data_batched(const float* d_dz, int64_t lddz, int64_t sdzb, const float* d_w, int64_t swb, int nbatch,
                                int64_t B, int in, int out, float* d_dx, int64_t lddx, int64_t sdxb, int in_used,
                                int accumulate, const float* d_zy, int64_t ldzy, int64_t szyb, int act, void* stream);
int npp_linear_bwd_weight_batched(const float* d_dz, int64_t lddz, int64_t sdzb, const float* d_x, int64_t ldx, int64_t sxb,
                                  int nbatch, int64_t B, int in, int out, float* d_dw, int64_t sdwb, float* d_db,
                                  int64_t sdbb, void* stream);
/* Weight gradient of nbatch stacked dense layers with EXPLICIT operand strides: dw[b][o][i] += sum_r dz(b, r, o) x(b, r, i),
 * db[b][o] += sum_r dz(b, r, o), where dz(b, r, o) = d_dz[b * sdzb + r * dz_sr + o * dz_so] and x(b, r, i) = d_x[b * sxb + r * x_sr +
 * i * x_si]: row-major operands (s?r = ld, s?o / s?i = 1: the form above) or feature-major ones (s?r = 1: the stashes of the fused
 * chains below).  x_snake != 0: d_x holds PRE-activations and the layer input is snake(d_x) = x + sin^2 x, formed while the operand is
 * staged (the fused chains stash z only).  Accumulates (caller clears). */
int npp_linear_bwd_weight_strided(const float* d_dz, int64_t dz_sr, int64_t dz_so, int64_t sdzb, const float* d_x, int64_t x_sr,
                                  int64_t x_si, int64_t sxb, int x_snake, int nbatch, int64_t B, int in, int out, float* d_dw,
                                  int64_t lddw, int64_t sdwb, float* d_db, int64_t sdbb, void* stream);

/* ---- f1 fused: NPP_Net_light(D = 4, W = 256, snake) forward and data-gradient chains, all candidates of an image in one launch
 * each, exact fp32 (models/networks.py:176-263 with len(freq_scales) == 1; NPP_proposal/search.py:113-147).  The parameter blob of
 * candidate c starts at d_params + c * params_stride; npp_light_desc says where its seven layers live (index 0-3 periodic_linears,
 * 4 pos_linears.0, 5 feature_linear1, 6 rgb_linear; weight [n_out][ld] with ld >= n_in, bias [n_out]).
 * npp_light_pack: the MFMA-ordered copies of the weights the chains stream (forward and transposed), npp_light_pack_floats()
 * floats per candidate; rebuild after every optimiser step.
 * npp_light_fwd: x_per (C, n_src, 20), x_pos (n_src, 42) shared; row r of the batch is table row d_idx[r] (the pixel rows drawn for
 * this iteration, search.py:113-116; d_idx null: r itself, n_src = B) -> d_pred (C, B, 3) = sigmoid(raw) and the FEATURE-major stash
 * (C, npp_light_stash_rows(), B): pre-activations z_0 .. z_3, [f1 | x_pos | 0] (304 rows), z_p -- row offsets by
 * npp_light_stash_row(0..6) = z0 z1 z2 z3 hp zp xper^T (the activations are snake(z): recomputed by their consumers).
 * npp_light_bwd: d_dpred (C, B, 3) = dL/dpred -- or, with d_gt (B, 3) non-null, the adaptive robust pixel loss itself folded in
 * (npp_pixel_loss_batched's arithmetic: d_latents (C, 6), loss words d_loss (C) and latent gradients d_dlatent (C, 6) accumulated,
 * d_dpred unused) -> d_draw (C, B, 3) = dL/draw and the gradient stash (C, npp_light_dstash_rows(), B):
 * d z_0 .. d z_3, d f1, d z_p, d raw^T (npp_light_dstash_row(0..6)).  The weight gradients: npp_light_wgrad (or
 * npp_linear_bwd_weight_strided layer by layer) over the two stashes.  B a multiple of 32 (workgroups of 64 or 32 rows, whichever loads the CUs more evenly; NPP_LIGHT_ROWS forces one). */
typedef struct {
  int64_t w_off[7], b_off[7];
  int32_t n_out[7], n_in[7], ld[7];
} npp_light_desc;
int64_t npp_light_pack_floats(void);
int64_t npp_light_stash_rows(void);
int64_t npp_light_dstash_rows(void);
int npp_light_stash_row(int which);
int npp_light_dstash_row(int which);
int npp_light_pack(const npp_light_desc* L, const float* d_params, int64_t params_stride, int C, float* d_pack, int64_t pack_stride,
                   void* stream);
int npp_light_fwd(const npp_light_desc* L, const float* d_params, int64_t params_stride, const float* d_pack, int64_t pack_stride,
                  const float* d_x_per, const float* d_x_pos, const int64_t* d_idx, int64_t n_src, int C, int64_t B, float* d_stash,
                  float* d_pred, void* stream);
/* optimizer.step() (Adam over the stacked blobs and the candidates' six latents each, npp_adam_step_net's arithmetic), zero_grad()
 * (d_grad, d_dlat and the C loss words d_zero cleared) and the re-pack of every updated weight (npp_light_pack's layout) in ONE launch.
 * n: live floats per candidate (<= stride). */
int npp_light_adam_pack(const npp_light_desc* L, float* d_params, float* d_m, float* d_v, float* d_grad, int64_t stride, int64_t n, int C,
                        float* d_pack, int64_t pack_stride, float* d_lat, float* d_lat_m, float* d_lat_v, float* d_dlat, float* d_zero,
                        float lr, float beta1, float beta2, float eps, int step, void* stream);
/* The seven weight / bias gradients of all candidates in one launch over the two stashes: into d_grad + c * grad_stride at the
 * parameters' own offsets (accumulated; clear first). */
int npp_light_wgrad(const npp_light_desc* L, const float* d_stash, const float* d_dstash, int C, int64_t B, float* d_grad,
                    int64_t grad_stride, void* stream);
int npp_light_bwd(const npp_light_desc* L, const float* d_params, int64_t params_stride, const float* d_pack, int64_t pack_stride,
                  const float* d_stash, const float* d_pred, const float* d_dpred, const float* d_gt, const float* d_latents,
                  const float* d_spline, int n_knots, float x_scale, float* d_loss, float* d_dlatent, int C, int64_t B,
                  float* d_draw, float* d_dstash, void* stream);
/* Bit-reproducible forms (round 6; the reference's candidate fits are not -- cuBLAS / atomics -- but rankings with near-equal scores
 * should not depend on arrival order): npp_light_bwd_det = npp_light_bwd with the pixel loss folded in (d_gt required) whose per-block
 * loss / latent-gradient sums go to d_part (C, npp_light_part_blocks(C, B), 8) by plain stores; npp_light_adam_pack_det adds them in
 * block order (latent gradients = d_dlat + the blocks' sums; d_loss_cur[c] += the blocks' loss terms, nullable).  With
 * npp_tune("light_det") = 1 (default) npp_light_wgrad does not split its contraction (no float atomicAdd): the whole candidate fit
 * has no order-dependent float sum left.  NPP_proposal/search.py:113-147. */
int npp_light_part_blocks(int C, int64_t B);
/* npp_light_wgrad with its contraction split over enough workgroups to fill the chip (a single candidate is 80 output tiles: 80
 * workgroups walking 2048 rows each when unsplit) AND bit-reproducible: the row ranges of an output tile leave their partial tiles in
 * d_scratch, the workgroup that arrives last adds them in range order and is the tile's only writer (no float atomicAdd).
 * d_scratch: npp_light_wgrad_det_scratch_bytes(C, B) bytes, ZEROED once before the first use (the arrival tickets reset themselves). */
int64_t npp_light_wgrad_det_scratch_bytes(int C, int64_t B);
int npp_light_wgrad_det(const npp_light_desc* L, const float* d_stash, const float* d_dstash, int C, int64_t B, float* d_grad,
                        int64_t grad_stride, float* d_scratch, int64_t scratch_bytes, void* stream);
/* "multi" forms: candidate c = ONE IMAGE's fit (the searches of several images of a rank advanced in one launch sequence: candidate k of
 * every image together, where run_completion.sh / search.py:85-215 walk images and candidates one after the other): per candidate its own
 * positional table d_x_pos (C, n_src, 42), periodic table d_x_per (C, n_src, 20) as before, pixel rows d_idx (C, B) into its own tables
 * (shorter tables padded to n_src rows) and targets d_gt (C, B, 3). */
int npp_light_fwd_multi(const npp_light_desc* L, const float* d_params, int64_t params_stride, const float* d_pack, int64_t pack_stride,
                        const float* d_x_per, const float* d_x_pos, const int64_t* d_idx, int64_t n_src, int C, int64_t B, float* d_stash,
                        float* d_pred, void* stream);
int npp_light_bwd_det_multi(const npp_light_desc* L, const float* d_params, int64_t params_stride, const float* d_pack, int64_t pack_stride,
                            const float* d_stash, const float* d_pred, const float* d_gt, const float* d_latents, const float* d_spline,
                            int n_knots, float x_scale, float* d_part, int C, int64_t B, float* d_draw, float* d_dstash, void* stream);
int npp_light_bwd_det(const npp_light_desc* L, const float* d_params, int64_t params_stride, const float* d_pack, int64_t pack_stride,
                      const float* d_stash, const float* d_pred, const float* d_gt, const float* d_latents, const float* d_spline,
                      int n_knots, float x_scale, float* d_part, int C, int64_t B, float* d_draw, float* d_dstash, void* stream);
int npp_light_adam_pack_det(const npp_light_desc* L, float* d_params, float* d_m, float* d_v, float* d_grad, int64_t stride, int64_t n,
                            int C, float* d_pack, int64_t pack_stride, float* d_lat, float* d_lat_m, float* d_lat_v, float* d_dlat,
                            float* d_zero, float lr, float beta1, float beta2, float eps, int step, const float* d_part, int n_part,
                            float* d_loss_cur, void* stream);
/* ---- f1 on the 16-bit matrix pipe (csrc/npp_light16.hip): the same chains with bf16 operands, fp32 accumulation and fp32 master
 * weights -- the numeric contract of the main loop's coordinate MLP (npp_mlp_fwd / npp_mlp_bwd / npp_mlp_wgrad), models/networks.py:176-263,
 * NPP_proposal/search.py:113-147.  B a multiple of 64.  Per candidate: a bf16 pack of npp_light16_pack_bytes() bytes (forward and
 * transposed weights), a forward stash of npp_light16_stash_bytes(B, 0) bytes (W-format fragment arrays: fp16 pre-activations z_0..z_3,
 * z_p, bf16 [f1 | x_pos], x_per) and a gradient stash of npp_light16_stash_bytes(B, 1) bytes (bf16 d z_0..d z_3, d f1, d z_p, d raw);
 * the strides (bytes, multiples of 16) place candidate c at + c * stride.
 * npp_light16_fwd: as npp_light_fwd.  npp_light16_bwd: as npp_light_bwd (d_gt non-null folds the adaptive robust pixel loss in).
 * npp_light16_wgrad: all seven weight / bias gradients of the C <= NPP_MAX_STACK candidates in ONE launch of the main loop's grouped
 * split-K kernel: candidate c's ksplit partial sums land, by plain stores, in d_gslabs + c * slab_cand_stride + s * slab_stride
 * (s < ksplit) at the parameters' own offsets (npp_light_desc; leading dimensions and offsets multiples of 4, pos_linears.0 stored 300
 * wide).  npp_light16_adam_pack: optimizer.step() over the stacked fp32 blobs with gradient = the slabs summed in slab order
 * (bit-reproducible), the six latents per candidate (d_dlat consumed and cleared, loss words d_zero cleared) and the re-pack of every
 * updated weight into the bf16 packs, one launch. */
int64_t npp_light16_pack_bytes(void);
int64_t npp_light16_stash_bytes(int64_t B, int which);
int npp_light16_pack(const npp_light_desc* L, const float* d_params, int64_t params_stride, int C, void* d_pack, int64_t pack_stride_bytes,
                     void* stream);
int npp_light16_fwd(const npp_light_desc* L, const float* d_params, int64_t params_stride, const void* d_pack, int64_t pack_stride_bytes,
                    const float* d_x_per, const float* d_x_pos, const int64_t* d_idx, int64_t n_src, int C, int64_t B, void* d_actF,
                    int64_t act_stride_bytes, float* d_pred, void* stream);
int npp_light16_bwd(const npp_light_desc* L, const float* d_params, int64_t params_stride, const void* d_pack, int64_t pack_stride_bytes,
                    const void* d_actF, int64_t act_stride_bytes, const float* d_pred, const float* d_dpred, const float* d_gt,
                    const float* d_latents, const float* d_spline, int n_knots, float x_scale, float* d_loss, float* d_dlatent, int C,
                    int64_t B, void* d_dzF, int64_t dz_stride_bytes, void* stream);
int npp_light16_wgrad(const npp_light_desc* L, const void* d_actF, int64_t act_stride_bytes, const void* d_dzF, int64_t dz_stride_bytes,
                      int C, int64_t B, int ksplit, float* d_gslabs, int64_t slab_stride, int64_t slab_cand_stride, void* stream);
int npp_light16_adam_pack(const npp_light_desc* L, float* d_params, float* d_m, float* d_v, int64_t stride, int64_t n, int C,
                          const float* d_gslabs, int n_slabs, int64_t slab_stride, int64_t slab_cand_stride, void* d_pack,
                          int64_t pack_stride_bytes, float* d_lat, float* d_lat_m, float* d_lat_v, float* d_dlat, float* d_zero, float lr,
                          float beta1, float beta2, float eps, int step, void* stream);
/* (round 6) the 16-bit candidate fits, bit-reproducible and across images -- what npp_light_bwd_det / npp_light_adam_pack_det /
 * npp_light_fwd_multi are to the fp32 chains.  npp_light16_bwd_det: the pixel loss folded in (d_gt required), every block's seven loss /
 * latent-gradient sums to d_part (C, B / 64, 8) by plain stores; gt_cs = elements per candidate of d_gt (0: one (B, 3) target shared;
 * 3 B: candidate c = one image's fit with its own targets).  npp_light16_adam_pack_det adds them in block order (latent gradients =
 * d_dlat + the sums; d_loss_cur[c] += the loss terms, nullable).  npp_light16_fwd_multi: per candidate its own positional table
 * d_x_pos (C, n_src, 42) and pixel rows d_idx (C, B).  NPP_proposal/search.py:85-215. */
int npp_light16_fwd_multi(const npp_light_desc* L, const float* d_params, int64_t params_stride, const void* d_pack,
                          int64_t pack_stride_bytes, const float* d_x_per, const float* d_x_pos, const int64_t* d_idx, int64_t n_src,
                          int C, int64_t B, void* d_actF, int64_t act_stride_bytes, float* d_pred, void* stream);
int npp_light16_bwd_det(const npp_light_desc* L, const float* d_params, int64_t params_stride, const void* d_pack,
                        int64_t pack_stride_bytes, const void* d_actF, int64_t act_stride_bytes, const float* d_pred,
                        const float* d_gt, int64_t gt_cs, const float* d_latents, const float* d_spline, int n_knots, float x_scale,
                        float* d_part, int C, int64_t B, void* d_dzF, int64_t dz_stride_bytes, void* stream);
int npp_light16_adam_pack_det(const npp_light_desc* L, float* d_params, float* d_m, float* d_v, int64_t stride, int64_t n, int C,
                              const float* d_gslabs, int n_slabs, int64_t slab_stride, int64_t slab_cand_stride, void* d_pack,
                              int64_t pack_stride_bytes, float* d_lat, float* d_lat_m, float* d_lat_v, float* d_dlat, float* d_zero,
                              float lr, float beta1, float beta2, float eps, int step, const float* d_part, int n_part,
                              float* d_loss_cur, void* stream);
/* img2mse with --loss_type l2 (coef = 1) or robust_loss (coef = 50: lossfun(diff, alpha = 2, scale = 0.1) = 0.5 (diff / 0.1)^2),
 * models/mse_calculator.py:13-27, for nbatch problems: d_loss[b] += weight * coef * mean(x^2), d_dpred = its gradient; the (N) mask
 * (nullable) is shared, the targets too when gt_stride == 0. */
int npp_pixel_loss_quad(const float* d_pred, const float* d_gt, int64_t gt_stride, const float* d_mask, int64_t N, int nbatch, float coef,
                        float weight, float* d_loss, float* d_dpred, void* stream);
/* npp_pixel_loss over nbatch problems: d_pred / d_dpred (nbatch, N, 3), d_latents / d_dlatent (nbatch, 6), d_loss (nbatch);
 * the targets d_gt (N, 3) are shared when gt_stride == 0, else problem b reads d_gt + b * gt_stride. */
int npp_pixel_loss_batched(const float* d_pred, const float* d_gt, int64_t gt_stride, int64_t N, int nbatch,
                           const float* d_latents, const float* d_spline, int n_knots, float x_scale, float weight,
                           float* d_loss, float* d_dpred, float* d_dlatent, void* stream);
int npp_act_bwd(const float* d_dy, int64_t lddy, const float* d_zy, int64_t ldzy, int64_t B, int n, int act,
                float* d_dz, int64_t lddz, void* stream);
int npp_act_fwd(const float* d_x, int64_t n, int act, float* d_y, void* stream);
/* LPIPS.forward(use_robust=False), one VGG16 tap, forward only (externel_lib/lpips/lpips.py:99-101,110,117,130; the
 * candidate score of NPP_proposal/search.py:193): d_out[0] += scale * sum_n mean_pos sum_c lin_c (f0n - f1n)^2. */
int npp_lpips_plain_layer(const float* d_f0, const float* d_f1, int N, int C, int hw, const float* d_lin,
                          float scale, float* d_out, void* stream);
/* The same with the workgroups' partial sums added in block order instead of by float atomics (the candidate SCORES that rank the
 * proposals, NPP_proposal/search.py:193, are then bit-reproducible): d_scratch = NPP_LPIPS_PLAIN_SCRATCH_FLOATS floats, zeroed once by
 * the caller.  Layout: 256 partial-sum slots (a launch uses the first min(256, ceil(N hw / 16))), then the arrival counter at the
 * fixed slot 256, which every launch leaves at zero: one scratch serves successive launches of any (N, hw).  Launches that may
 * run concurrently need scratches of their own. */
#define NPP_LPIPS_PLAIN_SCRATCH_FLOATS 264
int npp_lpips_plain_layer_det(const float* d_f0, const float* d_f1, int N, int C, int hw, const float* d_lin, float scale, float* d_out,
                              float* d_scratch, void* stream);

/* ---- remapping variant: Gram-matrix style loss (models/style_loss.py:37-74) ----------------- */
/* G[n] = F[n] F[n]^T for (N, C, hw) features and its backward dF[n] = (dG[n] + dG[n]^T) F[n]; the per-element adaptive
 * robust NLL of a - b over (N, D) with D latent pairs (AdaptiveLossFunction(num_dims = C^2), style_loss.py:23-27,60-69):
 * d_loss[0] += sum_n coef_n[n] sum_j nll(a - b)[n][j]; d_diff (N, D) scratch; d_ddiff / d_dlatent (nullable together):
 * coef_n dnll/dx and the accumulated latent gradients.  coef_n is a HOST array of N <= 64 factors. */
int npp_gram_fwd(const float* d_f, int N, int C, int hw, float* d_g, void* stream);
/* (round 6) the same with the split contraction's partial sums added in range order: bit-reproducible where npp_gram_fwd adds them with
 * float atomics in arrival order.  Two launches: the ranges leave their partial tiles in d_scratch, a small second launch adds them.
 * d_scratch: npp_gram_fwd_det_scratch_bytes(N, C, hw) bytes, no initial content required, not shared by launches that may run
 * concurrently. */
int64_t npp_gram_fwd_det_scratch_bytes(int N, int C, int hw);
int npp_gram_fwd_det(const float* d_f, int N, int C, int hw, float* d_g, float* d_scratch, int64_t scratch_bytes, void* stream);
int npp_gram_bwd(const float* d_dg, const float* d_f, int N, int C, int hw, float* d_df, void* stream);
/* (round 6) ONE launch: the per-channel constants, the difference a - b (written to d_diff) and the loss are all formed inside it
 * -- nothing is handed from one launch to the next through the workspace, which now holds only the blocks' loss partials and their
 * arrival ticket (the launcher clears the ticket itself; no initial content required; not shared by concurrent launches). */
int64_t npp_robust_elem_workspace_bytes(int D);
int npp_robust_elem(const float* d_a, const float* d_b, int N, int D, const float* d_latents,
                    const float* d_spline, int n_knots, float x_scale, const float* coef_n, float* d_loss,
                    float* d_diff, float* d_ddiff, float* d_dlatent, void* d_workspace, void* stream);

/* ---- SURVEY.md 8 f3 / f4 front ends: around the AlexNet convolutions ------------------------ */
/* (round 6) The segmentation task's LPIPS(alex, spatial = True) criterion (NPP_segmentation/train.py:361-372; externel_lib/lpips/
 * lpips.py:92-133, pretrained_networks.py alexnet slices) and the proposal search's conv1 features (NPP_proposal/feature_searching.py:
 * 20-24) run their convolutions as im2col rows x npp_linear_fwd; these are the pieces around the products (torch calls before).
 * Activations between the layers are POSITION-MAJOR (n, y, x, c) -- what npp_linear_fwd writes for rows (n, y, x).
 * npp_im2col: rows (n, oy, ox), columns (c, ky, kx) (torch.nn.functional.unfold's order = the (Cout, Cin k k) weight matrix's), zeros
 *   outside the image; nhwc != 0: d_x is position-major, else (N, C, H, W).  d_cols: N ho wo x C k k floats, ho = (H + 2 pad - k) / stride + 1.
 * npp_maxpool_nhwc: nn.MaxPool2d(k, stride) (no padding, floor size) on a position-major tensor; NaN propagates.
 * npp_lpips_spatial_layer: one tap of LPIPS.forward(spatial = True, use_robust = False) before the upsampling: d_map[p] = sum_c lin_c
 *   (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 for P positions of C channels (lpips.py:99-110, lpips/__init__.py:42-44).
 * npp_resize_bilinear: F.interpolate(size = (H, W), mode = 'bilinear', align_corners = False) of N maps (h, w) (lpips.py:20-22);
 *   accumulate != 0 adds into d_y (lpips.py:125-127 sums the taps). */
int npp_im2col(const float* d_x, int N, int C, int H, int W, int k, int stride, int pad, int nhwc, float* d_cols, void* stream);
int npp_maxpool_nhwc(const float* d_x, int N, int H, int W, int C, int k, int stride, float* d_y, void* stream);
int npp_lpips_spatial_layer(const float* d_f0, const float* d_f1, int64_t P, int C, const float* d_lin, float* d_map, void* stream);
int npp_resize_bilinear(const float* d_x, int N, int h, int w, int H, int W, int accumulate, float* d_y, void* stream);

/* ---- brute-force displacement search ------------------------------------- */
/* compute_loss of NPP_proposal/feature_searching.py:208-264: act (C, h, w) fp32 feature map whose LAST channel is excluded
 * from the sum (:247,250), mask (h, w) 1 = known, shifts (n, 2) int32 (dx, dy).  losses[s] = sum over positions of
 * mask * shifted mask * sum_c f(shifted act, act), f = -a*b when edge_searching else (a-b)^2; zero outside the map. */
int npp_shift_search(const float* d_act_chw, const float* d_mask_hw, int C, int h, int w,
                     const int32_t* d_shifts_xy, int n, int edge_searching, float* d_losses, void* stream);

/* ---- segmentation task: the per-pixel half of the initial coarse segmentation ------------------ */
/* loaders/loaders.py:162-205 runs SLIC superpixels, per-superpixel colour statistics, a Gaussian mixture and a graph cut before
 * the fit; the per-pixel work is here, the per-superpixel work (a few hundred nodes) on the host (init_segment.py).  Every entry
 * is bit-reproducible: member sums are integer sums.  Images are (H, W, 3) uint8 RGB; Lab planes are (3, H, W) fp32; labels are
 * (H, W) int32 with 0 = outside the mask and k + 1 = centre / superpixel k; centres are (K, 5) fp32 rows (y, x, L, a, b).
 * npp_slic_prepare (loaders.py:152, imsegm/superpixels.py:53-64 -> skimage.segmentation.slic(sigma = 1, convert2lab)): scale to
 *   [0, 1] by (v - vmin) / (vmax - vmin), Gaussian blur sigma = 1 per channel (separable, reflect border, truncated at 4 sigma),
 *   sRGB -> CIELAB (D65), divided by the compactness m = (sp_size * sp_regul)^1.5 (superpixels.py:59).  d_tmp_3hw: 3 H W floats.
 * npp_slic_assign (the assignment step of skimage's _slic_cython): every mask pixel takes the centre minimising
 *   D2 = |Lab_p - Lab_k|^2 + |p - c_k|^2 / S^2 among the centres within +-2S of it on both axes, lowest k on a tie; a mask pixel
 *   with no centre in that window takes the nearest of all centres by the same D2.
 * npp_slic_update (its update step): every centre becomes the mean (y, x, L, a, b) of its members; no members: unchanged.  The
 *   Lab values enter their sums rounded to 2^-20.  d_scratch: npp_slic_update_scratch_bytes(K) bytes, no initial content required.
 * npp_slic_features (imsegm/pipelines.py:253-278, descriptors.py:787-858: 'color': mean, median, meanGrad): per superpixel
 *   1..N of ANY label image (no bounding window assumed; labels outside 1..N are skipped) the member count and a row of 11
 *   floats: centroid (y, x), per-channel mean of the 0..255 values, exact per-channel median (256-bin histogram; the mean of the
 *   two middle values for an even count, as np.median), per-channel mean of np.gradient(ch)[0] + np.gradient(ch)[1].  A label
 *   without pixels gives count 0 and NaN.  H, W >= 2.  d_scratch: npp_slic_features_scratch_bytes(N) bytes, as above. */
int npp_slic_prepare(const uint8_t* d_img_hw3, int H, int W, float vmin, float vmax, float m, float* d_tmp_3hw, float* d_lab_3hw,
                     void* stream);
int npp_slic_assign(const float* d_lab_3hw, const uint8_t* d_mask_hw, int H, int W, const float* d_centres_k5, int K, float S,
                    int32_t* d_labels_hw, void* stream);
int64_t npp_slic_update_scratch_bytes(int K);
int npp_slic_update(const float* d_lab_3hw, const int32_t* d_labels_hw, int H, int W, float* d_centres_k5, int K, void* d_scratch,
                    int64_t scratch_bytes, void* stream);
int64_t npp_slic_features_scratch_bytes(int N);
int npp_slic_features(const uint8_t* d_img_hw3, const int32_t* d_labels_hw, int H, int W, int N, int32_t* d_count_n, float* d_feat_n11,
                      void* d_scratch, int64_t scratch_bytes, void* stream);

/* ---- remapping task: blur detection (NPP_remapping/blur_detection.py:13-60) ------------------------------------------------ */
/* The per-pixel work of get_blur_map; the normalisation and the percentile between the share and the morphology are the caller's
 * (blur.py).  No entry keeps state in device memory between launches and none uses atomics: results are bit-reproducible.
 * npp_rgb_to_gray_u8 (blur_detection.py:14, cv2.cvtColor(img, COLOR_RGB2GRAY) on uint8): (H, W, 3) -> (H, W),
 *   (R 4899 + G 9617 + B 1868 + 8192) >> 14, OpenCV's 14-bit fixed point; exact.
 * npp_blur_sv_share (blur_detection.py:32-46): per pixel (i, j), sum(s[:sv_num]) / (sum(s) + 1e-6) with s the singular values of
 *   the 20 x 20 block new_img[i:i+20, j:j+20] of the padded image of :15-30, gathered through the reference's own index map
 *   (rows 10 - i for i < 10, rows 2H - i for i > H + 9, counted from the end where that is negative; columns alike) and never
 *   materialised.  float64 one-sided Jacobi, float64 out.  The window is fixed (win_size = 10); H, W > 10; sv_num in 1..20.
 * npp_binary_morph (blur_detection.py:54-56, scipy.ndimage.binary_erosion / binary_dilation(iterations), default 4-connected
 *   cross, border_value 0): (H, W) uint8 (non-zero = set) -> (H, W) uint8 0 / 1 after `iterations` (1..254) erosions (dilate = 0:
 *   eats inwards from the image border) or dilations (dilate = 1), as ONE pass with the L1 ball of that radius.  d_tmp_hw: H W
 *   bytes of its own, no initial content required; d_out_hw may be d_in_hw. */
int npp_rgb_to_gray_u8(const uint8_t* d_img_hw3, int H, int W, uint8_t* d_gray_hw, void* stream);
int npp_blur_sv_share(const uint8_t* d_gray_hw, int H, int W, int sv_num, double* d_share_hw, void* stream);
int npp_binary_morph(const uint8_t* d_in_hw, int H, int W, int iterations, int dilate, uint8_t* d_tmp_hw, uint8_t* d_out_hw,
                     void* stream);

/* ---- segmentation task: 4-connected components (regions.py; csrc/npp_regions.hip) ------------------------------- */
/* The input is an (H, W) int32 LABEL IMAGE: 0 = outside, any other value a class; two pixels are connected when they are 4-neighbours
 * carrying the same non-zero value (a binary mask: every set value 1).  H, W >= 1 and H W < 2^31, otherwise arbitrary (1 x W and H x 1
 * included; no multiple of any tile).  No entry keeps state in device memory between launches; scratch is the caller's, its size is
 * stated by the entry and it needs no initial content; every sum is an integer sum: two calls give identical bits.  Bad arguments:
 * NPP_ERR_ARG and a message, nothing launched.
 * npp_cc_label: d_root_hw (H, W) int32 (an array of its own) = -1 where the input is 0, elsewhere the SMALLEST row-major index
 *   i W + j of the pixel's component: a pure function of the input, whatever the launch schedule.  Three launches (tiles in LDS, the
 *   pairs across tile borders by device-scope atomics, every pixel to its root); H <= 65535 * 16.
 * npp_cc_number: roots -> numbers 1..C in ascending root order = raster order of first appearance (a root is its component's first
 *   pixel in raster order), 0 outside: the numbering of scipy.ndimage.label.  *d_count = C (a device word).  d_numbered_hw may be
 *   d_root_hw.  d_scratch: npp_cc_number_scratch_bytes(H, W) bytes, 4-byte aligned.
 * npp_cc_stats: per component c = 1..C of a numbered image, at index c - 1: d_size_c int64 pixel count; d_sums_cn (C, nch) int64 sums
 *   of the nch <= 4 channels of the (H, W, nch) uint8 image d_values_hwc (nch = 0: no image, no sums); d_box_c4 (C, 4) int32 bounding
 *   box (first row, first column, last row, last column), (INT_MAX, INT_MAX, -1, -1) for a number without pixels; d_border_c one byte,
 *   1 = the component touches the image border.  Numbers outside 1..C are skipped.  The entry initialises its outputs itself.
 * npp_cc_*_host: the same definitions in plain C++ on host memory, no GPU. */
int npp_cc_label(const int32_t* d_labels_hw, int H, int W, int32_t* d_root_hw, void* stream);
int64_t npp_cc_number_scratch_bytes(int H, int W);
int npp_cc_number(const int32_t* d_root_hw, int H, int W, int32_t* d_numbered_hw, int32_t* d_count, void* d_scratch, int64_t scratch_bytes,
                  void* stream);
int npp_cc_stats(const int32_t* d_numbered_hw, int H, int W, int C, const uint8_t* d_values_hwc, int nch, int64_t* d_size_c,
                 int64_t* d_sums_cn, uint8_t* d_border_c, int32_t* d_box_c4, void* stream);
int npp_cc_label_host(const int32_t* labels_hw, int H, int W, int32_t* root_hw);
int npp_cc_number_host(const int32_t* root_hw, int H, int W, int32_t* numbered_hw, int32_t* count);
int npp_cc_stats_host(const int32_t* numbered_hw, int H, int W, int C, const uint8_t* values_hwc, int nch, int64_t* size_c,
                      int64_t* sums_cn, uint8_t* border_c, int32_t* box_c4);

/* ---- completion task: the image work in front of the periodicity search (frontend.py; csrc/npp_frontend.hip) ----- */
/* The per-pixel steps of NPP_proposal/feature_searching.py:14-75 and utils/miscs.py:53-96 behind `--front_end gpu`, each defined by
 * its host twin in cvlite.py / scipy and equal to it bit for bit.  The image and mask kernels are integer arithmetic; the resize
 * index rules and the normalisation are float64 in the host's operation order without contraction; there are no float atomics and
 * no entry keeps state in device memory between calls: every result is a PURE FUNCTION OF ITS INPUT, whatever the launch schedule.
 * (C, h, w) entries put the channel in a grid dimension (C <= 65535): 66 channels are one launch sequence.  h w < 2^31.  Bad
 * arguments (null pointers included): NPP_ERR_ARG and a message that names the entry, nothing launched.
 * npp_resize_nearest_u8 / npp_resize_linear_u8: (H, W) uint8 -> (h, w) uint8 (an array of its own) as cv2.resize with INTER_NEAREST
 *   (source index min(trunc(dst (src / dst_size)), src - 1)) / INTER_LINEAR (11-bit tap table built in the kernel, vertical pass
 *   (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2): cvlite.resize_nearest / cvlite.resize_linear_u8.
 * npp_normalize_u8: per channel of a (C, h, w) fp32 map, min and max in float64, then uint8((a - mn) / rng 255) in that order;
 *   rng = 1 for a constant channel (all zeros out): cvlite.normalize_to_uint8.
 * npp_gaussian_blur3_u8: weights [1 2 1]^2, BORDER_REFLECT_101, (v + 8) >> 4, out of place: cvlite.gaussian_blur3_u8.
 * npp_canny_mark: cvlite.canny_u8 up to the hysteresis in ONE launch -- Sobel with replicated border, |dx| + |dy|, the integer
 *   tangent test (13573 / 2^15) with OpenCV's strict / non-strict comparisons, zero magnitude outside the map -- d_map_chw (an array
 *   of its own) = 0, 1 (kept and > low) or 2 (kept and > high).
 * npp_canny_hysteresis: `rounds` (1..1024) launches that spread the mark 2 to 8-connected pixels marked 1, tile by tile in LDS;
 *   d_flags[r] (int32, cleared by the entry) = 1 when round r marked a pixel.  Repeat the call until the last flag reads 0: the
 *   map is then the unique fixed point, whatever the order in which the tiles ran.
 * npp_canny_finish: 2 -> 255, else 0 (d_out_chw may be d_map_chw).
 * npp_edge_count: d_out_hw (h, w) fp32 = the number of channels marked 2 at the pixel where d_eroded_hw is non-zero, else 0 (the
 *   sum over channels of Canny / 255 inside the mask eroded by npp_binary_morph: proposal.act2edge).
 * npp_edt_sq: d_dsq_hw (H, W) int32 = the exact SQUARED Euclidean distance of every pixel to the nearest zero pixel of the (H, W)
 *   uint8 mask (the image border is not a zero, as in scipy.ndimage.distance_transform_edt).  H, W <= 32767.  d_tmp_hw: H W words of
 *   its own, no initial content required.  The mask must hold a zero pixel (the caller checks; without one every distance reads 2^31).
 * npp_far_points: the greedy walk of utils/miscs.py:53-96 over the pixels in the order LARGEST d^2 FIRST, TIES BY SMALLEST ROW-MAJOR
 *   INDEX (np.argsort(-d, kind="stable")), as topk (1..16) rounds of a two-stage argmax in a fixed order: a round accepts the first
 *   pixel after the last accepted one whose squared distance to every accepted pixel is >= n_min (integers only), and a round that
 *   finds none accepts none.  d_record int32[2 + 2 topk] (cleared by the entry): [0] accepted count, [1] 0, then (index, d^2) pairs.
 *   d_scratch: NPP_FAR_POINTS_SCRATCH_BYTES bytes, 8-byte aligned, no initial content required. */
#define NPP_FAR_POINTS_SCRATCH_BYTES 2048
int npp_resize_nearest_u8(const uint8_t* d_in_hw, int H, int W, uint8_t* d_out_hw, int h, int w, void* stream);
int npp_resize_linear_u8(const uint8_t* d_in_hw, int H, int W, uint8_t* d_out_hw, int h, int w, void* stream);
int npp_normalize_u8(const float* d_in_chw, int C, int h, int w, uint8_t* d_out_chw, void* stream);
int npp_gaussian_blur3_u8(const uint8_t* d_in_chw, int C, int h, int w, uint8_t* d_out_chw, void* stream);
int npp_canny_mark(const uint8_t* d_img_chw, int C, int h, int w, int low, int high, uint8_t* d_map_chw, void* stream);
int npp_canny_hysteresis(uint8_t* d_map_chw, int C, int h, int w, int rounds, int32_t* d_flags, void* stream);
int npp_canny_finish(const uint8_t* d_map_chw, int C, int h, int w, uint8_t* d_out_chw, void* stream);
int npp_edge_count(const uint8_t* d_map_chw, int C, int h, int w, const uint8_t* d_eroded_hw, float* d_out_hw, void* stream);
int npp_edt_sq(const uint8_t* d_mask_hw, int H, int W, uint32_t* d_tmp_hw, int32_t* d_dsq_hw, void* stream);
int npp_far_points(const int32_t* d_dsq_hw, int H, int W, int topk, int n_min, void* d_scratch, int32_t* d_record, void* stream);

/* ---- perspective views: warp a uint8 image or mask under a 3 x 3 map (view.py; csrc/npp_view.hip) ------------------------------ */
/* d_src (Hs, Ws, C) uint8 with C in 1..4 -> d_out (Ho, Wo, C) and, unless null, d_inside (Ho, Wo).  m: the row-major map of npp_view
 * as nine doubles; canvas pixel (i, j) reads the source at
 *     d = (m6 i + m7 j) + m8,  y = ((m0 i + m1 j) + m2) / d,  x = ((m3 i + m4 j) + m5) / d
 * in FLOAT64, every product and sum rounded separately (no fma contraction), so NumPy, the host twin and the kernel agree bit for bit.
 * mode 0, nearest: taps iy = floor(y + 0.5), ix = floor(x + 0.5); in the source iff d > 0, y and x finite, 0 <= iy < Hs, 0 <= ix < Ws.
 * mode 1, bilinear: in the source iff d > 0, finite, 0 <= y <= Hs - 1 and 0 <= x <= Ws - 1; y0 = floor(y), y1 = min(y0 + 1, Hs - 1),
 *   fy = y - y0, likewise in x; v = ((1 - fy) ((1 - fx) a00 + fx a01)) + (fy ((1 - fx) a10 + fx a11)) in float64 in that order, and
 *   the result is floor(v + 0.5) clamped to [0, 255].
 * A pixel outside the source: value 0 and inside 0; otherwise inside 255.  Ho Wo and Hs Ws < 2^31.  Bad arguments (null pointers,
 * a non-finite matrix entry, a mode other than 0 or 1): NPP_ERR_ARG and a message, nothing launched.  The _host form is the same
 * definition by plain C++ on host arrays. */
int npp_warp_image_u8(const uint8_t* d_src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, uint8_t* d_out,
                      uint8_t* d_inside, void* stream);
int npp_warp_image_u8_host(const uint8_t* src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, uint8_t* out,
                           uint8_t* inside);
/* The antialiased warp: ss x ss samples per canvas pixel, ss in {1, 2, 4, 8}, reduced in the launch.  Sample s = a ss + b
 * (a, b = 0 .. ss - 1) of canvas pixel (i, j) sits at the canvas position (i + off[a], j + off[b]), off[a] = (2 a + 1) / (2 ss) - 0.5
 * in float64 (the offset and the sum are exact), and goes through the map as above: d, y, x in the written order, every product and
 * sum rounded separately.  Its value v_s (float64) is, in mode 1, the UNROUNDED blend v of above (before floor(v + 0.5)) and, in
 * mode 0, the tapped byte as a double.  A sample COUNTS iff it is in the source by its mode's test above.
 * reduce 0, mean: acc = +0.0; for s = 0 .. ss^2 - 1 in this order acc = acc + v_s for each sample that counts (one rounded add each);
 *   the byte is floor(acc / cnt + 0.5) clamped to [0, 255], cnt the number of samples that count, one IEEE quotient.
 * reduce 1, min: the smallest v_s over the samples that count, then the same floor(. + 0.5) and clamp (for masks: a canvas pixel is
 *   as white as its darkest sample).
 * inside is 255 iff the pixel CENTRE is in the source (the test above at (i, j)) AND at least one sample counts; otherwise every
 * channel is 0 and inside is 0 -- a pixel whose centre is outside stays empty even when some of its samples count.  Two consequences
 * of "a sample that is not in the source does not count": under bilinear the outermost canvas pixels of an identity-like map average
 * only their inward samples, and a source one pixel high (or wide) yields no bilinear sample at ss > 1 (every offset is a fraction,
 * and 0 <= y <= Hs - 1 = 0 admits none).  ss = 1: off = 0 and acc = 0 + v, so either reduce is npp_warp_image_u8 byte for byte.
 * One thread per canvas pixel loops over its samples in order: no atomics, no state between calls, the result does not depend on
 * the launch geometry.  Arguments as above, and ss outside {1, 2, 4, 8} or reduce outside {0, 1}: NPP_ERR_ARG and a message that
 * names the argument, nothing launched.  Not built: other filters (Lanczos, EWA), other ss, a per-pixel adaptive ss, float images. */
int npp_warp_image_u8_ss(const uint8_t* d_src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, int ss, int reduce,
                         uint8_t* d_out, uint8_t* d_inside, void* stream);
int npp_warp_image_u8_ss_host(const uint8_t* src, int Hs, int Ws, int C, int Ho, int Wo, const double m[9], int mode, int ss, int reduce,
                              uint8_t* out, uint8_t* inside);

/* ---- quality report: SSIM and region-wise PSNR / MAE of an image against a ground truth (metrics.py) ------------------------- */
/* Both images are (H, W, 3) fp32 in [0, 1], read as they lie; all arithmetic and every output is float64.  No entry keeps state in
 * device memory between launches and none uses atomics: two calls give identical bits.
 * npp_ssim_map (metrics.ssim_map; train.py --eval_metrics, evaluate.py): the SSIM index of Wang et al. -- 11 x 11 Gaussian window,
 *   sigma 1.5, normalised to sum 1 and applied separably; K1 = 0.01, K2 = 0.03, data range 1; population variances E[xy] - mu_x mu_y --
 *   at every pixel whose whole window lies inside the image, averaged over the three channels: d_map is (H - 10, W - 10), entry
 *   (i, j) belongs to image pixel (i + 5, j + 5).  There it equals what "filter with reflection, crop 5" implementations give.
 *   H, W >= 11, NPP_ERR_ARG (nothing launched) below.
 * npp_region_sums (metrics.report / psnr / mae / ssim): per-block partial sums over an (H, W) fp32 weight mask w, written to
 *   d_part[block][5], block < npp_region_sums_blocks(H, W) (a function of the shape only; at most 256): 0 sum w; 1 sum w |a - b|^2 and
 *   2 sum w |a - b| over the three channels; 3 sum w over the pixels the map covers (rows 5 .. H - 6, columns 5 .. W - 6) and
 *   4 sum w map there.  d_ssim_map may be NULL: 3 and 4 are then 0 and any H, W >= 1 is taken.  The caller adds the blocks in order. */
int npp_ssim_map(const float* d_a_hw3, const float* d_b_hw3, int H, int W, double* d_map, void* stream);
int npp_region_sums_blocks(int H, int W);
int npp_region_sums(const float* d_a_hw3, const float* d_b_hw3, const float* d_weight_hw, const double* d_ssim_map, int H, int W,
                    double* d_part, void* stream);

/* ---- quality report: LPIPS of whole images (metrics.LPIPSMetric; csrc/npp_lpips_map.hip) --------------------------------------- */
/* The head of LPIPS.forward(use_robust = False) on the fp32 features of ONE image pair, in float64 throughout (the fp32 features are
 * exact inputs; every sum has a fixed order; no atomics, nothing kept between launches: two calls give identical bits).
 * npp_lpips_tap_map (externel_lib/lpips/lpips.py:104-119, lpips/__init__.py:42-44 normalize_tensor, the NetLinLayer's 1 x 1
 *   convolution): d_map[p] = sum_c lin[c] (a_c(p) / (|a(p)| + 1e-10) - b_c(p) / (|b(p)| + 1e-10))^2 at the h w positions of a tap of C
 *   channels, two passes over the channels (norms, then differences).  layout: NPP_LPIPS_NCHW -- features (C, h, w); the launcher
 *   takes one lane per position (NPP_LPIPS_NCHW_LANE) from 16384 positions on and splits the channels over the lanes of a wave
 *   (NPP_LPIPS_NCHW_SPLIT) below; either form can be asked for by its own code -- or NPP_LPIPS_NHWC: position-major (h, w, C), one wave
 *   per position.  No transposing copy in either case.
 * npp_lpips_compose (lpips.py:19-23 upsample, :117, :126-128): d_out (H, W) = sum over the n_taps <= 8 maps d_maps[k] (hs[k], ws[k]),
 *   in tap order, of their bilinear resize to (H, W) with align_corners = False (source index max(0, (o + 0.5) h / H - 0.5), the +1
 *   neighbour clamped).  d_maps / hs / ws are HOST arrays (of device pointers / sizes), read before the call returns.  One launch.
 * npp_map_region_sums (the region mean of the distance map; with a tap's map and no weights, lpips.py:15-16 spatial_average): per-block
 *   partial sums (sum w, sum w map) over an (H, W) fp32 weight mask -- NULL: all ones -- written to d_part[block][2], block <
 *   npp_map_region_sums_blocks(H, W) (a function of the shape only; at most 256).  The caller adds the blocks in order.
 * Every launcher checks on the host first -- null pointers, C < 1, empty maps, an unknown layout code: NPP_ERR_ARG, nothing launched. */
#define NPP_LPIPS_NCHW 0
#define NPP_LPIPS_NHWC 1
#define NPP_LPIPS_NCHW_LANE 2
#define NPP_LPIPS_NCHW_SPLIT 3
int npp_lpips_tap_map(const float* d_f0, const float* d_f1, int C, int h, int w, int layout, const float* d_lin, double* d_map,
                      void* stream);
int npp_lpips_compose(const double* const* d_maps, const int* hs, const int* ws, int n_taps, int H, int W, double* d_out, void* stream);
int npp_map_region_sums_blocks(int H, int W);
int npp_map_region_sums(const double* d_map, const float* d_weight_hw, int H, int W, double* d_part, void* stream);

/* ---- host side: the reference's NumPy random stream, GIL-free ----------------------- */
/* numpy.random.RandomState(seed) restated bit for bit for the three draws of an iteration (models/sampler.py:260,324;
 * NPP_completion/train.py:172): MT19937 with init_genrand seeding, uniform() from the 53-bit double, and
 * choice(n, size, replace=False) == permutation(n)[:size] (full Fisher-Yates with the legacy masked-rejection
 * random_interval).  Host memory only, no GPU; one handle per stream, not thread-safe per handle. */
void* npp_rng_create(uint32_t seed);
void npp_rng_destroy(void* rng);
int npp_rng_seed(void* rng, uint32_t seed);
int npp_rng_get_state(void* rng, uint32_t* key624, int32_t* pos);      /* == RandomState.get_state()[1:3] */
int npp_rng_set_state(void* rng, const uint32_t* key624, int32_t pos);
double npp_rng_uniform(void* rng, double lo, double hi);
int npp_rng_choice_noreplace(void* rng, int64_t n, int64_t size, int64_t* scratch_n, int64_t* out_size);

/* ---- GridPatchSampler's host-side draw (models/sampler.py:242-354: patch source :324-331, fake centres :260, lattice
 * candidates + unknown-pixel filter + k nearest :148-214) in one GIL-free host call, consuming `rng` like the reference
 * consumes np.random.  sat: (H+1) x (W+1) summed-area table of the known mask; pools: (row, col) int32 pairs in the
 * reference's np.nonzero order; shifts_dydx: the two lattice shifts as (dy, dx) (sampler.py:35). */
void* npp_sampler_create(const int64_t* sat, int H, int W, const int32_t* pool_train, int64_t n_train,
                         const int32_t* pool_val, int64_t n_val, const double* shifts_dydx);
void npp_sampler_destroy(void* sampler);
int npp_sampler_set_patch(void* sampler, int patch_size, int n_samples, int64_t* pool_train_n, int64_t* pool_val_n);
int npp_sampler_draw(void* sampler, void* rng, int topk, double invalid_ratio, int32_t* source, int32_t* k,
                     int32_t* cen_n2, double* real_cen_ntopk2, float* weights_ntopk);

/* ---- rng_mode="device": the sampler's decisions drawn on the GPU -------------------------------------------------------
 * The same decisions as npp_sampler_draw (models/sampler.py:242-354) plus the N_rand pixel rows of
 * NPP_completion/train.py:172, drawn from Philox4x32-10 keyed by the fit's seed instead of np.random's stream: a draw is a
 * pure function of (seed, draw index t, inputs), for M images in one launch, with no state in device memory.
 *   patch source      word 0 of counter (0, 0, t, 0) times 2^-32, through the comparisons of sampler.py:324-331
 *   n of N, no repeat positions 0..n-1 of a keyed permutation of [0, N): a cycle-walking balanced Feistel network, eight
 *                     rounds F = word 0 of counter (R, round, t, stream); stream 1 = the n_p fake-patch centres (from the
 *                     bounds-filtered pool), stream 2 = the pixel rows (from i_train)
 *   lattice half      GridPatchSampler.draw(): 400 candidates, bounds test, unknown count from the summed-area table,
 *                     zero distance -> 10000, k = min over patches of min(count - 1, topk), stable order by distance then
 *                     candidate index, weights inv / sum(inv) in float64 rounded to float
 * npp_dev_image: the per-image constants (built once per patch size); every pointer is device memory for the launches and
 * host memory for the *_host twins, which run the same arithmetic (csrc/npp_dev_sampler.h) on the CPU. */
#define NPP_DEV_SRC_VAL 0
#define NPP_DEV_SRC_TRAIN 1
#define NPP_DEV_SRC_SAME 2
#define NPP_DEV_MAX_IMAGES 64      /* images per launch: the draw indices ride in the kernel arguments */
typedef struct npp_dev_image {
  const int32_t* sat;              /* (H+1) x (W+1) summed-area table of the known mask */
  const int32_t* pool_val;         /* bounds-filtered pools, (row, col) pairs (GridPatchSampler.pool_val / pool_train) */
  const int32_t* pool_train;
  int64_t n_pool_val, n_pool_train;
  int64_t n_train;                 /* population of the pixel draw (rows of i_train) */
  double shifts[4];                /* the two lattice shifts as (dy, dx), (dy, dx) (sampler.py:35) */
  double invalid_ratio;
  uint32_t seed_lo, seed_hi;       /* Philox key = (seed & 0xffffffff, seed >> 32) */
  int32_t H, W, P, pad;            /* P = 2 * (patch_size / 2) */
} npp_dev_image;

/* int32 words of one image's record: [0] source, [1] k (0 = no valid real patch: the iteration is skipped; -1 = the drawn
 * pool holds fewer than n_p pixels), [2] n_p, [3] t, then the (row, col) centres of the n_p fake patches followed by the n_p k
 * real ones -- what npp_patch_gather / npp_batch_assemble take -- and from word 4 + 2 n_p (1 + topk) the n_p k float weights
 * (n_p ones on 'same' draws, sampler.py:338). */
int64_t npp_dev_sampler_record_words(int n_p, int topk);
/* The decision launch: one workgroup per image, one wave per fake patch in turn (400 candidates, four table look-ups each,
 * wave-level stable selection), the minimum over the patches and the compact record behind a barrier.  h_t: M draw indices in
 * HOST memory (passed by value).  d_rec (M, rec_stride) int32, rec_stride >= npp_dev_sampler_record_words(). */
int npp_dev_sampler_decide(const npp_dev_image* d_imgs, int M, const uint32_t* h_t, int n_p, int topk, int32_t* d_rec,
                           int64_t rec_stride, void* stream);
int npp_dev_sampler_decide_host(const npp_dev_image* imgs, int M, const uint32_t* t, int n_p, int topk, int32_t* rec,
                                int64_t rec_stride);
/* The pixel-row launch: d_pix[m * pix_stride + j] = position j of image m's stream-2 permutation of [0, n_train), the int64
 * indices npp_batch_assemble reads, in sample order.  n_pix <= n_train of every image. */
int npp_dev_sampler_pixels(const npp_dev_image* d_imgs, int M, const uint32_t* h_t, int64_t n_pix, int64_t* d_pix,
                           int64_t pix_stride, void* stream);
int npp_dev_sampler_pixels_host(const npp_dev_image* imgs, int M, const uint32_t* t, int64_t n_pix, int64_t* pix,
                                int64_t pix_stride);
/* The generator and the permutation on their own (host): out[4] = Philox4x32-10(ctr, key); out[j] = position j, j < n. */
int npp_dev_philox4x32_10(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4);
int npp_dev_perm_host(uint64_t seed, uint32_t t, uint32_t stream, int64_t N, int64_t n, int64_t* out);

/* ---- diagnostics ---------------------------------------------------------- */
/* Checks the MFMA operand / accumulator lane maps this library relies on (incl. the
 * accumulator-as-next-operand chain) with exact integer data.  d_scratch >= 1 MiB. */
int npp_selftest_mfma(void* d_scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NPP_HIP_H */
