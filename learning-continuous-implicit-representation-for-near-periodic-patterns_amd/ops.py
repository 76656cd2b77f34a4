"""Thin torch-tensor wrappers over the C ABI (include/npp_hip.h).  torch is used for device
memory and streams only; every call goes to libnpp_hip.so on the current HIP stream."""
import ctypes as C
import math

import numpy as np
import torch

from . import audit
from ._lib import lib, check, EmbedCfg, param_layout, NPP_ROW_TILE, NPP_E, NPP_WIDTH  # noqa: F401


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def tune(key, value=-1):
    """npp_tune: choose between kernel forms that compute the same result ("conv_wink", "conv_win", "conv_wstat", "conv_pair", "light_det")
    or the training stash's format ("stash8": 1 = 8-bit stash + fp8 weight-gradient MFMA (default), 0 = the 16-bit stash);
    value < 0 only reads.  -> the previous value.  Both fused-width libraries are set (the trunk kernels live in the first)."""
    from ._lib import FUSED_WIDTHS
    old = None
    for w in FUSED_WIDTHS:
        try:
            r = lib(w).npp_tune(key.encode(), int(value))
        except OSError:
            continue
        check(r, "npp_tune", w)
        old = r if old is None else old
    return old


def _stream():
    """hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream object per
    call (5-8 us, x ~45 kernel calls per iteration: it was most of the host enqueue time); the raw accessor is ~0.3 us."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def select_device(device):
    """The torch.device a fit / net / ranker lives on, made the CURRENT device of this host thread.  Every entry point of the
    C ABI launches on a stream of the current device (one process -- or at least one host thread -- per GPU);
    objects built for another GPU must therefore select it before they allocate or launch."""
    dev = torch.device(device)
    if dev.type == "cuda":
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(dev)
    return dev


def check_current(device):
    """Raise (instead of enqueueing GPU-x kernels on GPU-y's stream) when `device` is not the thread's current device."""
    if device.type == "cuda" and device.index != torch.cuda.current_device():
        raise RuntimeError(f"npp_amd: object lives on {device} but the current device is cuda:{torch.cuda.current_device()}; "
                           f"call torch.cuda.set_device({device.index}) in this thread (one process / host thread per GPU)")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _req(t, dtype, name, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"{name}: expected a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


class _PinnedRing:
    """Persistent pinned staging buffers for small host -> device transfers (sampler indices, patch centres).
    A pageable .to(device) is a synchronous copy queued behind everything already in the stream, i.e. a device sync
    per call: it serialised the host-side sampler with the previous iteration's kernels (+0.5 ms per iteration);
    tensor.pin_memory() registers fresh host memory on every call (3.4 ms each, measured).  Here: per size class a ring
    of pinned blocks allocated once, each guarded by the event recorded after its last copy."""

    def __init__(self, slots=8):
        import threading
        self.slots, self.rings = slots, {}
        self.lock = threading.Lock()          # (several host threads transfer: the images of a rank searched side by side, run.py)

    def __call__(self, a, device):
        a = np.ascontiguousarray(a)
        if device.type != "cuda":
            return torch.from_numpy(a).to(device)
        with self.lock:
            return self._copy(a, device)

    def _copy(self, a, device):
        cap = 1 << max(12, int(a.nbytes - 1).bit_length())
        ring = self.rings.get((device, cap))
        if ring is None:
            ring = self.rings[(device, cap)] = {"buf": [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(self.slots)],
                                                "ev": [None] * self.slots, "i": 0}
        i = ring["i"]
        ring["i"] = (i + 1) % self.slots
        if ring["ev"][i] is not None:
            ring["ev"][i].synchronize()                       # long complete unless the host ran > slots transfers ahead
        stage = ring["buf"][i][:a.nbytes]
        stage.numpy()[:] = a.reshape(-1).view(np.uint8)
        out = stage.to(device, non_blocking=True).view(torch.from_numpy(a[:0]).dtype).reshape(a.shape)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        ring["ev"][i] = ev
        return out


_pinned_ring = _PinnedRing()
# Sections that save / reseed / restore the PROCESS-WIDE torch generator (the reference's torch.manual_seed(0) before every candidate,
# search.py:92; fixed-seed stand-in trunks) hold this lock: images searched on several host threads would otherwise read each other's
# generator state.
RNG_LOCK = __import__("threading").RLock()


def h2d(a, device):
    """NumPy array -> device tensor through a persistent pinned staging ring, non-blocking (see _PinnedRing)."""
    return _pinned_ring(a, device)


PIXEL_LOSS_SCRATCH = 1024 * 8 + 8       # NPP_PIXEL_LOSS_SCRATCH_FLOATS (include/npp_hip.h)
# False: the float-atomic reductions of the pixel loss and the LPIPS head (arrival order; the A/B comparator of the fixed-order forms)
DETERMINISTIC = True


def pad_rows(n):
    return (n + NPP_ROW_TILE - 1) // NPP_ROW_TILE * NPP_ROW_TILE


def selftest(device="cuda"):
    scratch = torch.empty(1 << 18, dtype=torch.float32, device=device)
    check(lib().npp_selftest_mfma(_p(scratch), _stream()), "npp_selftest_mfma")


def _coord_sym(coords, sym):
    """The entry point of `sym` for a coordinate tensor: int32 pixel indices, or float32 positions [row y, col x] of the fit's pixel
    frame (any real value: sub-pixel, negative, past the border) through its _coordf form."""
    if isinstance(coords, torch.Tensor) and coords.dtype == torch.float32:
        _req(coords, torch.float32, "coords")
        return sym + "_coordf"
    _req(coords, torch.int32, "coords")
    return sym


def embed_fwd(coords, cfg, out_dtype=torch.float32, precise=True):
    """coords (N,2) int32 (row, col) or float32 positions -> (N, K*462); replaces Embedder_periodic.embed +
    Embedder.embed + cat (models/embedder.py:140-148, :51-56; train.py:93-105)."""
    sym = _coord_sym(coords, "npp_embed_fwd")
    n = coords.shape[0]
    out = torch.empty((n, cfg.K * NPP_E), dtype=out_dtype, device=coords.device)
    code = {torch.float32: 0, torch.bfloat16: 1}[out_dtype]
    check(getattr(lib(), sym)(_p(coords), n, C.byref(cfg), _p(out), code, int(bool(precise)), _stream()), sym)
    return out


def warp_fwd(coords, cfg):
    """(N,2) int32 or float32 -> (N, K*22) fp32: the Embedder_periodic stage alone (embedder.py:140-148), the same precise
    arithmetic for both."""
    sym = _coord_sym(coords, "npp_warp_fwd")
    n = coords.shape[0]
    out = torch.empty((n, cfg.K * 22), dtype=torch.float32, device=coords.device)
    check(getattr(lib(), sym)(_p(coords), n, C.byref(cfg), _p(out), _stream()), sym)
    return out


def pack_bytes(K, which, width=NPP_WIDTH):
    n = lib(width).npp_pack_bytes(K, width, which)
    check(n, "npp_pack_bytes", width)
    return int(n)


def pack_weights(params, K, wf=None, wb=None, width=NPP_WIDTH):
    _req(params, torch.float32, "params")
    if wf is None:
        wf = torch.empty(pack_bytes(K, 0, width), dtype=torch.uint8, device=params.device)
    if wb is None:
        wb = torch.empty(pack_bytes(K, 1, width), dtype=torch.uint8, device=params.device)
    check(lib(width).npp_pack_weights(_p(params), _p(wf), _p(wb), K, width, _stream()), "npp_pack_weights", width)
    return wf, wb


def train_workspace(K, Bp, ksplit, width=NPP_WIDTH):
    sizes = (C.c_int64 * 4)()
    check(lib(width).npp_train_workspace(K, width, Bp, ksplit, sizes), "npp_train_workspace", width)
    return [int(s) for s in sizes]


def mlp_fwd(coords, cfg, wf, params, pred=None, actF=None, width=NPP_WIDTH, out_act=1):
    """Fused embedder + MLP + sigmoid: coords (Bp,2) -> pred (Bp,3).  Replaces the table
    gather + render() (train.py:166-189; helpers.py:41-62; networks.py:56-95).  out_act: 1 sigmoid, 2 tanh (--normalize_type 2), 0 raw."""
    _req(coords, torch.int32, "coords")
    bp = coords.shape[0]
    if pred is None:
        pred = torch.empty((bp, 3), dtype=torch.float32, device=coords.device)
    if out_act != 1:
        check(lib(width).npp_mlp_fwd_act(_p(coords), bp, C.byref(cfg), width, _p(wf), _p(params), _p(pred), _p(actF), int(out_act), _stream()),
              "npp_mlp_fwd_act", width)
        return pred
    check(lib(width).npp_mlp_fwd(_p(coords), bp, C.byref(cfg), width, _p(wf), _p(params), _p(pred), _p(actF), _stream()),
          "npp_mlp_fwd", width)
    return pred


def mlp_fwd_emb(emb, K, wf, params, out=None, actF=None, out_act=0, width=NPP_WIDTH):
    """NPP_Net.forward(None, x_periodic) on a materialised (Bp, K*462) embedding (networks.py:56-95);
    out_act: 0 raw network output, 1 sigmoid, 2 tanh (render, helpers.py:55-60)."""
    _req(emb, torch.float32, "emb")
    bp = emb.shape[0]
    if out is None:
        out = torch.empty((bp, 3), dtype=torch.float32, device=emb.device)
    check(lib(width).npp_mlp_fwd_emb(_p(emb), emb.stride(0), bp, K, width, _p(wf), _p(params), _p(out), _p(actF), out_act,
                                _stream()), "npp_mlp_fwd_emb", width)
    return out


def mlp_bwd_act(dout, out, K, wb, params, actF, dzF, out_act, width=NPP_WIDTH):
    _req(dout, torch.float32, "dout")
    _req(out, torch.float32, "out", dout.shape)
    check(lib(width).npp_mlp_bwd_act(_p(dout), _p(out), dout.shape[0], K, width, _p(wb), _p(params), _p(actF), _p(dzF),
                                out_act, _stream()), "npp_mlp_bwd_act", width)


def grad_reduce(gslabs, n_slabs, n, grad, accumulate=False):
    """grad (+)= sum of the split-K slabs (the blob-shaped .grad a torch optimiser consumes)."""
    check(lib().npp_grad_reduce(_p(gslabs), n_slabs, gslabs.numel() // n_slabs, n, _p(grad), int(bool(accumulate)), _stream()),
          "npp_grad_reduce")


def fourier_fwd(x, freqs, include_input=True):
    """Embedder.embed (models/embedder.py:11-56): (N,d) -> (N, d*(2*len(freqs)+include_input))."""
    _req(x, torch.float32, "x")
    n, d = x.shape
    f = (C.c_float * len(freqs))(*[float(v) for v in freqs])
    out = torch.empty((n, d * (2 * len(freqs) + int(bool(include_input)))), dtype=torch.float32, device=x.device)
    check(lib().npp_fourier_fwd(_p(x), n, d, f, len(freqs), int(bool(include_input)), _p(out), _stream()), "npp_fourier_fwd")
    return out


def mlp_bwd(dpred, pred, K, wb, params, actF, dzF, width=NPP_WIDTH, out_act=1):
    _req(dpred, torch.float32, "dpred")
    _req(pred, torch.float32, "pred", dpred.shape)
    if out_act != 1:
        return mlp_bwd_act(dpred, pred, K, wb, params, actF, dzF, out_act, width)
    check(lib(width).npp_mlp_bwd(_p(dpred), _p(pred), dpred.shape[0], K, width, _p(wb), _p(params), _p(actF), _p(dzF),
                            _stream()), "npp_mlp_bwd", width)


def mlp_bwd_patch(dpred, pred, K, wb, params, actF, dzF, dx_a, dx_b, fmask, rmask, row0, n_p, k, P, comp, width=NPP_WIDTH, out_act=1):
    """mlp_bwd with the patch rows' dL/dpred formed in the launch (patch_compose_bwd folded in; rows [row0, row0 + n_p P^2) of
    dpred are written)."""
    from ._lib import PatchGrad
    _req(dpred, torch.float32, "dpred")
    _req(pred, torch.float32, "pred", dpred.shape)
    for nm, t in (("dx_a", dx_a), ("dx_b", dx_b)):                  # the leading n_p k images are read (a [x | y] batch gradient is fine)
        if t is not None:
            _req(t, torch.float32, nm)
            if t.dim() != 4 or t.shape[0] < n_p * k or tuple(t.shape[1:]) != (3, P, P):
                raise ValueError(f"{nm}: expected (>= {n_p * k}, 3, {P}, {P}), got {tuple(t.shape)}")
    _req(fmask, torch.float32, "fmask")
    _req(rmask, torch.float32, "rmask")
    if fmask.numel() != n_p * P * P or rmask.numel() != n_p * k * P * P:
        raise ValueError("fmask / rmask: expected (n_p,1,P,P) / (n_p k,1,P,P)")
    pg = PatchGrad(dx_a.data_ptr(), dx_b.data_ptr() if dx_b is not None else None, fmask.data_ptr(), rmask.data_ptr(), int(row0),
                   int(n_p), int(k), int(P), int(bool(comp)))
    if out_act != 1:
        check(lib(width).npp_mlp_bwd_patch_act(_p(dpred), _p(pred), dpred.shape[0], K, width, _p(wb), _p(params), _p(actF), _p(dzF),
                                               C.byref(pg), int(out_act), _stream()), "npp_mlp_bwd_patch_act", width)
        return
    check(lib(width).npp_mlp_bwd_patch(_p(dpred), _p(pred), dpred.shape[0], K, width, _p(wb), _p(params), _p(actF), _p(dzF),
                                       C.byref(pg), _stream()), "npp_mlp_bwd_patch", width)


def auto_ksplit(K, device, width=NPP_WIDTH):
    """Split-K factor that makes the grouped weight-gradient launch (tiles x ksplit workgroups, one per CU) fill the
    chip in exactly one round."""
    tiles = check(lib(width).npp_mlp_wgrad_tiles(K), "npp_mlp_wgrad_tiles", width)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(64, cus // tiles))


def pack_weights32(params, K, w32=None, width=NPP_WIDTH):
    """fp32 blob -> the fp32 A-operand pack of npp_mlp_fwd32."""
    n = int(lib(width).npp_pack32_bytes(K, width))
    if w32 is None:
        w32 = torch.empty(n, dtype=torch.uint8, device=params.device)
    check(lib(width).npp_pack_weights32(_p(params), _p(w32), K, width, _stream()), "npp_pack_weights32", width)
    return w32


def mlp_fwd32(coords_yx, cfg, w32, params, out=None, out_act=1, width=NPP_WIDTH):
    """Exact-fp32 fused embedder + MLP forward (render), coords (Bp,2) int32 with Bp % 64 == 0 -> (Bp,3)."""
    _req(coords_yx, torch.int32, "coords")
    return render(coords_yx, cfg, w32, params, "fp32", out=out, out_act=out_act, width=width)


# ---- exact-fp32 training chain (include/npp_hip.h "exact-fp32 training of the fused MLP") ------------------------------------
def train_workspace32(K, Bp, ksplit, width=NPP_WIDTH):
    """Byte sizes [0, fp32 stash, fp32 pre-activation gradients, gradient slabs] of the exact-fp32 fit for Bp padded rows."""
    sizes = (C.c_int64 * 4)()
    check(lib(width).npp_train_workspace32(K, width, Bp, ksplit, sizes), "npp_train_workspace32", width)
    return [int(s) for s in sizes]


def pack_weights32_bwd(params, K, w32b=None, width=NPP_WIDTH):
    """fp32 blob -> the transposed fp32 pack of npp_mlp_bwd32."""
    _req(params, torch.float32, "params")
    n = int(check(lib(width).npp_pack32_bwd_bytes(K, width), "npp_pack32_bwd_bytes", width))
    if w32b is None:
        w32b = torch.empty(n, dtype=torch.uint8, device=params.device)
    check(lib(width).npp_pack_weights32_bwd(_p(params), _p(w32b), K, width, _stream()), "npp_pack_weights32_bwd", width)
    return w32b


def mlp_fwd32_train(coords_yx, cfg, w32, params, pred, stash, out_act=1, width=NPP_WIDTH):
    """mlp_fwd32 (bit for bit) that also writes the fp32 training stash; coords (Bp,2) int32, Bp % 64 == 0."""
    _req(coords_yx, torch.int32, "coords")
    _req(pred, torch.float32, "pred", (coords_yx.shape[0], 3))
    check(lib(width).npp_mlp_fwd32_train(_p(coords_yx), coords_yx.shape[0], C.byref(cfg), width, _p(w32), _p(params), _p(pred),
                                         _p(stash), int(out_act), _stream()), "npp_mlp_fwd32_train", width)
    return pred


def mlp_bwd32(dpred, pred, K, w32b, params, stash, dz, width=NPP_WIDTH, out_act=1):
    """loss.backward() through the MLP in exact fp32: dpred (Bp,3) (rows beyond the batch 0) -> the pre-activation gradients dz."""
    _req(dpred, torch.float32, "dpred")
    _req(pred, torch.float32, "pred", dpred.shape)
    check(lib(width).npp_mlp_bwd32(_p(dpred), _p(pred), dpred.shape[0], K, width, _p(w32b), _p(params), _p(stash), _p(dz),
                                   int(out_act), _stream()), "npp_mlp_bwd32", width)


def mlp_wgrad32(dz, stash, cfg, Bp, K, ksplit, gslabs, width=NPP_WIDTH):
    """Weight / bias gradients of mlp_bwd32 into ksplit slabs (every slab written in full, fixed row-tile assignment, no atomics)."""
    _req(gslabs, torch.float32, "gslabs")
    check(lib(width).npp_mlp_wgrad32(_p(dz), _p(stash), C.byref(cfg), Bp, K, width, ksplit, _p(gslabs), _stream()),
          "npp_mlp_wgrad32", width)


def grid_arg(start, n, canvas_width, origin=(0.0, 0.0), scale=(1.0, 1.0)):
    """npp_grid: canvas pixels [start, start + n) of a canvas `canvas_width` wide, pixel (i, j) at (y0 + i / sy, x0 + j / sx)."""
    from ._lib import Grid
    return Grid(int(start), int(n), int(canvas_width), float(origin[0]), float(origin[1]), float(scale[0]), float(scale[1]))


def view_arg(start, n, canvas_width, M):
    """npp_view: canvas pixels [start, start + n) of a canvas `canvas_width` wide under the row-major 3 x 3 map M (nine numbers,
    stored as float32): pixel (i, j) at ((m0 i + m1 j) + m2, (m3 i + m4 j) + m5) / ((m6 i + m7 j) + m8)."""
    from ._lib import View
    m = np.asarray(M, dtype=np.float32).reshape(-1)
    if m.size != 9:
        raise ValueError(f"M: expected a 3 x 3 matrix, got {np.shape(M)}")
    return View(int(start), int(n), int(canvas_width), (C.c_float * 9)(*[float(v) for v in m]))


def _grid_out(out, n, device):
    if out is None:
        return torch.empty((n, 3), dtype=torch.float32, device=device)
    _req(out, torch.float32, "out")
    if out.dim() != 2 or out.shape[1] != 3 or out.shape[0] < n:
        raise ValueError(f"out: expected at least ({n}, 3), got {tuple(out.shape)}")
    return out


def _view_inside(inside, n):
    if inside is not None:
        _req(inside, torch.uint8, "inside")
        if inside.dim() != 1 or inside.shape[0] < n:
            raise ValueError(f"inside: expected at least ({n},), got {tuple(inside.shape)}")
    return inside


# The inference entry point of every (kind of coordinate source, precision), called on the library L: the one table of render()
_RENDER = {("int32", "bf16"): lambda L, *a: L.npp_mlp_fwd_act(*a), ("int32", "fp32"): lambda L, *a: L.npp_mlp_fwd32(*a),
           ("float32", "bf16"): lambda L, *a: L.npp_mlp_fwd_coordf(*a), ("float32", "fp32"): lambda L, *a: L.npp_mlp_fwd32_coordf(*a),
           ("grid", "bf16"): lambda L, *a: L.npp_mlp_fwd_grid(*a), ("grid", "fp32"): lambda L, *a: L.npp_mlp_fwd32_grid(*a),
           ("view", "bf16"): lambda L, *a: L.npp_mlp_fwd_view(*a), ("view", "fp32"): lambda L, *a: L.npp_mlp_fwd32_view(*a),
           ("grid_ss", "bf16"): lambda L, *a: L.npp_mlp_fwd_grid_ss(*a), ("grid_ss", "fp32"): lambda L, *a: L.npp_mlp_fwd32_grid_ss(*a),
           ("view_ss", "bf16"): lambda L, *a: L.npp_mlp_fwd_view_ss(*a), ("view_ss", "fp32"): lambda L, *a: L.npp_mlp_fwd32_view_ss(*a),
           ("view_list", "bf16"): lambda L, *a: L.npp_mlp_fwd_view_list(*a), ("view_list", "fp32"): lambda L, *a: L.npp_mlp_fwd32_view_list(*a)}
SUPERSAMPLES = (1, 2, 4, 8)     # samples per canvas pixel and direction of a supersampled launch (include/npp_hip.h)


def check_supersample(supersample):
    """supersample as an int; ValueError (by name) unless it is one of SUPERSAMPLES."""
    if isinstance(supersample, bool) or not isinstance(supersample, (int, np.integer)) or int(supersample) not in SUPERSAMPLES:
        raise ValueError(f"supersample {supersample!r}: must be one of {SUPERSAMPLES} samples per canvas pixel in each direction")
    return int(supersample)


def render(src, cfg, pack, params, precision="bf16", out=None, inside=None, out_act=1, width=NPP_WIDTH, supersample=1, pixels=None):
    """The fused embedder + MLP render (no stash) of one coordinate source -> out (rows, 3) float32.  src: an int32 (Bp, 2) tensor of
    pixel indices or a float32 (Bp, 2) tensor of positions [y, x], Bp % 64 == 0 (out: (Bp, 3)); a grid_arg(...) or a view_arg(...):
    src.n canvas pixels -> out[:src.n], no coordinate buffer and no padding (out: at least (n, 3)).  precision: 'bf16' (the fused
    chain; pack = the wf pack) or 'fp32' (the exact chain; pack = the w32 pack).  inside (uint8, a view only, optional) receives
    the bytes 0 not in view (the row is zero) / 1 in view / 3 also inside the fit's image rectangle.  out_act: 1 sigmoid, 2 tanh, 0 raw.
    supersample (a grid or a view only): S in SUPERSAMPLES; every pixel is the ordered mean of S x S samples, formed inside the one
    launch of n S^2 chain rows (include/npp_hip.h "supersampled launches"); 1 is the point-sampled launch.
    pixels (a view only): an int64 tensor of absolute row-major canvas pixel indices; only those pixels of the window are computed
    and stored, each with the bits of the supersample = S launch, and no other word of out / inside changes (include/npp_hip.h
    "listed launches": len(pixels) S^2 chain rows; an index outside the window stores nothing)."""
    from ._lib import Grid, View
    ss = check_supersample(supersample)
    if precision not in ("bf16", "fp32"):
        raise ValueError(f"precision {precision!r}: 'bf16' (fused chain) or 'fp32' (exact chain)")
    canvas = isinstance(src, (Grid, View))
    if inside is not None and not isinstance(src, View):
        raise ValueError("inside: only a view launch writes inside bytes")
    if ss != 1 and not canvas:
        raise ValueError(f"supersample={ss}: only a grid_arg(...) or a view_arg(...) is supersampled, not a tensor of positions "
                         "(place the samples yourself)")
    if pixels is not None and not isinstance(src, View):
        raise ValueError("pixels: only a view_arg(...) launch takes a pixel list, not a grid or a tensor of positions")
    if canvas:
        kind = "view" if isinstance(src, View) else "grid"
        out = _grid_out(out, src.n, params.device)
        head = (C.byref(src), C.byref(cfg), width, _p(pack), _p(params), _p(out))
        if pixels is not None:
            _req(pixels, torch.int64, "pixels")
            if pixels.dim() != 1:
                raise ValueError(f"pixels: expected a 1-d tensor of canvas pixel indices, got {tuple(pixels.shape)}")
            kind, head = "view_list", (head[0], ss, _p(pixels), int(pixels.shape[0])) + head[1:]
        elif ss != 1:
            kind, head = kind + "_ss", (head[0], ss) + head[1:]
        tail = (_p(_view_inside(inside, src.n)),) if kind in ("view", "view_ss", "view_list") else ()
    else:
        if not (isinstance(src, torch.Tensor) and src.dtype in (torch.int32, torch.float32)):
            raise TypeError("src: expected an int32 or float32 (Bp, 2) tensor, a grid_arg(...) or a view_arg(...)")
        kind = "int32" if src.dtype == torch.int32 else "float32"
        _req(src, src.dtype, "coords")
        bp = src.shape[0]
        if out is None:
            out = torch.empty((bp, 3), dtype=torch.float32, device=src.device)
        head = (_p(src), bp, C.byref(cfg), width, _p(pack), _p(params), _p(out))
        tail = (None,) if (kind, precision) == ("int32", "bf16") else ()       # npp_mlp_fwd_act's stash: none
    check(_RENDER[kind, precision](lib(width), *head, *tail, int(out_act), _stream()), f"render({kind}, {precision})", width)
    return out


def view_coords_host(view, res):
    """npp_view_coords_host: the fp32 positions (n, 2) [y, x] and inside bytes (n,) a view launch forms, by plain C++ on the host;
    res = (H, W) of the fit."""
    yx = np.zeros((view.n, 2), np.float32)
    inside = np.zeros(view.n, np.uint8)
    check(lib().npp_view_coords_host(C.byref(view), int(res[0]), int(res[1]), C.c_void_p(yx.ctypes.data), C.c_void_p(inside.ctypes.data)),
          "npp_view_coords_host")
    return yx, inside


def view_ss_classes(view, res, cls=None, inside=None):
    """npp_view_ss_classes: the supersampling class (0 not in view, else 1, 2, 4 or 8 samples per direction) of each of the view's
    n canvas pixels, one launch -> cls (uint8, at least (n,); made on the current device when neither tensor is given); inside (uint8, optional) receives the point launch's inside bytes for a
    fit of res = (H, W).  The rule is exact (include/npp_hip.h "adaptive supersampling"): the host twin gives the same bytes."""
    if cls is None:
        cls = torch.empty(view.n, dtype=torch.uint8, device=inside.device if inside is not None else torch.device("cuda", torch.cuda.current_device()))
    _view_inside(cls, view.n)
    check(lib().npp_view_ss_classes(C.byref(view), int(res[0]), int(res[1]), _p(cls), _p(_view_inside(inside, view.n)), _stream()),
          "npp_view_ss_classes")
    return cls


def view_ss_classes_host(view, res):
    """npp_view_ss_classes_host: (classes (n,), inside bytes (n,)) of view_ss_classes as NumPy arrays, by plain C++ on the host."""
    cls = np.zeros(view.n, np.uint8)
    inside = np.zeros(view.n, np.uint8)
    check(lib().npp_view_ss_classes_host(C.byref(view), int(res[0]), int(res[1]), C.c_void_p(cls.ctypes.data),
                                         C.c_void_p(inside.ctypes.data)), "npp_view_ss_classes_host")
    return cls, inside


def grid_samples_host(grid, supersample):
    """npp_grid_samples_host: the (n S^2, 2) fp32 sample positions [y, x] of a supersampled grid launch in chain-row order, by plain
    C++ on the host."""
    ss = check_supersample(supersample)
    yx = np.zeros((grid.n * ss * ss, 2), np.float32)
    check(lib().npp_grid_samples_host(C.byref(grid), ss, C.c_void_p(yx.ctypes.data)), "npp_grid_samples_host")
    return yx


def view_samples_host(view, supersample, res):
    """npp_view_samples_host: the (n S^2, 2) fp32 sample positions of a supersampled view launch, which of them are in view
    (n S^2,) and the per-pixel inside bytes (n,) it writes, by plain C++ on the host; res = (H, W) of the fit."""
    ss = check_supersample(supersample)
    yx = np.zeros((view.n * ss * ss, 2), np.float32)
    counts = np.zeros(view.n * ss * ss, np.uint8)
    inside = np.zeros(view.n, np.uint8)
    check(lib().npp_view_samples_host(C.byref(view), ss, int(res[0]), int(res[1]), C.c_void_p(yx.ctypes.data),
                                      C.c_void_p(counts.ctypes.data), C.c_void_p(inside.ctypes.data)), "npp_view_samples_host")
    return yx, counts, inside


WARP_REDUCES = ("mean", "min")      # how the antialiased warp reduces a pixel's samples (include/npp_hip.h npp_warp_image_u8_ss)


def check_warp(mode, supersample=1, reduce="mean"):
    """(mode code, ss, reduce code) of a warp; ValueError by the argument's name for a value the library does not take."""
    if mode not in ("nearest", "bilinear"):
        raise ValueError(f"mode {mode!r}: 'nearest' or 'bilinear'")
    ss = check_supersample(supersample)
    if reduce not in WARP_REDUCES:
        raise ValueError(f"reduce {reduce!r}: one of {WARP_REDUCES}")
    return int(mode == "bilinear"), ss, WARP_REDUCES.index(reduce)


def _warp_args(M, size, mode, supersample, reduce):
    m = np.asarray(M, dtype=np.float64).reshape(-1)
    if m.size != 9:
        raise ValueError(f"M: expected a 3 x 3 matrix, got {np.shape(M)}")
    md, ss, rd = check_warp(mode, supersample, reduce)
    Ho, Wo = (int(s) for s in size)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"size {tuple(size)}: both sides must be >= 1")
    return (C.c_double * 9)(*[float(v) for v in m]), Ho, Wo, md, ss, rd


def warp_image_u8(img_u8, M, size, mode="bilinear", supersample=1, reduce="mean"):
    """(Hs, Ws) or (Hs, Ws, C <= 4) uint8 on the device -> the size = (Ho, Wo) canvas under the map M (canvas pixel -> source
    position, float64) and its (Ho, Wo) coverage mask (255 inside the source): include/npp_hip.h npp_warp_image_u8.  supersample = S
    in SUPERSAMPLES, reduce 'mean' or 'min': S x S samples per canvas pixel, reduced in the launch (npp_warp_image_u8_ss); the
    defaults are the point launch."""
    _req(img_u8, torch.uint8, "img_u8")
    if img_u8.dim() not in (2, 3) or img_u8.numel() == 0:
        raise ValueError("img_u8: expected a non-empty (H, W) or (H, W, C)")
    m, Ho, Wo, md, ss, rd = _warp_args(M, size, mode, supersample, reduce)
    Cn = 1 if img_u8.dim() == 2 else img_u8.shape[2]
    out = torch.empty((Ho, Wo) + tuple(img_u8.shape[2:]), dtype=torch.uint8, device=img_u8.device)
    inside = torch.empty((Ho, Wo), dtype=torch.uint8, device=img_u8.device)
    if (ss, rd) == (1, 0):
        check(lib().npp_warp_image_u8(_p(img_u8), img_u8.shape[0], img_u8.shape[1], Cn, Ho, Wo, m, md, _p(out), _p(inside), _stream()),
              "npp_warp_image_u8")
    else:
        check(lib().npp_warp_image_u8_ss(_p(img_u8), img_u8.shape[0], img_u8.shape[1], Cn, Ho, Wo, m, md, ss, rd, _p(out), _p(inside),
                                         _stream()), "npp_warp_image_u8_ss")
    return out, inside


def warp_image_u8_host(img_u8, M, size, mode="bilinear", supersample=1, reduce="mean"):
    """warp_image_u8 on a NumPy array, by the library's host twin."""
    img = np.ascontiguousarray(img_u8, np.uint8)
    if img.ndim not in (2, 3) or img.size == 0:
        raise ValueError("img_u8: expected a non-empty (H, W) or (H, W, C)")
    m, Ho, Wo, md, ss, rd = _warp_args(M, size, mode, supersample, reduce)
    Cn = 1 if img.ndim == 2 else img.shape[2]
    out = np.empty((Ho, Wo) + img.shape[2:], np.uint8)
    inside = np.empty((Ho, Wo), np.uint8)
    src, dst, ins = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(inside.ctypes.data)
    if (ss, rd) == (1, 0):
        check(lib().npp_warp_image_u8_host(src, img.shape[0], img.shape[1], Cn, Ho, Wo, m, md, dst, ins), "npp_warp_image_u8_host")
    else:
        check(lib().npp_warp_image_u8_ss_host(src, img.shape[0], img.shape[1], Cn, Ho, Wo, m, md, ss, rd, dst, ins),
              "npp_warp_image_u8_ss_host")
    return out, inside


def mlp_wgrad(dzT, actT, Bp, K, ksplit, gslabs, width=NPP_WIDTH):
    _req(gslabs, torch.float32, "gslabs")
    check(lib(width).npp_mlp_wgrad(_p(dzT), _p(actT), Bp, K, width, ksplit, _p(gslabs), _stream()), "npp_mlp_wgrad", width)


def stash8_census(actT, dzT, Bp, n_rows, K, record=None, width=NPP_WIDTH):
    """npp_stash8_census on one training workspace (actT / dzT as the launches were given them; a stacked workspace: image m's rows)
    -> the int64 record on the device (census_decode reads it).  Clears the record itself; nothing else is written."""
    from ._lib import census_layout
    words = census_layout(K, width)[2]
    if record is None:
        record = torch.empty(words, dtype=torch.int64, device=actT.device)
    _req(record, torch.int64, "record", (words,))
    check(lib(width).npp_stash8_census(_p(actT), _p(dzT), int(Bp), int(n_rows), K, width, _p(record), _stream()), "npp_stash8_census", width)
    return record


def stash8_census_host(act, dz, Bp, n_rows, K, width=NPP_WIDTH):
    """npp_stash8_census_host: the same record by plain C++ on host copies (uint8 NumPy arrays) of the same bytes."""
    from ._lib import census_layout
    act, dz = np.ascontiguousarray(act, np.uint8), np.ascontiguousarray(dz, np.uint8)
    rec = np.zeros(census_layout(K, width)[2], np.int64)
    check(lib(width).npp_stash8_census_host(C.c_void_p(act.ctypes.data), C.c_void_p(dz.ctypes.data), int(Bp), int(n_rows), K, width,
                                            C.c_void_p(rec.ctypes.data)), "npp_stash8_census_host", width)
    return rec


def census_decode(record, K, width=NPP_WIDTH):
    """An int64 census record (NumPy) -> ({array name: {"format", "features", "elements", "zero", "subnormal", "at_max", "nonfinite",
    "exp_hist": [32]}}, {"tiles", "scale_min", "scale_max"}), by the library's own table (census_layout)."""
    from ._lib import census_layout, CENSUS_TILE_FIELDS
    table, tile_off, _ = census_layout(K, width)
    rec = np.asarray(record, np.int64)
    out = {name: {"format": fmt, "features": feats, **audit.decode_entry(rec, off)} for name, fmt, feats, off in table}
    return out, {f: int(rec[tile_off + i]) for i, f in enumerate(CENSUS_TILE_FIELDS)}


def refuse_stash_audit(precision, exc=ValueError, flag=False, capturing=None):
    """The stash audit reads the 8-bit stash of the bf16 chain: refused by name where there is none (audit.refuse)."""
    audit.refuse("stash", exc, flag, capturing, precision=precision)


# ---- trunk audit: census of a stored fp16 trunk tensor ---------------------------------------------------
def trunk16_census(act, N_total, n, C, c_real, H, W, ref32=None, record=None):
    """npp_trunk16_census on one flat padded fp16 tensor (trunk_alloc's layout; logical (N_total, C, H, W)): the interior
    positions of images < n and the true channels < c_real -> the int64 record on the device (trunk16_census_decode reads it).
    ref32: the exact-fp32 trunk's tensor of the same layer, fp32 (>= n, c_real, H, W), for the ReLU-gate counters (None: both 0).
    Clears the record itself; nothing else is written."""
    from ._lib import TRUNK_CENSUS_WORDS
    nbytes = int(check(lib().npp_trunk_act_bytes(N_total, C, H, W), "npp_trunk_act_bytes"))
    if not (isinstance(act, torch.Tensor) and act.is_cuda and act.is_contiguous() and act.numel() * act.element_size() >= nbytes):
        raise ValueError(f"act: expected a contiguous flat trunk tensor of >= {nbytes} bytes on the GPU")
    if ref32 is not None:
        _req(ref32, torch.float32, "ref32")
        if ref32.dim() != 4 or ref32.shape[0] < n or tuple(ref32.shape[1:]) != (c_real, H, W):
            raise ValueError(f"ref32: expected shape (>= {n}, {c_real}, {H}, {W}), got {tuple(ref32.shape)}")
    if record is None:
        record = torch.empty(TRUNK_CENSUS_WORDS, dtype=torch.int64, device=act.device)
    _req(record, torch.int64, "record", (TRUNK_CENSUS_WORDS,))
    check(lib().npp_trunk16_census(_p(act), int(N_total), int(n), int(C), int(c_real), int(H), int(W), _p(ref32), _p(record), _stream()),
          "npp_trunk16_census")
    return record


def trunk16_census_host(act, N_total, n, C, c_real, H, W, ref32=None):
    """npp_trunk16_census_host: the same record by plain C++ on host copies (act: the tensor's bytes as a NumPy array of uint8 or
    uint16 codes; ref32: NumPy fp32 (>= n, c_real, H, W))."""
    import ctypes as ct                                       # (the parameter C, the channel count, shadows the module alias)
    from ._lib import TRUNK_CENSUS_WORDS
    act = np.ascontiguousarray(act)
    nbytes = int(check(lib().npp_trunk_act_bytes(N_total, C, H, W), "npp_trunk_act_bytes"))
    if act.dtype not in (np.uint8, np.uint16) or act.nbytes < nbytes:
        raise ValueError(f"act: expected >= {nbytes} bytes of uint8 / uint16 codes")
    rp = None
    if ref32 is not None:
        ref32 = np.ascontiguousarray(ref32, np.float32)
        if ref32.ndim != 4 or ref32.shape[0] < n or tuple(ref32.shape[1:]) != (c_real, H, W):
            raise ValueError(f"ref32: expected shape (>= {n}, {c_real}, {H}, {W}), got {tuple(ref32.shape)}")
        rp = ct.c_void_p(ref32.ctypes.data)
    rec = np.zeros(TRUNK_CENSUS_WORDS, np.int64)
    check(lib().npp_trunk16_census_host(ct.c_void_p(act.ctypes.data), int(N_total), int(n), int(C), int(c_real), int(H), int(W), rp,
                                        ct.c_void_p(rec.ctypes.data)), "npp_trunk16_census_host")
    return rec


def trunk16_census_decode(record):
    """An int64 trunk-census record (NumPy, TRUNK_CENSUS_WORDS words) -> {"format": "fp16", "elements", "zero", "subnormal", "at_max",
    "nonfinite", "exp_hist": [32], "gate_on", "gate_flips"}."""
    from ._lib import TRUNK_CENSUS_GATE_FIELDS, TRUNK_CENSUS_WORDS
    rec = np.asarray(record, np.int64).reshape(-1)
    if rec.shape[0] != TRUNK_CENSUS_WORDS:
        raise ValueError(f"record: expected {TRUNK_CENSUS_WORDS} int64 words, got {rec.shape[0]}")
    return {"format": "fp16", **audit.decode_entry(rec), **dict(zip(TRUNK_CENSUS_GATE_FIELDS, rec[-len(TRUNK_CENSUS_GATE_FIELDS):].tolist()))}


def trunk16_census_encode(entry):
    """The inverse of trunk16_census_decode: a decoded census -> its int64 record (NumPy)."""
    from ._lib import CENSUS_FIELDS, TRUNK_CENSUS_GATE_FIELDS
    return np.asarray([entry[f] for f in CENSUS_FIELDS] + list(entry["exp_hist"]) + [entry[f] for f in TRUNK_CENSUS_GATE_FIELDS], np.int64)


def trunk_census_flags(layers):
    """["saturated"] exactly when some layer of {name: decoded census} holds a value at 65504 or a non-finite one, else []."""
    return ["saturated"] if audit.saturated(layers.values()) else []


def rel_l2(a, b):
    """||a - b||_2 / ||b||_2 in float64 on the device -> a 0-dim float64 tensor (no read-back)."""
    a, b = a.double(), b.double()
    return torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-300)


def refuse_trunk_audit(trunk_precision="fp16", exc=ValueError, flag=False, capturing=None, patch_losses=True, stacked=False):
    """The trunk audit compares the fp16 trunks of the patch losses with the exact-fp32 trunks: refused by name where there is nothing
    16-bit to audit, for a fit without patch losses and for stacked fits (audit.refuse)."""
    audit.refuse("trunk", exc, flag, capturing, trunk_precision=trunk_precision, patch_losses=patch_losses, stacked=stacked)


def load_spline(device):
    """values|tangents fp32 on the device + (n_knots, x_scale); table: resources/partition_spline.npz
    (this repo's own derivation, tools/gen_partition_spline.py; distribution.py:129-141)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resources", "partition_spline.npz")
    with np.load(path) as f:
        vals, tans, xs = f["values"].astype(np.float32), f["tangents"].astype(np.float32), float(f["x_scale"])
    t = torch.from_numpy(np.concatenate([vals, tans])).to(device)
    return t, int(vals.shape[0]), xs


QUAD_COEF = {"robust_loss_adaptive": 0.0, "l2": 1.0, "robust_loss": 50.0}


def quad_coef(loss_type):
    """--loss_type (options/arg_config.py:34, models/mse_calculator.py:19-23) -> the `quad` switch of the pixel-loss kernels: 0 = the
    adaptive robust loss; 'l2' = mean(x^2); 'robust_loss' = lossfun(x, alpha = 2, scale = 0.1) = 0.5 (x / 0.1)^2 = 50 x^2."""
    if loss_type not in QUAD_COEF:
        raise ValueError(f"loss_type {loss_type!r}: one of {sorted(QUAD_COEF)}")
    return QUAD_COEF[loss_type]


def pixel_loss_quad(pred, gt, mask, coef, weight, loss, dpred):
    """img2mse(pred, gt, 'l2' | 'robust_loss', None, mask) + backward for one (N, 3) problem or C stacked ones (pred / dpred (C, N, 3),
    gt (N, 3) shared or (C, N, 3), loss (C)); loss is accumulated into."""
    _req(pred, torch.float32, "pred")
    _req(dpred, torch.float32, "dpred", pred.shape)
    nb = 1 if pred.dim() == 2 else pred.shape[0]
    n = pred.shape[-2]
    assert gt.is_contiguous() and gt.shape[-2:] == (n, 3) and loss.numel() >= nb and (mask is None or mask.numel() == n)
    check(lib().npp_pixel_loss_quad(_p(pred), _p(gt), 0 if gt.dim() == 2 else n * 3, _p(mask), n, nb, float(coef), float(weight), _p(loss),
                                    _p(dpred), _stream()), "npp_pixel_loss_quad")


def pixel_loss(pred, gt, mask, latents, spline, n_knots, x_scale, weight, loss, dpred, dlatent, quad=0.0):
    """img2mse(pred, gt, 'robust_loss_adaptive', adaptive_pix, mask) + backward
    (models/mse_calculator.py:13-27).  loss / dlatent are accumulated into (caller zeroes).  quad > 0: the non-adaptive forms."""
    _req(pred, torch.float32, "pred")
    _req(gt, torch.float32, "gt", pred.shape)
    n = pred.shape[0]
    if quad > 0:
        return pixel_loss_quad(pred, gt, mask, quad, weight, loss, dpred)
    check(lib().npp_pixel_loss(_p(pred), _p(gt), _p(mask), n, _p(latents), _p(spline), n_knots, x_scale, weight,
                               _p(loss), _p(dpred), _p(dlatent), _stream()), "npp_pixel_loss")


def adam_step(p, m, v, gslabs, n_slabs, slab_stride, lr, step, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam step (helpers.py:164) over the flat blob; g = sum of the slabs."""
    _req(p, torch.float32, "p")
    check(lib().npp_adam_step(_p(p), _p(m), _p(v), _p(gslabs), p.numel(), n_slabs, slab_stride, lr, b1, b2, eps,
                              step, _stream()), "npp_adam_step")


def adam_step_net(p, m, v, gslabs, n_slabs, slab_stride, lat, lat_m, lat_v, dlat, zero, lr, step,
                  b1=0.9, b2=0.999, eps=1e-8):
    """optimizer.step() over the network blob and the adaptive-loss latents in one launch; clears the
    latent gradient and `zero` (the next iteration's zero_grad of the small accumulators)."""
    _req(p, torch.float32, "p")
    check(lib().npp_adam_step_net(_p(p), _p(m), _p(v), _p(gslabs), p.numel(), n_slabs, slab_stride, _p(lat), _p(lat_m),
                                  _p(lat_v), _p(dlat), lat.numel(), _p(zero), 0 if zero is None else zero.numel(),
                                  lr, b1, b2, eps, step, _stream()), "npp_adam_step_net")


def adam_step_net_pack(p, m, v, gslabs, n_slabs, slab_stride, lat, lat_m, lat_v, dlat, zero, lr, step, K, wf, wb, width=NPP_WIDTH,
                       b1=0.9, b2=0.999, eps=1e-8, pl_partials=None, loss_cur=None):
    """adam_step_net + pack_weights in one launch: the updated weights are scattered into the bf16 packs wf / wb as well.
    pl_partials / loss_cur: the per-block sums the iteration's pixel-loss launch left in its scratch are added here, in block order,
    to the latent gradients and to the iteration's loss accumulator (include/npp_hip.h npp_pixel_loss_args.scratch)."""
    _req(p, torch.float32, "p")
    check(lib(width).npp_adam_step_net_pack(_p(p), _p(m), _p(v), _p(gslabs), p.numel(), n_slabs, slab_stride, _p(lat), _p(lat_m),
                                            _p(lat_v), _p(dlat), lat.numel(), _p(zero), 0 if zero is None else zero.numel(),
                                            lr, b1, b2, eps, step, K, width, _p(wf), _p(wb), _p(pl_partials), _p(loss_cur), _stream()),
          "npp_adam_step_net_pack", width)


def adam_words(lr, step, b1=0.9, b2=0.999):
    """(step_size, 1 / sqrt(1 - b2^t)) as the argument forms of the Adam launches compute them from (lr, step) -- the float
    arguments widened to double, pow / sqrt in double, the results rounded to float -- for the device-word forms
    (adam_step_dev, adam_step_net_pack_dev): np.float32 pair, equal to the launches' own values bit for bit."""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    bc1, bc2 = 1.0 - math.pow(b1, int(step)), 1.0 - math.pow(b2, int(step))
    return np.float32(lr / bc1), np.float32(1.0 / math.sqrt(bc2))


def lr_rule(lrate, lrate_decay, global_step):
    """The learning rate of the step after `global_step` schedule ticks (train.py:256-262): the one statement of the schedule; the
    fits' clocks (NPPNet.optimizer_advance, NPPNetLight.advance_clock) call it and then tick."""
    return lrate * (0.1 ** (global_step / (lrate_decay * 100)))


def adam_step_net_pack_dev(p, m, v, gslabs, n_slabs, slab_stride, lat, lat_m, lat_v, dlat, zero, hp, K, wf, wb, width=NPP_WIDTH,
                           b1=0.9, b2=0.999, eps=1e-8, pl_partials=None, loss_cur=None):
    """adam_step_net_pack whose step_size / bias correction come from the device tensor hp[0:2] (adam_words): the form a captured
    iteration replays (fit.CompletionFit(graph_iteration=True))."""
    _req(p, torch.float32, "p")
    _req(hp, torch.float32, "hp")
    if hp.numel() < 2:
        raise ValueError("hp: two floats (step_size, 1 / sqrt(1 - b2^t))")
    check(lib(width).npp_adam_step_net_pack_dev(_p(p), _p(m), _p(v), _p(gslabs), p.numel(), n_slabs, slab_stride, _p(lat), _p(lat_m),
                                                _p(lat_v), _p(dlat), lat.numel(), _p(zero), 0 if zero is None else zero.numel(),
                                                b1, b2, eps, _p(hp), K, width, _p(wf), _p(wb), _p(pl_partials), _p(loss_cur), _stream()),
          "npp_adam_step_net_pack_dev", width)


def patch_gather(img_hwc, mask_hw, centres_yx, P, want_mask=True, out=None):
    """extract_glimpse(mode='nearest', zeros padding) at integer centres
    (utils/extract_glimpse.py:53-79 via models/sampler.py:171-178,284-291).  out = (rgb, mask) buffers with room for at least
    M crops each (contiguous; a stacked fit's slice): written in place, the returned tensors are views of them."""
    _req(img_hwc, torch.float32, "img")
    _req(centres_yx, torch.int32, "centres")
    H, W = img_hwc.shape[:2]
    M = centres_yx.shape[0]
    if out is not None:
        rgb, msk = out[0][:M], out[1][:M]
        _req(rgb, torch.float32, "out rgb", (M, 3, P, P))
        _req(msk, torch.float32, "out mask", (M, 1, P, P))
    else:
        rgb = torch.empty((M, 3, P, P), dtype=torch.float32, device=img_hwc.device)
        msk = torch.empty((M, 1, P, P), dtype=torch.float32, device=img_hwc.device) if want_mask else None
    check(lib().npp_patch_gather(_p(img_hwc), _p(mask_hw), H, W, _p(centres_yx), M, P, _p(rgb), _p(msk), _stream()),
          "npp_patch_gather")
    return rgb, msk


def batch_assemble(i_train, pix, cen, P, bp, img_hwc, pmask_hw=None, out=None):
    """-> (coords int32 (bp,2), gt (n_pix,3), pmask (n_pix,) | None): the input rows of one loop iteration, train.py:166-181.
    out = (coords, gt[, pmask]): written in place (a stacked fit's slices)."""
    n_pix, n_p = pix.shape[0], 0 if cen is None else cen.shape[0]
    H, W = img_hwc.shape[:2]
    dev = img_hwc.device
    pm = None
    if out is not None:
        coords, gt = out[:2]
        pm = out[2] if len(out) > 2 else None
        _req(coords, torch.int32, "out coords", (bp, 2))
        _req(gt, torch.float32, "out gt", (n_pix, 3))
        if pm is not None:
            _req(pm, torch.float32, "out pmask", (n_pix,))
    else:
        coords = torch.empty((bp, 2), dtype=torch.int32, device=dev)
        gt = torch.empty((n_pix, 3), dtype=torch.float32, device=dev)
    if pmask_hw is None:
        pm = None
    elif pm is None:
        pm = torch.empty((n_pix,), dtype=torch.float32, device=dev)
    check(lib().npp_batch_assemble(_p(i_train), i_train.shape[0], _p(pix), n_pix, _p(cen), n_p, P, bp, _p(img_hwc), _p(pmask_hw), H, W,
                                   _p(coords), _p(gt), _p(pm), _stream()), "npp_batch_assemble")
    return coords, gt, pm


def dev_sampler_record_words(n_p, topk):
    return int(check(lib().npp_dev_sampler_record_words(int(n_p), int(topk)), "npp_dev_sampler_record_words"))


def dev_philox4x32_10(ctr, key):
    """Philox4x32-10 of one counter (4 words) under one key (2 words) -> 4 uint32: the generator of rng_mode="device", on the host."""
    c, k, out = (np.ascontiguousarray(v, np.uint32) for v in (ctr, key, np.zeros(4)))
    check(lib().npp_dev_philox4x32_10(c.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)),
          "npp_dev_philox4x32_10")
    return out


def dev_sampler_decide(imgs, M, ts, n_p, topk, rec):
    """The decision launch of rng_mode="device" for M images (npp_dev_sampler_decide): imgs = the npp_dev_image array in device
    memory (uint8), ts = the M draw indices (host, uint32), rec (M, stride) int32 = the records, written in place."""
    _req(imgs, torch.uint8, "imgs")
    _req(rec, torch.int32, "rec")
    ts = np.ascontiguousarray(ts, np.uint32)
    if ts.shape != (M,) or rec.dim() != 2 or rec.shape[0] != M:
        raise ValueError("dev_sampler_decide: one draw index and one record per image")
    check(lib().npp_dev_sampler_decide(_p(imgs), M, ts.ctypes.data_as(C.c_void_p), int(n_p), int(topk), _p(rec), rec.shape[1], _stream()),
          "npp_dev_sampler_decide")
    return rec


def dev_sampler_pixels(imgs, M, ts, n_pix, pix, n_train_min):
    """The pixel-row launch of rng_mode="device" (npp_dev_sampler_pixels): pix (M, >= n_pix) int64, written in place -- the
    indices npp_batch_assemble reads.  n_train_min: the smallest population of the M images (n_pix beyond it is refused like
    np.random.choice(replace=False) refuses it)."""
    if n_pix > n_train_min:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    _req(imgs, torch.uint8, "imgs")
    _req(pix, torch.int64, "pix")
    ts = np.ascontiguousarray(ts, np.uint32)
    if ts.shape != (M,) or pix.dim() != 2 or pix.shape[0] != M:
        raise ValueError("dev_sampler_pixels: one draw index and one row of indices per image")
    check(lib().npp_dev_sampler_pixels(_p(imgs), M, ts.ctypes.data_as(C.c_void_p), int(n_pix), _p(pix), pix.shape[1], _stream()),
          "npp_dev_sampler_pixels")
    return pix


_cx_ws = {}


def _cx_workspace(device, nbytes, st):
    """The contextual core's scratch (D, cx, mu, row sums and the last-arriver tickets of its six launches): ONE PER STREAM -- two fits
    of one shape on two streams (bench throughput mode, the LPIPS side stream) would otherwise race on the matrices and the tickets."""
    key = (device, int(nbytes), st.value)
    ws = _cx_ws.get(key)
    if ws is None:
        ws = _cx_ws[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return ws


def _cx_intake(fx, fy):
    """What the three CX wrappers do first: fp32 features (N, C, h, w) of one shape -> N, C, hw, the stream's workspace, its byte
    count and the stream."""
    _req(fx, torch.float32, "fx")
    _req(fy, torch.float32, "fy", fx.shape)
    N, C = fx.shape[:2]
    hw = fx.shape[2] * fx.shape[3]
    nbytes = lib().npp_cx_workspace_bytes(N, C, hw)
    check(nbytes, "npp_cx_workspace_bytes")
    st = _stream()
    return N, C, hw, _cx_workspace(fx.device, nbytes, st), nbytes, st


def cx_fwd_bwd(fx, fy, band_width=0.5, weight=None, scale=1.0, loss=None, want_grad=True):
    """contextual_loss(x, y, band_width, weight, 'cosine') on features (N,C,h,w) + dL/dx
    (externel_lib/contextual_loss/functional.py:9-63).  Returns (loss tensor[1], dfx or None)."""
    N, C, hw, ws, nbytes, st = _cx_intake(fx, fy)
    if loss is None:
        loss = torch.zeros(1, dtype=torch.float32, device=fx.device)
    dfx = torch.empty_like(fx) if want_grad else None
    check(lib().npp_cx_fwd_bwd(_p(fx), _p(fy), N, C, hw, band_width, _p(weight), scale, _p(loss), _p(dfx), _p(ws),
                               int(nbytes), st), "npp_cx_fwd_bwd")
    return loss, dfx


_lp_ws = {}


def lpips_layer(f0, f1, lin, latents, spline, n_knots, x_scale, scale, loss, df0=None, dlatent=None):
    """One VGG16 tap of LPIPS.forward(use_robust=True) (externel_lib/lpips/lpips.py:99-121,130); latents None: the plain head
    (use_robust=False, lpips.py:108-109) with its gradient df0 (spline / dlatent unused)."""
    if latents is None:
        spline, n_knots, x_scale, dlatent = None, 0, 0.0, None
    _req(f0, torch.float32, "f0")
    _req(f1, torch.float32, "f1", f0.shape)
    N, C = f0.shape[:2]
    hw = f0.shape[2] * f0.shape[3]
    key = (f0.device, C, _stream().value)               # (accumulators of a launch in flight: one workspace per stream)
    ws = _lp_ws.get(key)
    if ws is None and DETERMINISTIC:
        ws = _lp_ws[key] = torch.zeros(int(lib().npp_lpips_workspace_bytes(C)), dtype=torch.uint8, device=f0.device)
    check(lib().npp_lpips_layer(_p(f0), _p(f1), N, C, hw, _p(lin), _p(latents), _p(spline), n_knots, x_scale, scale,
                                _p(loss), _p(df0), _p(dlatent), _p(ws), _stream()), "npp_lpips_layer")


def lpips_layers(f0s, f1s, lins, latents, spline, n_knots, x_scale, scale, loss, df0s=None, dlatents=None, dflats=None):
    """All taps of LPIPS.forward in ONE launch (the heads are independent of each other): lists per tap of the arguments of lpips_layer
    (latents None: the plain head for every tap).  dflats[i] = (flat bf16 tensor from trunk_alloc, N_total[, yact]) takes the place of
    df0s[i] (then None): the tap's gradient goes straight into the trunk's flat layout, gated by [yact > 0] when the tapped layer's
    flat activation is given."""
    from ._lib import LpipsTap
    n = len(f0s)
    N = f0s[0].shape[0]
    arr = (LpipsTap * n)()
    st = _stream()
    for i in range(n):
        f0, f1 = f0s[i], f1s[i]
        _req(f0, torch.float32, "f0")
        _req(f1, torch.float32, "f1", f0.shape)
        Cc = f0.shape[1]
        ws = None
        if DETERMINISTIC:
            key = (f0.device, Cc, st.value, i)             # one workspace per (stream, tap): the taps of the launch run side by side
            ws = _lp_ws.get(key)
            if ws is None:
                ws = _lp_ws[key] = torch.zeros(int(lib().npp_lpips_workspace_bytes(Cc)), dtype=torch.uint8, device=f0.device)
        fl = None if dflats is None else dflats[i]
        arr[i] = LpipsTap(f0.data_ptr(), f1.data_ptr(), Cc, f0.shape[2] * f0.shape[3], lins[i].data_ptr(),
                          None if latents is None else latents[i].data_ptr(),
                          None if (df0s is None or df0s[i] is None) else df0s[i].data_ptr(),
                          None if (dlatents is None or latents is None) else dlatents[i].data_ptr(), None if ws is None else ws.data_ptr(),
                          None if fl is None else fl[0].data_ptr(), 0 if fl is None else int(fl[1]), f0.shape[2], f0.shape[3],
                          None if (fl is None or len(fl) < 3 or fl[2] is None) else fl[2].data_ptr())
    check(lib().npp_lpips_layers(n, arr, N, None if latents is None else _p(spline), n_knots if latents is not None else 0,
                                 x_scale if latents is not None else 0.0, scale, _p(loss), st), "npp_lpips_layers")


def adam_step_dev(p, m, v, gslabs, n_slabs, slab_stride, hp, b1=0.9, b2=0.999, eps=1e-8):
    """Adam step whose step_size / bias correction come from the device tensor hp[0:2]
    (graph-replayable form of adam_step)."""
    check(lib().npp_adam_step_dev(_p(p), _p(m), _p(v), _p(gslabs), p.numel(), n_slabs, slab_stride, b1, b2, eps, _p(hp),
                                  _stream()), "npp_adam_step_dev")


# ---- a11 / a13 trunks: conv3x3 + ReLU / MaxPool2d stacks on flat padded bf16 tensors ----------------
def trunk_nposp(N, H, W):
    return int(check(lib().npp_trunk_nposp(N, H, W), "npp_trunk_nposp"))


def trunk_alloc(N, C, H, W, device):
    """Zero-initialised flat tensor for a logical (N,C,H,W) activation (csrc/npp_conv.hip layout)."""
    nbytes = int(check(lib().npp_trunk_act_bytes(N, C, H, W), "npp_trunk_act_bytes"))
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def conv_pack(weight, in_natural=False):
    """torch Conv2d weight (Cout,Cin,3,3) fp32 -> (forward pack, data-gradient pack), bf16 MFMA fragments."""
    _req(weight, torch.float32, "weight")
    cout, cin = weight.shape[:2]
    assert tuple(weight.shape[2:]) == (3, 3)
    nf = int(check(lib().npp_conv_pack_bytes(cin, cout, 0), "npp_conv_pack_bytes"))
    nb = int(check(lib().npp_conv_pack_bytes(cin, cout, 1), "npp_conv_pack_bytes"))
    pf = torch.empty(nf, dtype=torch.uint8, device=weight.device)
    pb = torch.empty(nb, dtype=torch.uint8, device=weight.device)
    check(lib().npp_conv_pack(_p(weight), cin, cout, int(bool(in_natural)), _p(pf), _p(pb), _stream()), "npp_conv_pack")
    return pf, pb


def trunk_image_in(img, scale, shift, x0):
    """(N,3,H,W) fp32 -> flat C=16 tensor of img*scale[c] + shift[c]."""
    _req(img, torch.float32, "img")
    N, c, H, W = img.shape
    assert c == 3
    s = (C.c_float * 3)(*[float(v) for v in scale])
    b = (C.c_float * 3)(*[float(v) for v in shift])
    check(lib().npp_trunk_image_in(_p(img), N, H, W, s, b, _p(x0), _stream()), "npp_trunk_image_in")


def trunk_patch_in(pred_rows, fake, fmask, real, rmask, n_p, k, P, comp, scale, shift, x0, xy=None, zero=None, which=0, loss=None):
    """npp_patch_compose_fwd + npp_trunk_image_in in one launch: [x | y] -> flat trunk input x0 (and fp32 xy when given);
    zero (small fp32 tensor) is cleared on the way.  which: 0 both halves, 1 prediction half only, 2 real half only
    (x0 then holds n_p*k images).  loss = the argument tuple of pixel_loss(): that loss rides in the same launch."""
    if which != 2:
        _req(pred_rows, torch.float32, "pred_rows", (n_p * P * P, 3))
    if which != 1:
        _req(real, torch.float32, "real", (n_p * k, 3, P, P))
    _req(rmask, torch.float32, "rmask", (n_p * k, 1, P, P))
    if comp and which != 2:
        _req(fake, torch.float32, "fake", (n_p, 3, P, P))
        _req(fmask, torch.float32, "fmask", (n_p, 1, P, P))
    if xy is not None:
        _req(xy, torch.float32, "xy", (2 * n_p * k, 3, P, P))
    s = (C.c_float * 3)(*[float(v) for v in scale])
    b = (C.c_float * 3)(*[float(v) for v in shift])
    if loss is not None:
        from ._lib import PixelLossArgs
        pred, gt, mask, latents, spline, n_knots, x_scale, weight, loss_buf, dpred, dlatent = loss[:11]
        scratch = loss[11] if len(loss) > 11 else None        # PIXEL_LOSS_SCRATCH floats: fixed-order sums (include/npp_hip.h)
        quad = float(loss[12]) if len(loss) > 12 else 0.0     # > 0: --loss_type l2 / robust_loss (quad_coef)
        _req(pred, torch.float32, "pred")
        _req(gt, torch.float32, "gt", pred.shape)
        la = PixelLossArgs(pred.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), pred.shape[0], latents.data_ptr(),
                           spline.data_ptr(), int(n_knots), float(x_scale), float(weight), loss_buf.data_ptr(), dpred.data_ptr(),
                           dlatent.data_ptr(), None if scratch is None else scratch.data_ptr(), quad)
        check(lib().npp_trunk_patch_in_loss(_p(pred_rows), _p(fake), _p(fmask), _p(real), _p(rmask), n_p, k, P, int(bool(comp)), s, b,
                                            _p(x0), _p(xy), _p(zero), 0 if zero is None else zero.numel(), int(which), C.byref(la),
                                            _stream()), "npp_trunk_patch_in_loss")
        return
    check(lib().npp_trunk_patch_in(_p(pred_rows), _p(fake), _p(fmask), _p(real), _p(rmask), n_p, k, P, int(bool(comp)), s, b,
                                   _p(x0), _p(xy), _p(zero), 0 if zero is None else zero.numel(), int(which), _stream()),
          "npp_trunk_patch_in")


def conv3x3(x, N_total, n_run, H, W, cin, cout, pack, bias, mode, mask, y, tap=None, ctap=0, tap_scale=None, next_pack=None):
    """next_pack: the weight pack of the launch that follows (its lines are requested into L2 by this one)."""
    ts = None if tap_scale is None else (C.c_float * len(tap_scale))(*[float(v) for v in tap_scale])
    if next_pack is not None:
        check(lib().npp_conv3x3_pf(_p(x), N_total, n_run, H, W, cin, cout, _p(pack), _p(bias), mode, _p(mask), _p(y), _p(tap),
                                   ctap, ts, _p(next_pack), next_pack.numel() * next_pack.element_size(), _stream()), "npp_conv3x3_pf")
        return
    check(lib().npp_conv3x3(_p(x), N_total, n_run, H, W, cin, cout, _p(pack), _p(bias), mode, _p(mask), _p(y), _p(tap),
                            ctap, ts, _stream()), "npp_conv3x3")


CONV_PLAN_FIELDS = ("family", "ct", "pt", "s", "npt", "wstat", "grid_x", "grid_y", "lds")
CONV_PLAN_FAMILIES = ("tile", "win", "wink")


def conv3x3_plan(N_total, n_run, H, W, cin, cout, mode, fold=0):
    """The kernel form the launch of these arguments takes under the current tune() values (npp_conv3x3_plan: host only, no GPU) as
    a dict of CONV_PLAN_FIELDS, family by name.  fold: 0 conv3x3, 1 conv3x3_pool (mode 0), 2 conv3x3_dgrad_pool (mode 2)."""
    out = (C.c_int32 * len(CONV_PLAN_FIELDS))()
    check(lib().npp_conv3x3_plan(N_total, n_run, H, W, cin, cout, mode, fold, out), "npp_conv3x3_plan")
    p = dict(zip(CONV_PLAN_FIELDS, (int(v) for v in out)))
    p["family"] = CONV_PLAN_FAMILIES[p["family"]]
    return p


def conv3x3_pool(x, N_total, n_run, H, W, cin, cout, pack, bias, y, ypool, tap=None, ctap=0, tap_scale=None, next_pack=None):
    """Forward layer + the 2 x 2 max-pool that follows it in one launch (y: the layer's output, ypool: the pooled tensor)."""
    ts = None if tap_scale is None else (C.c_float * len(tap_scale))(*[float(v) for v in tap_scale])
    nb = 0 if next_pack is None else next_pack.numel() * next_pack.element_size()
    check(lib().npp_conv3x3_pool(_p(x), N_total, n_run, H, W, cin, cout, _p(pack), _p(bias), _p(y), _p(ypool), _p(tap), ctap, ts,
                                 _p(next_pack), nb, _stream()), "npp_conv3x3_pool")


def conv_pair_fwd_ok(H, W, cin, cmid, cout):
    """Whether the fused conv a -> conv b -> pool launch is built for this shape (and switched on: tune("conv_pair"))."""
    return bool(lib().npp_conv_pair_fwd_ok(H, W, cin, cmid, cout))


def conv_pair_fwd(x, N_total, n_run, n_keep, H, W, cin, cmid, cout, pack_a, bias_a, pack_b, bias_b, y_a, y_b, y_pool, tap_b=None):
    """relu(conv a) -> relu(conv b) -> MaxPool2d(2,2) in one launch; y_a / y_b only for the first n_keep images."""
    check(lib().npp_conv_pair_fwd(_p(x), N_total, n_run, n_keep, H, W, cin, cmid, cout, _p(pack_a), _p(bias_a), _p(pack_b), _p(bias_b),
                                  _p(y_a), _p(y_b), _p(y_pool), _p(tap_b), _stream()), "npp_conv_pair_fwd")


def _pixel_loss_args(loss):
    """The argument tuple of pixel_loss() (NPPNet.pixel_loss_args) as the C struct npp_pixel_loss_args."""
    from ._lib import PixelLossArgs
    pred, gt, mask, latents, spline, n_knots, x_scale, weight, loss_buf, dpred, dlatent = loss[:11]
    scratch = loss[11] if len(loss) > 11 else None
    quad = float(loss[12]) if len(loss) > 12 else 0.0
    _req(pred, torch.float32, "pred")
    _req(gt, torch.float32, "gt", pred.shape)
    return PixelLossArgs(pred.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), pred.shape[0], latents.data_ptr(),
                         spline.data_ptr(), int(n_knots), float(x_scale), float(weight), loss_buf.data_ptr(), dpred.data_ptr(),
                         dlatent.data_ptr(), None if scratch is None else scratch.data_ptr(), quad)


def conv_pair_fwd_patch(pred_rows, fake, fmask, real, rmask, n_p, k, P, comp, scale, shift, zero, loss, n_keep, cmid, cout,
                        pack_a, bias_a, pack_b, bias_b, y_a, y_b, y_pool, tap_b=None):
    """trunk_patch_in(loss=...) + conv_pair_fwd of the first block in one launch (no flat input tensor, no fp32 batch copy)."""
    _req(pred_rows, torch.float32, "pred_rows", (n_p * P * P, 3))
    _req(real, torch.float32, "real", (n_p * k, 3, P, P))
    _req(rmask, torch.float32, "rmask", (n_p * k, 1, P, P))
    if comp:
        _req(fake, torch.float32, "fake", (n_p, 3, P, P))
        _req(fmask, torch.float32, "fmask", (n_p, 1, P, P))
    s = (C.c_float * 3)(*[float(v) for v in scale])
    b = (C.c_float * 3)(*[float(v) for v in shift])
    la = None if loss is None else _pixel_loss_args(loss)
    check(lib().npp_conv_pair_fwd_patch(_p(pred_rows), _p(fake), _p(fmask), _p(real), _p(rmask), n_p, k, P, int(bool(comp)), s, b, _p(zero),
                                        0 if zero is None else zero.numel(), None if la is None else C.byref(la), n_keep, cmid, cout,
                                        _p(pack_a), _p(bias_a), _p(pack_b), _p(bias_b), _p(y_a), _p(y_b), _p(y_pool), _p(tap_b), _stream()),
          "npp_conv_pair_fwd_patch")


def conv_pair_dgrad(dz_b, N_total, n_run, H, W, cmid, pack_b_bwd, y_a, pack_a_bwd, dimg, scale):
    """dL/d(pre-activation of conv b) -> dL/dimage through the first block in one launch (conv b dgrad, conv a's ReLU gate, conv a dgrad)."""
    ts = (C.c_float * 3)(*[float(v) for v in scale])
    check(lib().npp_conv_pair_dgrad(_p(dz_b), N_total, n_run, H, W, cmid, _p(pack_b_bwd), _p(y_a), _p(pack_a_bwd), _p(dimg), ts, _stream()),
          "npp_conv_pair_dgrad")


def conv3x3_dgrad_pool(x, N_total, n_run, H, W, cin, cout, pack, xpre, addend, dz, next_pack=None):
    """Data gradient of a convolution that reads a pooled tensor + the pool's backward + the pre-pool ReLU gate (+ tap gradient)
    in one launch; H, W: the pooled geometry, xpre / addend / dz: the pre-pool layer's flat tensors."""
    nb = 0 if next_pack is None else next_pack.numel() * next_pack.element_size()
    check(lib().npp_conv3x3_dgrad_pool(_p(x), N_total, n_run, H, W, cin, cout, _p(pack), _p(xpre), _p(addend), _p(dz),
                                       _p(next_pack), nb, _stream()), "npp_conv3x3_dgrad_pool")


def maxpool2_fwd(x, N, H, W, c, y):
    check(lib().npp_maxpool2_fwd(_p(x), N, H, W, c, _p(y), _stream()), "npp_maxpool2_fwd")


def maxpool2_bwd(dy, x, addend, N_total, n_run, H, W, c, dz):
    check(lib().npp_maxpool2_bwd(_p(dy), _p(x), _p(addend), N_total, n_run, H, W, c, _p(dz), _stream()), "npp_maxpool2_bwd")


def trunk_grad_in(df, y, N_total, n_run, c, H, W, dz, as_f16=False, accumulate=False, next_pack=None):
    _req(df, torch.float32, "df", (n_run, c, H, W))
    if next_pack is not None:
        check(lib().npp_trunk_grad_in_pf(_p(df), _p(y), N_total, n_run, c, H, W, _p(dz), int(bool(as_f16)), int(bool(accumulate)),
                                         _p(next_pack), next_pack.numel() * next_pack.element_size(), _stream()), "npp_trunk_grad_in_pf")
        return
    check(lib().npp_trunk_grad_in(_p(df), _p(y), N_total, n_run, c, H, W, _p(dz), int(bool(as_f16)), int(bool(accumulate)), _stream()),
          "npp_trunk_grad_in")


def trunk_export(act, N_total, n_run, c, H, W, is_f16=False):
    out = torch.empty((n_run, c, H, W), dtype=torch.float32, device=act.device)
    check(lib().npp_trunk_export(_p(act), N_total, n_run, c, H, W, _p(out), int(bool(is_f16)), _stream()), "npp_trunk_export")
    return out


# ---- the trunks in exact fp32 (csrc/npp_conv32.hip): plain fp32 NCHW tensors --------------------------------
def conv32_pack(weight):
    """torch Conv2d weight (Cout,Cin,3,3) fp32 -> (forward pack, data-gradient pack), fp32 MFMA operands."""
    _req(weight, torch.float32, "weight")
    cout, cin = weight.shape[:2]
    assert tuple(weight.shape[2:]) == (3, 3)
    nf = int(check(lib().npp_conv32_pack_bytes(cin, cout, 0), "npp_conv32_pack_bytes"))
    nb = int(check(lib().npp_conv32_pack_bytes(cin, cout, 1), "npp_conv32_pack_bytes"))
    pf = torch.empty(nf // 4, dtype=torch.float32, device=weight.device)
    pb = torch.empty(nb // 4, dtype=torch.float32, device=weight.device)
    check(lib().npp_conv32_pack(_p(weight), cin, cout, _p(pf), _p(pb), _stream()), "npp_conv32_pack")
    return pf, pb


def _f3(v):
    return None if v is None else (C.c_float * 3)(*[float(t) for t in v])


def conv32(x, n_run, cout, pack, mode, y, bias=None, in_norm=None, in_gate=None, gate=None, add=None, out_scale=None):
    """npp_conv32 on x (N, Cin, H, W) -> y (N, Cout, H, W), the leading n_run images.  mode 0: relu(conv + bias), in_norm =
    (scale, shift) of the image layer; 1: data gradient (gate / add: the layer below's stored output / tap gradient);
    2: the image layer's data gradient times out_scale.  in_gate: the layer's own stored output (x is dL/d(its output))."""
    _req(x, torch.float32, "x")
    N, cin, H, W = x.shape
    if n_run > N:
        raise ValueError(f"x: {N} images, n_run = {n_run}")
    for t, name in ((y, "y"), (in_gate, "in_gate"), (gate, "gate"), (add, "add")):
        if t is not None:
            _req(t, torch.float32, name)
            if tuple(t.shape[1:]) != ((cin, H, W) if name == "in_gate" else (cout, H, W)) or t.shape[0] < n_run:
                raise ValueError(f"{name}: shape {tuple(t.shape)} does not cover {n_run} images of this launch")
    sc, sh = (None, None) if in_norm is None else in_norm
    check(lib().npp_conv32(_p(x), N, n_run, H, W, cin, cout, _p(pack), mode, _p(bias), _f3(sc), _f3(sh), _p(in_gate), _p(gate), _p(add),
                           _f3(out_scale), _p(y), _stream()), "npp_conv32")
    return y


def maxpool2_fwd32(x, n_run, y=None):
    _req(x, torch.float32, "x")
    N, c, H, W = x.shape
    if y is None:
        y = torch.empty((N, c, H // 2, W // 2), dtype=torch.float32, device=x.device)
    _req(y, torch.float32, "y", (N, c, H // 2, W // 2))
    check(lib().npp_maxpool2_fwd32(_p(x), N, n_run, H, W, c, _p(y), _stream()), "npp_maxpool2_fwd32")
    return y


def maxpool2_bwd32(dy, x, n_run, dz, add=None, gate=True):
    """dz = (route(dy) + add) * [x > 0 if gate] on the leading n_run images; x: the pool's fp32 input (N, C, H, W)."""
    _req(x, torch.float32, "x")
    N, c, H, W = x.shape
    _req(dy, torch.float32, "dy")
    if tuple(dy.shape[1:]) != (c, H // 2, W // 2) or dy.shape[0] < n_run:
        raise ValueError(f"dy: shape {tuple(dy.shape)} is not the pooled gradient of {n_run} images of {tuple(x.shape)}")
    _req(dz, torch.float32, "dz", x.shape)
    if add is not None:
        _req(add, torch.float32, "add")
        if tuple(add.shape[1:]) != (c, H, W) or add.shape[0] < n_run:
            raise ValueError(f"add: shape {tuple(add.shape)} does not cover {n_run} images of {tuple(x.shape)}")
    check(lib().npp_maxpool2_bwd32(_p(dy), _p(x), _p(add), N, n_run, H, W, c, int(bool(gate)), _p(dz), _stream()), "npp_maxpool2_bwd32")
    return dz


# ---- a10: patch plumbing (train.py:200-236) -----------------------------------------------------------
def patch_compose_fwd(pred_rows, fake, fmask, real, rmask, n_p, k, P, comp, xy=None):
    """-> xy (2*n_p*k, 3, P, P) = [x | y] (see include/npp_hip.h)."""
    _req(pred_rows, torch.float32, "pred_rows", (n_p * P * P, 3))
    _req(real, torch.float32, "real", (n_p * k, 3, P, P))
    _req(rmask, torch.float32, "rmask", (n_p * k, 1, P, P))
    if comp:
        _req(fake, torch.float32, "fake", (n_p, 3, P, P))
        _req(fmask, torch.float32, "fmask", (n_p, 1, P, P))
    if xy is None:
        xy = torch.empty((2 * n_p * k, 3, P, P), dtype=torch.float32, device=pred_rows.device)
    check(lib().npp_patch_compose_fwd(_p(pred_rows), _p(fake), _p(fmask), _p(real), _p(rmask), n_p, k, P, int(bool(comp)),
                                      _p(xy), _stream()), "npp_patch_compose_fwd")
    return xy


def patch_compose_bwd(dx_a, dx_b, fmask, rmask, n_p, k, P, comp, dpred_rows):
    _req(dpred_rows, torch.float32, "dpred_rows", (n_p * P * P, 3))
    check(lib().npp_patch_compose_bwd(_p(dx_a), _p(dx_b), _p(fmask), _p(rmask), n_p, k, P, int(bool(comp)), _p(dpred_rows),
                                      _stream()), "npp_patch_compose_bwd")


# ---- generic dense layers (exact fp32): F.linear + snake and their autograd ----------------
def linear_fwd(x, w, b, act, y, z=None):
    """y = act(x w^T + b) on row-major 2-D tensors; x / y / z may be column blocks of wider buffers (stride(0) = ld)."""
    B, cin = x.shape
    cout = w.shape[0]
    assert w.shape[1] == cin and y.shape == (B, cout) and x.stride(1) == 1 and y.stride(1) == 1 and w.is_contiguous()
    check(lib().npp_linear_fwd(_p(x), x.stride(0), _p(w), _p(b), B, cin, cout, act, _p(y), y.stride(0), _p(z),
                               0 if z is None else z.stride(0), _stream()), "npp_linear_fwd")
    return y


def linear_bwd_data(dz, w, dx, in_used=None, accumulate=False):
    """dx (+)= dz w.  `w` may be a column slice w_full[:, a:b] of the (out, in) matrix (gradient w.r.t. one block of a
    concatenated input, networks.py:71,76,85)."""
    B, cout = dz.shape
    cin = w.stride(0)                                    # leading dimension of the full matrix
    in_used = w.shape[1] if in_used is None else in_used
    assert dx.shape == (B, in_used) and dz.stride(1) == 1 and dx.stride(1) == 1 and w.stride(1) == 1
    check(lib().npp_linear_bwd_data(_p(dz), dz.stride(0), _p(w), B, cin, cout, _p(dx), dx.stride(0), in_used, int(bool(accumulate)),
                                    _stream()), "npp_linear_bwd_data")
    return dx


def linear_bwd_weight(dz, x, dw, db=None, accumulate=False):
    B, cout = dz.shape
    cin = x.shape[1]
    assert dw.shape == (cout, cin) and dw.is_contiguous() and x.stride(1) == 1 and dz.stride(1) == 1
    check(lib().npp_linear_bwd_weight(_p(dz), dz.stride(0), _p(x), x.stride(0), B, cin, cout, _p(dw), _p(db), int(bool(accumulate)),
                                      _stream()), "npp_linear_bwd_weight")


# ---- the same layers over several independent problems of one shape in one launch (light.NPPNetLightBatch) -----------------
def linear_fwd_batched(x, w, b, act, y, z=None):
    """y[c] = act(x[c] w[c]^T + b[c]): x (C,B,in), w (C,out,in), b (C,out), y / z (C,B,out); any batch strides, rows may be column
    blocks of wider buffers.  x may be shared by the problems (stride(0) == 0)."""
    C, B, cin = x.shape
    cout = w.shape[1]
    assert w.shape == (C, cout, cin) and y.shape == (C, B, cout) and b.shape == (C, cout)
    assert x.stride(2) == 1 and y.stride(2) == 1 and w.stride(2) == 1 and w.stride(1) == cin and b.stride(1) == 1
    assert z is None or (z.shape == y.shape and z.stride(2) == 1)
    check(lib().npp_linear_fwd_batched(_p(x), x.stride(1), x.stride(0), _p(w), w.stride(0), _p(b), b.stride(0), C, B, cin, cout, act, _p(y),
                                       y.stride(1), y.stride(0), _p(z), 0 if z is None else z.stride(1), 0 if z is None else z.stride(0),
                                       _stream()), "npp_linear_fwd_batched")
    return y


def linear_bwd_data_batched(dz, w, dx, in_used=None, accumulate=False, zy=None, act=0):
    """dx[c] (+)= dz[c] w[c] (first in_used input columns); with zy (C,B,in_used) and act: dx[c] = (dz[c] w[c]) * act'(zy[c]) -- the
    activation backward of the layer below folded into this launch (act / zy as act_bwd takes them)."""
    C, B, cout = dz.shape
    cin = w.shape[2]
    in_used = cin if in_used is None else in_used
    assert w.shape == (C, cout, cin) and dx.shape == (C, B, in_used) and dz.stride(2) == 1 and dx.stride(2) == 1
    assert w.stride(2) == 1 and w.stride(1) == cin
    assert zy is None or (zy.shape == dx.shape and zy.stride(2) == 1)
    check(lib().npp_linear_bwd_data_batched(_p(dz), dz.stride(1), dz.stride(0), _p(w), w.stride(0), C, B, cin, cout, _p(dx), dx.stride(1),
                                            dx.stride(0), in_used, int(bool(accumulate)), _p(zy), 0 if zy is None else zy.stride(1),
                                            0 if zy is None else zy.stride(0), int(act), _stream()), "npp_linear_bwd_data_batched")
    return dx


def linear_bwd_weight_batched(dz, x, dw, db):
    """dw[c] += dz[c]^T x[c], db[c] += column sums of dz[c] (ACCUMULATES: the contraction is split; clear the gradients first)."""
    C, B, cout = dz.shape
    cin = x.shape[2]
    assert dw.shape == (C, cout, cin) and dw.stride(2) == 1 and dw.stride(1) == cin and db.shape == (C, cout) and db.stride(1) == 1
    assert x.shape[:2] == (C, B) and x.stride(2) == 1 and dz.stride(2) == 1
    check(lib().npp_linear_bwd_weight_batched(_p(dz), dz.stride(1), dz.stride(0), _p(x), x.stride(1), x.stride(0), C, B, cin, cout, _p(dw),
                                              dw.stride(0), _p(db), db.stride(0), _stream()), "npp_linear_bwd_weight_batched")


def pixel_loss_batched(pred, gt, latents, spline, n_knots, x_scale, weight, loss, dpred, dlatent):
    """pixel_loss() for C problems: pred / dpred (C,N,3) contiguous, latents / dlatent (C,6), loss (C); gt (N,3) shared or (C,N,3)."""
    _req(pred, torch.float32, "pred")
    C, n = pred.shape[:2]
    assert pred.is_contiguous() and dpred.is_contiguous() and dpred.shape == pred.shape and gt.is_contiguous()
    assert latents.shape == (C, 6) and dlatent.shape == (C, 6) and loss.numel() == C and latents.is_contiguous() and dlatent.is_contiguous()
    assert gt.shape in ((n, 3), (C, n, 3))
    check(lib().npp_pixel_loss_batched(_p(pred), _p(gt), 0 if gt.dim() == 2 else n * 3, n, C, _p(latents), _p(spline), n_knots, x_scale,
                                       weight, _p(loss), _p(dpred), _p(dlatent), _stream()), "npp_pixel_loss_batched")


def linear_bwd_weight_strided(dz, x, dw, db, feature_major_dz, feature_major_x, x_snake=False):
    """dw[c] += dz[c]^T x[c], db[c] += column sums of dz[c], for operands that are row-major (C, B, n) or feature-major (C, n, B) --
    the stashes of the fused NPP_Net_light chains (x_snake: x holds pre-activations, the layer input is snake(x)).  dw (C, out, ld >= in)
    views of a blob, db (C, out)."""
    C = dz.shape[0]
    B, cout = (dz.shape[2], dz.shape[1]) if feature_major_dz else (dz.shape[1], dz.shape[2])
    cin = dw.shape[2]
    assert dz.stride(2) == 1 and x.stride(2) == 1 and dw.stride(2) == 1 and dw.shape[:2] == (C, cout) and db.shape == (C, cout) and db.stride(1) == 1
    assert (x.shape[1] >= cin and x.shape[2] == B) if feature_major_x else (x.shape[1] == B and x.shape[2] >= cin)
    dz_sr, dz_so = (1, dz.stride(1)) if feature_major_dz else (dz.stride(1), 1)
    x_sr, x_si = (1, x.stride(1)) if feature_major_x else (x.stride(1), 1)
    check(lib().npp_linear_bwd_weight_strided(_p(dz), dz_sr, dz_so, dz.stride(0), _p(x), x_sr, x_si, x.stride(0), int(bool(x_snake)), C, B, cin, cout, _p(dw),
                                              dw.stride(1), dw.stride(0), _p(db), db.stride(0), _stream()), "npp_linear_bwd_weight_strided")


# ---- f1: the fused NPP_Net_light chains (csrc/npp_light.hip exact fp32, csrc/npp_light16.hip bf16 operands) ---------------------------
class BoundCall:
    """A library entry point with its arguments checked and marshalled by the wrapper that built it (bind=True), not launched yet.
    call() launches and returns the entry point's code for check(); before it, args[slots[name]] = value replaces an argument the
    wrapper named (raw device addresses / scalars: their tensors are the caller's to keep valid).  A loop that repeats a launch
    sequence pays the wrapper once (light.NPPNetLightBatch)."""
    __slots__ = ("fn", "what", "args", "slots")

    def __init__(self, what, args, slots):
        self.fn, self.what, self.args, self.slots = getattr(lib(), what), what, list(args), slots

    def __call__(self):
        return self.fn(*self.args)


def _go(what, args, bind=False, **slots):
    """Launch entry point `what` -- or (bind) hand the call back; slots: argument positions that call may replace by name."""
    if bind:
        return BoundCall(what, args, slots)
    check(getattr(lib(), what)(*args), what)


def _light_fwd_inputs(x_per, x_pos, pred, idx):
    """The forward inputs of C candidates: tables x_per (C, n, 20) and x_pos (n, 42) whose rows idx (B int64 on the device; None: n == B, row
    r itself) are the batch -> pred (C, B, 3).  Multi-image form (x_pos (C, n, 42), idx (C, B)): every candidate is another image's fit
    with its own tables and pixel rows.  -> (C, n, B, multi)"""
    C, n = x_per.shape[:2]
    B = pred.shape[1]
    multi = x_pos.dim() == 3
    assert x_per.is_contiguous() and x_pos.is_contiguous() and pred.is_contiguous()
    assert x_per.shape == (C, n, 20) and x_pos.shape == ((C, n, 42) if multi else (n, 42)) and pred.shape == (C, B, 3)
    if multi:
        assert idx is not None and idx.dtype == torch.int64 and idx.is_contiguous() and idx.shape == (C, B)
    else:
        assert (idx is None and n == B) or (idx is not None and idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == B)
    return C, n, B, multi


def _light_loss_args(loss_args, dpred, C, B):
    """loss_args = (gt (B, 3), latents (C, 6), spline, n_knots, x_scale, loss (C), dlatent (C, 6)): the adaptive robust pixel loss evaluated
    inside the backward launch (dpred unused), or None: dpred (C, B, 3) is the input.  -> the seven, None / 0 for a missing one"""
    if loss_args is None:
        assert dpred.is_contiguous()
        return None, None, None, 0, 0.0, None, None
    gt, lat, spl, nk, xs, loss, dlat = loss_args
    assert gt.shape == (B, 3) and gt.is_contiguous() and lat.shape == (C, 6) and lat.is_contiguous() and dlat.shape == (C, 6) and dlat.is_contiguous()
    assert loss.numel() == C and loss.is_contiguous()
    return loss_args


def _light_adam_state(params, others, lat4, zero):
    """Stacked blobs (C, stride) sharing params' shape and strides, the latents and their moments / gradients (C, 6), the loss words (C)."""
    C = params.shape[0]
    assert all(t.shape == params.shape and t.stride() == params.stride() for t in others) and params.stride(1) == 1
    assert all(t.shape == (C, 6) and t.is_contiguous() for t in lat4) and (zero is None or (zero.numel() == C and zero.is_contiguous()))
    return C


def _part_args(part, loss_cur, C):
    """The two more arguments of the _det Adam launches: the backward blocks' sums part (C, blocks, 8) and the loss words (C) they are added to."""
    assert part.is_contiguous() and part.shape[0] == C and part.shape[2] == 8
    return _p(part), part.shape[1], _p(loss_cur)


def light_pack(desc, params, pack):
    """MFMA-ordered weight copies of C stacked NPP_Net_light blobs (params (C, n) -> pack (C, npp_light_pack_floats()))."""
    n_c = params.shape[0]
    assert params.stride(1) == 1 and pack.stride(1) == 1 and pack.shape[0] == n_c
    _go("npp_light_pack", [C.byref(desc), _p(params), params.stride(0), n_c, _p(pack), pack.stride(0), _stream()])


def light_fwd(desc, params, pack, x_per, x_pos, stash, pred, idx=None):
    """Fused NPP_Net_light forward of C candidates (_light_fwd_inputs) -> pred (C, B, 3), stash (C, rows, B)."""
    n_c, n, B, multi = _light_fwd_inputs(x_per, x_pos, pred, idx)
    assert stash.is_contiguous() and stash.shape[0] == n_c and stash.shape[2] == B
    _go("npp_light_fwd_multi" if multi else "npp_light_fwd",
        [C.byref(desc), _p(params), params.stride(0), _p(pack), pack.stride(0), _p(x_per), _p(x_pos), _p(idx), n, n_c, B, _p(stash), _p(pred), _stream()])


def light_bwd(desc, params, pack, stash, pred, dpred, draw, dstash, loss_args=None):
    """Fused data-gradient chain: dpred (C, B, 3) -> draw (C, B, 3), dstash (C, rows, B); loss_args: _light_loss_args."""
    n_c, B = pred.shape[:2]
    assert all(t.is_contiguous() for t in (stash, pred, draw, dstash)) and dstash.shape[0] == n_c and dstash.shape[2] == B
    gt, lat, spl, nk, xs, loss, dlat = _light_loss_args(loss_args, dpred, n_c, B)
    _go("npp_light_bwd", [C.byref(desc), _p(params), params.stride(0), _p(pack), pack.stride(0), _p(stash), _p(pred), _p(dpred), _p(gt), _p(lat),
                          _p(spl), nk, xs, _p(loss), _p(dlat), n_c, B, _p(draw), _p(dstash), _stream()])


def light_part_blocks(C, B):
    return int(check(lib().npp_light_part_blocks(C, B), "npp_light_part_blocks"))


def light_bwd_det(desc, params, pack, stash, pred, draw, dstash, gt, lat, spline, n_knots, x_scale, part):
    """light_bwd with the adaptive pixel loss folded in, its per-block sums to part (C, light_part_blocks(C, B), 8) by plain stores.
    gt (B, 3) shared, or (C, B, 3): targets per candidate (multi-image form)."""
    n_c, B = pred.shape[:2]
    assert all(t.is_contiguous() for t in (stash, pred, draw, dstash, part, gt, lat)) and part.shape == (n_c, light_part_blocks(n_c, B), 8)
    assert gt.dim() == 2 or gt.shape == (n_c, B, 3)
    _go("npp_light_bwd_det_multi" if gt.dim() == 3 else "npp_light_bwd_det",
        [C.byref(desc), _p(params), params.stride(0), _p(pack), pack.stride(0), _p(stash), _p(pred), _p(gt), _p(lat), _p(spline), n_knots, x_scale,
         _p(part), n_c, B, _p(draw), _p(dstash), _stream()])


def light_adam_pack(desc, params, m, v, grad, n, pack, lat, lat_m, lat_v, dlat, zero, lr, step, b1=0.9, b2=0.999, eps=1e-8, det=()):
    """Adam over C stacked blobs (C, stride) and their latents (C, 6) + gradient / loss-word clear + re-pack, one launch."""
    n_c = _light_adam_state(params, (m, v, grad), (lat, lat_m, lat_v, dlat), zero)
    _go("npp_light_adam_pack_det" if det else "npp_light_adam_pack",
        [C.byref(desc), _p(params), _p(m), _p(v), _p(grad), params.stride(0), n, n_c, _p(pack), pack.stride(0), _p(lat), _p(lat_m), _p(lat_v), _p(dlat),
         _p(zero), lr, b1, b2, eps, step, *det, _stream()])


def light_adam_pack_det(desc, params, m, v, grad, n, pack, lat, lat_m, lat_v, dlat, zero, lr, step, part, loss_cur, b1=0.9, b2=0.999, eps=1e-8):
    """light_adam_pack after light_bwd_det: the blocks' sums are added in block order (latent gradients, loss_cur (C))."""
    light_adam_pack(desc, params, m, v, grad, n, pack, lat, lat_m, lat_v, dlat, zero, lr, step, b1, b2, eps, det=_part_args(part, loss_cur, params.shape[0]))


def light_wgrad(desc, stash, dstash, grad, scratch=None):
    """All seven weight / bias gradients of the C candidates in one launch: grad (C, n) += ... (clear first).
    scratch: light_wgrad_det_scratch(C, B, device) -- the ordered-split form (npp_light_wgrad_det: chip-filling AND bit-reproducible)."""
    n_c, B = stash.shape[0], stash.shape[2]
    assert stash.is_contiguous() and dstash.is_contiguous() and grad.stride(1) == 1 and grad.shape[0] == n_c
    det = [] if scratch is None else [_p(scratch), scratch.numel() * 4]
    _go("npp_light_wgrad_det" if det else "npp_light_wgrad", [C.byref(desc), _p(stash), _p(dstash), n_c, B, _p(grad), grad.stride(0), *det, _stream()])


def light_wgrad_det_scratch(C, B, device):
    """Zeroed scratch of npp_light_wgrad_det for C candidates of B rows (tickets + partial tiles; the tickets reset themselves)."""
    n = int(lib().npp_light_wgrad_det_scratch_bytes(int(C), int(B)))
    return torch.zeros(n // 4, dtype=torch.float32, device=device)


# The 16-bit forms: packs and stashes are byte buffers (C, bytes) uint8.  bind=True: the BoundCall instead of its launch.
def light16_sizes(B):
    """(pack bytes, forward-stash bytes, gradient-stash bytes) per candidate for batches of B rows (a multiple of 64)."""
    L = lib()
    return int(L.npp_light16_pack_bytes()), int(L.npp_light16_stash_bytes(B, 0)), int(L.npp_light16_stash_bytes(B, 1))


def _bytes2d(C, **named):
    for name, t in named.items():
        assert t.dtype == torch.uint8 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 16 == 0 and t.data_ptr() % 16 == 0 and t.shape[0] == C, name


def light16_pack(desc, params, pack):
    """bf16 MFMA-ordered copies (forward + transposed) of C stacked NPP_Net_light blobs: params (C, n) fp32 -> pack (C, bytes) uint8."""
    n_c = params.shape[0]
    _bytes2d(n_c, pack=pack)
    assert params.stride(1) == 1
    _go("npp_light16_pack", [C.byref(desc), _p(params), params.stride(0), n_c, _p(pack), pack.stride(0), _stream()])


def light16_fwd(desc, params, pack, x_per, x_pos, actF, pred, idx=None, bind=False):
    """light_fwd on bf16 operands: pred (C, B, 3) fp32 and the W-format forward stash actF."""
    n_c, n, B, multi = _light_fwd_inputs(x_per, x_pos, pred, idx)
    _bytes2d(n_c, pack=pack, actF=actF)
    return _go("npp_light16_fwd_multi" if multi else "npp_light16_fwd",
               [C.byref(desc), _p(params), params.stride(0), _p(pack), pack.stride(0), _p(x_per), _p(x_pos), _p(idx), n, n_c, B, _p(actF), actF.stride(0),
                _p(pred), _stream()], bind, idx=7)


def light16_bwd(desc, params, pack, actF, pred, dpred, dzF, loss_args=None, bind=False):
    """light_bwd on bf16 operands: the W-format gradient stash dzF; loss_args: _light_loss_args."""
    n_c, B = pred.shape[:2]
    _bytes2d(n_c, pack=pack, actF=actF, dzF=dzF)
    assert pred.is_contiguous()
    gt, lat, spl, nk, xs, loss, dlat = _light_loss_args(loss_args, dpred, n_c, B)
    return _go("npp_light16_bwd", [C.byref(desc), _p(params), params.stride(0), _p(pack), pack.stride(0), _p(actF), actF.stride(0), _p(pred), _p(dpred),
                                   _p(gt), _p(lat), _p(spl), nk, xs, _p(loss), _p(dlat), n_c, B, _p(dzF), dzF.stride(0), _stream()], bind, gt=9, loss=14)


def light16_bwd_det(desc, params, pack, actF, pred, dzF, gt, lat, spline, n_knots, x_scale, part, bind=False):
    """light16_bwd with the pixel loss folded in and the blocks' loss / latent-gradient sums left in part (C, B / 64, 8) by plain stores
    (added in block order by light16_adam_pack_det): bit-reproducible.  gt (B, 3) shared, or (C, B, 3) per candidate (multi-image set)."""
    n_c, B = pred.shape[:2]
    _bytes2d(n_c, pack=pack, actF=actF, dzF=dzF)
    multi = gt.dim() == 3
    assert pred.is_contiguous() and gt.is_contiguous() and gt.shape == ((n_c, B, 3) if multi else (B, 3))
    assert lat.shape == (n_c, 6) and lat.is_contiguous() and part.is_contiguous() and part.shape == (n_c, B // 64, 8) and part.dtype == torch.float32
    return _go("npp_light16_bwd_det", [C.byref(desc), _p(params), params.stride(0), _p(pack), pack.stride(0), _p(actF), actF.stride(0), _p(pred), _p(gt),
                                       3 * B if multi else 0, _p(lat), _p(spline), n_knots, x_scale, _p(part), n_c, B, _p(dzF), dzF.stride(0), _stream()],
               bind, gt=8)


def light16_wgrad(desc, actF, dzF, B, gslabs, bind=False):
    """All seven weight / bias gradients of the C candidates in one launch of the grouped split-K kernel: gslabs (C, ksplit, n) fp32
    receives the ksplit partial sums (plain stores: no clearing needed, bit-reproducible)."""
    n_c, ks, n = gslabs.shape
    assert gslabs.is_contiguous() and gslabs.dtype == torch.float32 and actF.shape[0] == n_c and dzF.shape[0] == n_c
    return _go("npp_light16_wgrad", [C.byref(desc), _p(actF), actF.stride(0), _p(dzF), dzF.stride(0), n_c, B, ks, _p(gslabs), n, ks * n, _stream()], bind)


def light16_adam_pack(desc, params, m, v, n, gslabs, pack, lat, lat_m, lat_v, dlat, zero, lr, step, b1=0.9, b2=0.999, eps=1e-8, bind=False, det=()):
    """Adam over C stacked blobs (gradient = the slabs summed in order) and their latents + loss-word clear + bf16 re-pack, one launch."""
    n_c, ks, ns = gslabs.shape
    _bytes2d(n_c, pack=pack)
    assert _light_adam_state(params, (m, v), (lat, lat_m, lat_v, dlat), zero) == n_c
    return _go("npp_light16_adam_pack_det" if det else "npp_light16_adam_pack",
               [C.byref(desc), _p(params), _p(m), _p(v), params.stride(0), n, n_c, _p(gslabs), ks, ns, ks * ns, _p(pack), pack.stride(0), _p(lat), _p(lat_m),
                _p(lat_v), _p(dlat), _p(zero), lr, b1, b2, eps, step, *det, _stream()], bind, zero=17, lr=18, step=22, loss_cur=25)


def light16_adam_pack_det(desc, params, m, v, n, gslabs, pack, lat, lat_m, lat_v, dlat, zero, lr, step, part, loss_cur, b1=0.9, b2=0.999, eps=1e-8,
                          bind=False):
    """light16_adam_pack after light16_bwd_det: the blocks' sums of `part` added in block order (latent gradients; loss_cur[c] += loss terms)."""
    return light16_adam_pack(desc, params, m, v, n, gslabs, pack, lat, lat_m, lat_v, dlat, zero, lr, step, b1, b2, eps, bind,
                             det=_part_args(part, loss_cur, params.shape[0]))


def act_bwd(dy, zy, act, dz):
    B, n = dy.shape
    check(lib().npp_act_bwd(_p(dy), dy.stride(0), _p(zy), zy.stride(0), B, n, act, _p(dz), dz.stride(0), _stream()), "npp_act_bwd")
    return dz


def act_fwd(x, act, y):
    check(lib().npp_act_fwd(_p(x), x.numel(), act, _p(y), _stream()), "npp_act_fwd")
    return y


LPIPS_PLAIN_SCRATCH = 264               # NPP_LPIPS_PLAIN_SCRATCH_FLOATS (include/npp_hip.h)


def lpips_plain_layer(f0, f1, lin, scale, out, scratch=None):
    """scratch (LPIPS_PLAIN_SCRATCH floats, zeroed once, one per tap launched back to back): the fixed-order, bit-reproducible form.
    The kernel keeps its arrival counter at the fixed slot 256 and leaves it at zero, so a scratch may be re-used by later
    launches of any (N, h, w); it must not be shared by launches that may run concurrently."""
    _req(f0, torch.float32, "f0")
    _req(f1, torch.float32, "f1", f0.shape)
    N, C = f0.shape[:2]
    if scratch is not None:
        assert scratch.dtype == torch.float32 and scratch.numel() >= LPIPS_PLAIN_SCRATCH and scratch.is_contiguous()
        check(lib().npp_lpips_plain_layer_det(_p(f0), _p(f1), N, C, f0.shape[2] * f0.shape[3], _p(lin), scale, _p(out), _p(scratch), _stream()),
              "npp_lpips_plain_layer_det")
        return
    check(lib().npp_lpips_plain_layer(_p(f0), _p(f1), N, C, f0.shape[2] * f0.shape[3], _p(lin), scale, _p(out), _stream()),
          "npp_lpips_plain_layer")


# ---- around the AlexNet convolutions (segmentation criterion, proposal conv1 features): include/npp_hip.h "f3 / f4 front ends" ----
def im2col(x, k, stride, pad, nhwc=False):
    """Rows (n, oy, ox) x columns (c, ky, kx) of a k x k / stride / zero-pad convolution over x: (N,C,H,W), or (N,H,W,C) with nhwc."""
    _req(x, torch.float32, "x")
    if nhwc:
        N, H, W, Cc = x.shape
    else:
        N, Cc, H, W = x.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = torch.empty((N * ho * wo, Cc * k * k), dtype=torch.float32, device=x.device)
    check(lib().npp_im2col(_p(x), N, Cc, H, W, k, stride, pad, 1 if nhwc else 0, _p(cols), _stream()), "npp_im2col")
    return cols, ho, wo


def maxpool_nhwc(x, k, stride):
    _req(x, torch.float32, "x")
    N, H, W, Cc = x.shape
    y = torch.empty((N, (H - k) // stride + 1, (W - k) // stride + 1, Cc), dtype=torch.float32, device=x.device)
    check(lib().npp_maxpool_nhwc(_p(x), N, H, W, Cc, k, stride, _p(y), _stream()), "npp_maxpool_nhwc")
    return y


def lpips_spatial_layer(f0, f1, lin):
    """(N,h,w,C) position-major features of the two images -> the tap's distance map (N,h,w) (lpips.py:99-110, spatial, plain head)."""
    _req(f0, torch.float32, "f0")
    _req(f1, torch.float32, "f1", f0.shape)
    _req(lin, torch.float32, "lin", (f0.shape[-1],))
    d = torch.empty(f0.shape[:-1], dtype=torch.float32, device=f0.device)
    check(lib().npp_lpips_spatial_layer(_p(f0), _p(f1), d.numel(), f0.shape[-1], _p(lin), _p(d), _stream()), "npp_lpips_spatial_layer")
    return d


def resize_bilinear(x, H, W, out=None, accumulate=False):
    """F.interpolate(x[:, None], size=(H, W), mode='bilinear', align_corners=False)[:, 0] of maps (N,h,w); accumulate: out += it."""
    _req(x, torch.float32, "x")
    N, h, w = x.shape
    if out is None:
        assert not accumulate
        out = torch.empty((N, H, W), dtype=torch.float32, device=x.device)
    else:
        _req(out, torch.float32, "out", (N, H, W))
    check(lib().npp_resize_bilinear(_p(x), N, h, w, H, W, 1 if accumulate else 0, _p(out), _stream()), "npp_resize_bilinear")
    return out


# ---- segmentation task: the per-pixel half of the initial coarse segmentation (include/npp_hip.h npp_slic_*) ---------------
# Scratch is allocated per call (torch's caching allocator hands the block back): nothing is kept between two image shapes.
def slic_prepare(img_u8, vmin, vmax, m):
    """(H,W,3) uint8 RGB -> (3,H,W) fp32 CIELAB / m of the min-max scaled, sigma = 1 blurred image (what SLIC clusters)."""
    _req(img_u8, torch.uint8, "img_u8")
    H, W, ch = img_u8.shape
    if ch != 3:
        raise ValueError("img_u8: expected (H, W, 3)")
    tmp = torch.empty((3, H, W), dtype=torch.float32, device=img_u8.device)
    lab = torch.empty((3, H, W), dtype=torch.float32, device=img_u8.device)
    check(lib().npp_slic_prepare(_p(img_u8), H, W, float(vmin), float(vmax), float(m), _p(tmp), _p(lab), _stream()), "npp_slic_prepare")
    return lab


def slic_assign(lab, mask_u8, centres, S, labels=None):
    """lab (3,H,W) fp32, mask (H,W) uint8, centres (K,5) fp32 rows (y, x, L, a, b), step S -> labels (H,W) int32: 0 outside the mask,
    k + 1 for centre k."""
    _req(lab, torch.float32, "lab")
    H, W = lab.shape[1:]
    _req(mask_u8, torch.uint8, "mask_u8", (H, W))
    _req(centres, torch.float32, "centres", (centres.shape[0], 5))
    if labels is None:
        labels = torch.empty((H, W), dtype=torch.int32, device=lab.device)
    else:
        _req(labels, torch.int32, "labels", (H, W))
    check(lib().npp_slic_assign(_p(lab), _p(mask_u8), H, W, _p(centres), centres.shape[0], float(S), _p(labels), _stream()), "npp_slic_assign")
    return labels


def slic_update(lab, labels, centres):
    """In place: every centre becomes the mean (y, x, L, a, b) of the pixels labelled k + 1; a centre without members is kept."""
    _req(lab, torch.float32, "lab")
    H, W = lab.shape[1:]
    _req(labels, torch.int32, "labels", (H, W))
    _req(centres, torch.float32, "centres", (centres.shape[0], 5))
    K = centres.shape[0]
    nbytes = check(lib().npp_slic_update_scratch_bytes(K), "npp_slic_update_scratch_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=lab.device)
    check(lib().npp_slic_update(_p(lab), _p(labels), H, W, _p(centres), K, _p(ws), int(nbytes), _stream()), "npp_slic_update")
    return centres


def slic_features(img_u8, labels, N):
    """Per superpixel 1..N of an (H,W) int32 label image over an (H,W,3) uint8 image -> count (N,) int32 and (N,11) fp32 rows:
    centroid (y, x), mean x 3, median x 3, meanGrad x 3 (NaN for a label without pixels)."""
    _req(img_u8, torch.uint8, "img_u8")
    H, W = img_u8.shape[:2]
    _req(labels, torch.int32, "labels", (H, W))
    N = int(N)
    nbytes = check(lib().npp_slic_features_scratch_bytes(N), "npp_slic_features_scratch_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=img_u8.device)
    count = torch.empty(N, dtype=torch.int32, device=img_u8.device)
    feat = torch.empty((N, 11), dtype=torch.float32, device=img_u8.device)
    check(lib().npp_slic_features(_p(img_u8), _p(labels), H, W, N, _p(count), _p(feat), _p(ws), int(nbytes), _stream()), "npp_slic_features")
    return count, feat


# ---- remapping task: blur detection (include/npp_hip.h npp_rgb_to_gray_u8 / npp_blur_sv_share / npp_binary_morph) --------------
def rgb_to_gray_u8(img_u8):
    """(H,W,3) uint8 RGB -> (H,W) uint8 gray, OpenCV's 14-bit fixed point (== io.rgb_to_gray_u8, bit for bit)."""
    _req(img_u8, torch.uint8, "img_u8")
    if img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError("img_u8: expected (H, W, 3)")
    H, W = img_u8.shape[:2]
    gray = torch.empty((H, W), dtype=torch.uint8, device=img_u8.device)
    check(lib().npp_rgb_to_gray_u8(_p(img_u8), H, W, _p(gray), _stream()), "npp_rgb_to_gray_u8")
    return gray


def blur_sv_share(gray_u8, sv_num=3):
    """(H,W) uint8 gray -> (H,W) float64: the share of the `sv_num` largest singular values of the 20 x 20 block around every pixel
    (blur_detection.py:32-46, window 10, the reference's own border index map)."""
    _req(gray_u8, torch.uint8, "gray_u8")
    if gray_u8.dim() != 2:
        raise ValueError("gray_u8: expected (H, W)")
    H, W = gray_u8.shape
    out = torch.empty((H, W), dtype=torch.float64, device=gray_u8.device)
    check(lib().npp_blur_sv_share(_p(gray_u8), H, W, int(sv_num), _p(out), _stream()), "npp_blur_sv_share")
    return out


def binary_morph(mask_u8, iterations, dilate):
    """(H,W) uint8 (non-zero = set) -> (H,W) uint8 0 / 1: scipy.ndimage.binary_dilation (dilate) or binary_erosion with their
    defaults (4-connected cross, border_value 0) after `iterations` rounds.  The scratch is allocated per call."""
    _req(mask_u8, torch.uint8, "mask_u8")
    if mask_u8.dim() != 2:
        raise ValueError("mask_u8: expected (H, W)")
    H, W = mask_u8.shape
    tmp = torch.empty((H, W), dtype=torch.uint8, device=mask_u8.device)
    out = torch.empty((H, W), dtype=torch.uint8, device=mask_u8.device)
    check(lib().npp_binary_morph(_p(mask_u8), H, W, int(iterations), int(bool(dilate)), _p(tmp), _p(out), _stream()), "npp_binary_morph")
    return out


# ---- completion task: the image work in front of the periodicity search (include/npp_hip.h npp_resize_* .. npp_far_points;
# frontend.py is the public face).  Device tensors in, device tensors out; scratch is allocated per call.
FAR_POINTS_SCRATCH_BYTES, FAR_POINTS_MAX_TOPK, EDT_MAX_DIM = 2048, 16, 32767


def _req_hw(t, dtype, name):
    _req(t, dtype, name)
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty (H, W)")
    return t.shape


def _req_chw(t, dtype, name):
    _req(t, dtype, name)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty (C, h, w)")
    return t.shape


def _resize_u8(entry, img_u8, dsize):
    H, W = _req_hw(img_u8, torch.uint8, "img_u8")
    w, h = int(dsize[0]), int(dsize[1])
    if h < 1 or w < 1:
        raise ValueError(f"dsize: expected (w, h) >= 1, got {tuple(dsize)}")
    out = torch.empty((h, w), dtype=torch.uint8, device=img_u8.device)
    check(getattr(lib(), entry)(_p(img_u8), H, W, _p(out), h, w, _stream()), entry)
    return out


def resize_nearest_u8(img_u8, dsize):
    """(H,W) uint8 -> (h,w) uint8, dsize = (w, h): cv2.resize INTER_NEAREST (== cvlite.resize_nearest, bit for bit)."""
    return _resize_u8("npp_resize_nearest_u8", img_u8, dsize)


def resize_linear_u8(img_u8, dsize):
    """(H,W) uint8 -> (h,w) uint8, dsize = (w, h): cv2.resize INTER_LINEAR on uint8 (== cvlite.resize_linear_u8, bit for bit)."""
    return _resize_u8("npp_resize_linear_u8", img_u8, dsize)


def normalize_u8(act):
    """(C,h,w) fp32 -> (C,h,w) uint8: per channel uint8((a - min) / (max - min) * 255) in float64, zeros for a constant channel
    (== cvlite.normalize_to_uint8(channel_idx=(1, 2)))."""
    C_, h, w = _req_chw(act, torch.float32, "act")
    out = torch.empty((C_, h, w), dtype=torch.uint8, device=act.device)
    check(lib().npp_normalize_u8(_p(act), C_, h, w, _p(out), _stream()), "npp_normalize_u8")
    return out


def gaussian_blur3_u8(img_u8):
    """(C,h,w) uint8 -> (C,h,w) uint8: cv2.GaussianBlur((3, 3), 0) per channel (== cvlite.gaussian_blur3_u8)."""
    C_, h, w = _req_chw(img_u8, torch.uint8, "img_u8")
    out = torch.empty_like(img_u8)
    check(lib().npp_gaussian_blur3_u8(_p(img_u8), C_, h, w, _p(out), _stream()), "npp_gaussian_blur3_u8")
    return out


def canny_mark(img_u8, low, high):
    """(C,h,w) uint8 -> (C,h,w) uint8 in {0, 1 weak, 2 strong}: cvlite.canny_u8 up to the hysteresis, thresholds already floored."""
    C_, h, w = _req_chw(img_u8, torch.uint8, "img_u8")
    out = torch.empty_like(img_u8)
    check(lib().npp_canny_mark(_p(img_u8), C_, h, w, int(low), int(high), _p(out), _stream()), "npp_canny_mark")
    return out


def canny_hysteresis(marks, rounds=8):
    """`rounds` hysteresis rounds on a canny_mark map, in place -> (rounds,) int32 device flags, flag r = round r marked a pixel."""
    C_, h, w = _req_chw(marks, torch.uint8, "marks")
    flags = torch.empty(int(rounds), dtype=torch.int32, device=marks.device)
    check(lib().npp_canny_hysteresis(_p(marks), C_, h, w, int(rounds), _p(flags), _stream()), "npp_canny_hysteresis")
    return flags


def canny_finish(marks):
    """Marks (C,h,w) -> uint8 {0, 255}: 255 where the mark is 2."""
    C_, h, w = _req_chw(marks, torch.uint8, "marks")
    out = torch.empty_like(marks)
    check(lib().npp_canny_finish(_p(marks), C_, h, w, _p(out), _stream()), "npp_canny_finish")
    return out


def edge_count(marks, eroded_u8):
    """Marks (C,h,w) after the hysteresis, eroded mask (h,w) uint8 -> (h,w) fp32: channels marked 2 per pixel inside the mask."""
    C_, h, w = _req_chw(marks, torch.uint8, "marks")
    _req(eroded_u8, torch.uint8, "eroded_u8", (h, w))
    out = torch.empty((h, w), dtype=torch.float32, device=marks.device)
    check(lib().npp_edge_count(_p(marks), C_, h, w, _p(eroded_u8), _p(out), _stream()), "npp_edge_count")
    return out


def edt_sq(mask_u8):
    """(H,W) uint8 -> (H,W) int32: exact squared Euclidean distance to the nearest zero pixel (the caller has checked there is one)."""
    H, W = _req_hw(mask_u8, torch.uint8, "mask_u8")
    tmp = torch.empty((H, W), dtype=torch.int32, device=mask_u8.device)
    out = torch.empty((H, W), dtype=torch.int32, device=mask_u8.device)
    check(lib().npp_edt_sq(_p(mask_u8), H, W, _p(tmp), _p(out), _stream()), "npp_edt_sq")
    return out


def far_points(dsq, topk, n_min):
    """Squared distances (H,W) int32 -> (2 + 2 topk,) int32 device record [count, 0, (index, d^2) ...]: the greedy far-point walk,
    largest d^2 first, ties by smallest row-major index, accepted pixels >= n_min (squared) apart."""
    H, W = _req_hw(dsq, torch.int32, "dsq")
    scratch = torch.empty(FAR_POINTS_SCRATCH_BYTES // 8, dtype=torch.int64, device=dsq.device)
    rec = torch.empty(2 + 2 * int(topk), dtype=torch.int32, device=dsq.device)
    check(lib().npp_far_points(_p(dsq), H, W, int(topk), int(n_min), _p(scratch), _p(rec), _stream()), "npp_far_points")
    return rec


# ---- segmentation task: 4-connected components (include/npp_hip.h npp_cc_*; regions.py is the public face) ----------------------
# Device tensors in, device tensors out; the *_host forms take and return NumPy arrays and never touch a GPU.  Scratch is allocated
# per call and needs no initial content.
CC_MAX_CHANNELS = 4


def cc_label(labels):
    """(H,W) int32 label image (0 = outside) -> (H,W) int32 roots: -1 outside, else the smallest row-major index of the pixel's
    4-connected component of equal labels."""
    _req(labels, torch.int32, "labels")
    if labels.dim() != 2:
        raise ValueError("labels: expected (H, W)")
    H, W = labels.shape
    root = torch.empty((H, W), dtype=torch.int32, device=labels.device)
    check(lib().npp_cc_label(_p(labels), H, W, _p(root), _stream()), "npp_cc_label")
    return root


def cc_number(root):
    """Roots (H,W) int32 -> (numbered (H,W) int32: 1..C in raster order of first appearance, 0 outside; C as a one-word int32 device
    tensor)."""
    _req(root, torch.int32, "root")
    if root.dim() != 2:
        raise ValueError("root: expected (H, W)")
    H, W = root.shape
    nbytes = check(lib().npp_cc_number_scratch_bytes(H, W), "npp_cc_number_scratch_bytes")
    ws = torch.empty(int(nbytes) // 4, dtype=torch.int32, device=root.device)
    numbered = torch.empty((H, W), dtype=torch.int32, device=root.device)
    count = torch.empty(1, dtype=torch.int32, device=root.device)
    check(lib().npp_cc_number(_p(root), H, W, _p(numbered), _p(count), _p(ws), int(nbytes), _stream()), "npp_cc_number")
    return numbered, count


def cc_stats(numbered, C_, values_u8=None):
    """Per component 1..C_ of a numbered (H,W) int32 image -> sizes (C,) int64, sums (C,nch) int64 of the (H,W,nch) uint8 image
    `values_u8` (None: nch = 0), border (C,) uint8 (1 = touches the image border), boxes (C,4) int32 (y0, x0, y1, x1 inclusive)."""
    _req(numbered, torch.int32, "numbered")
    if numbered.dim() != 2:
        raise ValueError("numbered: expected (H, W)")
    H, W = numbered.shape
    nch = 0
    if values_u8 is not None:
        _req(values_u8, torch.uint8, "values_u8")
        if values_u8.dim() != 3 or tuple(values_u8.shape[:2]) != (H, W) or not 1 <= values_u8.shape[2] <= CC_MAX_CHANNELS:
            raise ValueError(f"values_u8: expected ({H}, {W}, 1..{CC_MAX_CHANNELS}), got {tuple(values_u8.shape)}")
        nch = int(values_u8.shape[2])
    C_ = int(C_)
    dev = numbered.device
    size = torch.empty(C_, dtype=torch.int64, device=dev)
    sums = torch.empty((C_, nch), dtype=torch.int64, device=dev)
    border = torch.empty(C_, dtype=torch.uint8, device=dev)
    box = torch.empty((C_, 4), dtype=torch.int32, device=dev)
    check(lib().npp_cc_stats(_p(numbered), H, W, C_, _p(values_u8), nch, _p(size), _p(sums), _p(border), _p(box), _stream()), "npp_cc_stats")
    return size, sums, border, box


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


def cc_label_host(labels):
    """cc_label on a NumPy (H,W) int32 array, by the library's host twin."""
    labels = np.ascontiguousarray(labels, np.int32)
    if labels.ndim != 2:
        raise ValueError("labels: expected (H, W)")
    root = np.empty(labels.shape, np.int32)
    check(lib().npp_cc_label_host(_np_ptr(labels), labels.shape[0], labels.shape[1], _np_ptr(root)), "npp_cc_label_host")
    return root


def cc_number_host(root):
    """cc_number on a NumPy array -> (numbered (H,W) int32, C int)."""
    root = np.ascontiguousarray(root, np.int32)
    if root.ndim != 2:
        raise ValueError("root: expected (H, W)")
    numbered = np.empty(root.shape, np.int32)
    count = np.zeros(1, np.int32)
    check(lib().npp_cc_number_host(_np_ptr(root), root.shape[0], root.shape[1], _np_ptr(numbered), _np_ptr(count)), "npp_cc_number_host")
    return numbered, int(count[0])


def cc_stats_host(numbered, C_, values_u8=None):
    """cc_stats on NumPy arrays."""
    numbered = np.ascontiguousarray(numbered, np.int32)
    if numbered.ndim != 2:
        raise ValueError("numbered: expected (H, W)")
    H, W = numbered.shape
    nch = 0
    if values_u8 is not None:
        values_u8 = np.asarray(values_u8)
        if values_u8.dtype != np.uint8 or values_u8.ndim != 3 or values_u8.shape[:2] != (H, W) or not 1 <= values_u8.shape[2] <= CC_MAX_CHANNELS:
            raise ValueError(f"values_u8: expected a uint8 ({H}, {W}, 1..{CC_MAX_CHANNELS}) array")
        values_u8 = np.ascontiguousarray(values_u8)
        nch = int(values_u8.shape[2])
    C_ = int(C_)
    size, sums = np.empty(C_, np.int64), np.empty((C_, nch), np.int64)
    border, box = np.empty(C_, np.uint8), np.empty((C_, 4), np.int32)
    check(lib().npp_cc_stats_host(_np_ptr(numbered), H, W, C_, _np_ptr(values_u8) if nch else None, nch, _np_ptr(size), _np_ptr(sums),
                                  _np_ptr(border), _np_ptr(box)), "npp_cc_stats_host")
    return size, sums, border, box


# ---- quality report (include/npp_hip.h npp_ssim_map / npp_region_sums) ----------------------------------------------------------
SSIM_WIN = 11           # window taps per axis; the map is (H - 10, W - 10)


def _req_img_pair(a, b):
    _req(a, torch.float32, "a")
    if a.dim() != 3 or a.shape[2] != 3:
        raise ValueError("a: expected (H, W, 3)")
    _req(b, torch.float32, "b", a.shape)
    return int(a.shape[0]), int(a.shape[1])


def ssim_map(a, b):
    """Two (H,W,3) fp32 images in [0, 1] -> (H-10, W-10) float64: the SSIM index (11 x 11 Gaussian window, sigma 1.5, K1 0.01, K2 0.03,
    data range 1), channel mean, at the pixels whose whole window lies inside.  ValueError (from the launcher's own argument check;
    nothing is launched) when H or W is below 11."""
    H, W = _req_img_pair(a, b)
    out = torch.empty((max(H - SSIM_WIN + 1, 0), max(W - SSIM_WIN + 1, 0)), dtype=torch.float64, device=a.device)
    rc = lib().npp_ssim_map(_p(a), _p(b), H, W, _p(out), _stream())
    if rc < 0 and (H < SSIM_WIN or W < SSIM_WIN):
        raise ValueError(lib().npp_last_error_string().decode())
    check(rc, "npp_ssim_map")
    return out


def region_sums(a, b, weight, smap=None):
    """Per-block partial sums (blocks, 5) float64 of one (H,W) fp32 weight mask over two (H,W,3) fp32 images: weights, weighted squared
    and absolute error over the channels, and -- with `smap`, the (H-10, W-10) map of ssim_map -- the weights of the pixels the map
    covers and the weighted map.  Fixed block count and order: the caller's sum over the blocks is bit-reproducible."""
    H, W = _req_img_pair(a, b)
    _req(weight, torch.float32, "weight", (H, W))
    if smap is not None:
        _req(smap, torch.float64, "smap", (H - SSIM_WIN + 1, W - SSIM_WIN + 1))
    nb = check(lib().npp_region_sums_blocks(H, W), "npp_region_sums_blocks")
    part = torch.empty((nb, 5), dtype=torch.float64, device=a.device)
    check(lib().npp_region_sums(_p(a), _p(b), _p(weight), _p(smap), H, W, _p(part), _stream()), "npp_region_sums")
    return part


# ---- quality report: LPIPS of whole images (include/npp_hip.h npp_lpips_tap_map / npp_lpips_compose / npp_map_region_sums) -----
LPIPS_LAYOUTS = {"nchw": 0, "nhwc": 1, "nchw_lane": 2, "nchw_split": 3}      # NPP_LPIPS_*


def lpips_tap_map(f0, f1, lin, layout="nchw"):
    """One tap's distance map (h, w) float64 from the fp32 features of the two images -- (C, h, w) for the "nchw" layouts ("nchw": the
    launcher picks one lane per position or split channels by the number of positions; "nchw_lane" / "nchw_split" ask for one), (h, w,
    C) for "nhwc" -- and the tap's lin vector (C,) (lpips.py:104-119, plain head, before the upsampling)."""
    _req(f0, torch.float32, "f0")
    if f0.dim() != 3:
        raise ValueError("f0: expected the features of one image, (C, h, w) or (h, w, C)")
    _req(f1, torch.float32, "f1", f0.shape)
    if layout not in LPIPS_LAYOUTS:
        raise ValueError(f"layout: one of {sorted(LPIPS_LAYOUTS)}, got {layout!r}")
    (h, w, Cc) = f0.shape if layout == "nhwc" else (f0.shape[1], f0.shape[2], f0.shape[0])
    _req(lin, torch.float32, "lin", (Cc,))
    d = torch.empty((h, w), dtype=torch.float64, device=f0.device)
    check(lib().npp_lpips_tap_map(_p(f0), _p(f1), Cc, h, w, LPIPS_LAYOUTS[layout], _p(lin), _p(d), _stream()), "npp_lpips_tap_map")
    return d


def lpips_compose(maps, H, W):
    """The (H, W) float64 distance map of LPIPS(spatial=True): the taps' maps [(h_k, w_k) float64] resized bilinearly
    (align_corners=False) and summed in tap order, one launch (lpips.py:117, :126-128)."""
    for k, m in enumerate(maps):
        _req(m, torch.float64, f"maps[{k}]")
        if m.dim() != 2:
            raise ValueError(f"maps[{k}]: expected (h, w)")
    n = len(maps)
    ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in maps])
    hs, ws = (C.c_int32 * n)(*[m.shape[0] for m in maps]), (C.c_int32 * n)(*[m.shape[1] for m in maps])
    out = torch.empty((int(H), int(W)), dtype=torch.float64, device=maps[0].device)
    check(lib().npp_lpips_compose(ptrs, hs, ws, n, int(H), int(W), _p(out), _stream()), "npp_lpips_compose")
    return out


def map_region_sums(dmap, weight=None):
    """Per-block partial sums (blocks, 2) float64 -- the weights and the weighted map -- of an (H, W) float64 map under an (H, W) fp32
    weight mask (None: all ones).  Fixed block count and order, like region_sums."""
    _req(dmap, torch.float64, "dmap")
    if dmap.dim() != 2:
        raise ValueError("dmap: expected (H, W)")
    H, W = int(dmap.shape[0]), int(dmap.shape[1])
    if weight is not None:
        _req(weight, torch.float32, "weight", (H, W))
    nb = check(lib().npp_map_region_sums_blocks(H, W), "npp_map_region_sums_blocks")
    part = torch.empty((nb, 2), dtype=torch.float64, device=dmap.device)
    check(lib().npp_map_region_sums(_p(dmap), _p(weight), H, W, _p(part), _stream()), "npp_map_region_sums")
    return part


# ---- remapping variant: Gram-matrix style loss pieces (models/style_loss.py:37-74) ----------------------------
_gram_ws = {}


def gram_fwd(f):
    """Gram matrices (N, C, C) of features (N, C, h, w) (models/style_loss.py:55-58).  ops.DETERMINISTIC: the ordered-split form
    (npp_gram_fwd_det) over a zeroed per-stream scratch."""
    _req(f, torch.float32, "f")
    N, Cc = f.shape[:2]
    hw = f.shape[2] * f.shape[3]
    g = torch.empty((N, Cc, Cc), dtype=torch.float32, device=f.device)
    if DETERMINISTIC:
        key = (f.device, N, Cc, hw, _stream().value)
        ws = _gram_ws.get(key)
        if ws is None:
            ws = _gram_ws[key] = torch.zeros(int(lib().npp_gram_fwd_det_scratch_bytes(N, Cc, hw)) // 4, dtype=torch.float32, device=f.device)
        check(lib().npp_gram_fwd_det(_p(f), N, Cc, hw, _p(g), _p(ws), ws.numel() * 4, _stream()), "npp_gram_fwd_det")
        return g
    check(lib().npp_gram_fwd(_p(f), N, Cc, hw, _p(g), _stream()), "npp_gram_fwd")
    return g


def gram_bwd(dg, f):
    df = torch.empty_like(f)
    N, Cc = f.shape[:2]
    check(lib().npp_gram_bwd(_p(dg), _p(f), N, Cc, f.shape[2] * f.shape[3], _p(df), _stream()), "npp_gram_bwd")
    return df


_re_ws = {}


def robust_elem(a, b, latents, spline, n_knots, x_scale, coef_n, loss, want_grad=True, dlatent=None):
    """per-element adaptive robust NLL of (a - b) over (N, D); returns d(loss)/d(a) (N, D) or None."""
    N, D = a.shape
    key = (a.device, D, _stream().value)                 # (it holds the launch's partial sums and arrival ticket: one per stream)
    ws = _re_ws.get(key)
    if ws is None:
        ws = _re_ws[key] = torch.empty(int(lib().npp_robust_elem_workspace_bytes(D)), dtype=torch.uint8, device=a.device)
    diff = torch.empty_like(a)
    dd = torch.empty_like(a) if want_grad else None
    cf = (C.c_float * N)(*[float(v) for v in coef_n])
    check(lib().npp_robust_elem(_p(a), _p(b), N, D, _p(latents), _p(spline), n_knots, x_scale, cf, _p(loss), _p(diff), _p(dd),
                                _p(dlatent) if want_grad else None, _p(ws), _stream()), "npp_robust_elem")
    return dd


# ---- stacked launches (include/npp_hip.h "stacked launches"): M images per launch -----------------------------------------
def embed_dev_blob(cfgs, device):
    """The fused kernels' embedder constants of M images as one device blob (npp_embed_dev_build per image)."""
    nb = lib().npp_embed_dev_bytes()
    host = np.zeros((len(cfgs), nb), np.uint8)
    for i, cfg in enumerate(cfgs):
        check(lib().npp_embed_dev_build(C.byref(cfg), host[i].ctypes.data_as(C.c_void_p)), "npp_embed_dev_build")
    return torch.from_numpy(host).to(device)


def mlp_fwd_stack(coords, edev, M, K, wf, params, pred, actF, it, width=NPP_WIDTH):
    """coords (M,Bp,2) int32, wf (M, pack bytes) uint8, params (M, stride) fp32, pred (M,Bp,3), actF (M, bytes) uint8."""
    _req(coords, torch.int32, "coords")
    Bp = coords.shape[1]
    check(lib(width).npp_mlp_fwd_stack(_p(coords), Bp, _p(edev), M, K, width, _p(wf), wf.stride(0), _p(params), params.stride(0), _p(pred),
                                       _p(actF), actF.stride(0), _p(it), _stream()), "npp_mlp_fwd_stack", width)


def trunk_patch_in_loss_stack(pred, row0, crops, cmasks, M, n_p, P, X, N_total, scale, shift, x0, xy, zero, it, loss, gt_stride,
                              lat_stride, loss_stride):
    from ._lib import PixelLossArgs
    s = (C.c_float * 3)(*[float(v) for v in scale])
    b = (C.c_float * 3)(*[float(v) for v in shift])
    pr, gt, mask, latents, spline, n_knots, x_scale, weight, loss_buf, dpred, dlatent, n_rows, scratch = loss[:13]
    la = PixelLossArgs(pr.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), int(n_rows), latents.data_ptr(),
                       spline.data_ptr(), int(n_knots), float(x_scale), float(weight), loss_buf.data_ptr(), dpred.data_ptr(),
                       dlatent.data_ptr(), scratch.data_ptr(), float(loss[13]) if len(loss) > 13 else 0.0)
    check(lib().npp_trunk_patch_in_loss_stack(_p(pred), pred.shape[1], row0, _p(crops), crops.stride(0), _p(cmasks), cmasks.stride(0), M,
                                              n_p, P, X, N_total, s, b, _p(x0), _p(xy), 0 if xy is None else xy.stride(0), _p(zero),
                                              _p(it), C.byref(la), gt_stride, lat_stride, loss_stride, scratch.stride(0), _stream()),
          "npp_trunk_patch_in_loss_stack")


def cx_fwd_bwd_groups(fx, fy, it, M, band_width, scale, loss, loss_stride=1):
    """npp_cx_fwd_bwd over sample groups (one per image of a stack): fx / fy (X, C, h, w); loss (M * loss_stride,) accumulated."""
    N, Cc, hw, ws, nbytes, st = _cx_intake(fx, fy)
    dfx = torch.empty_like(fx)
    check(lib().npp_cx_fwd_bwd_groups(_p(fx), _p(fy), N, Cc, hw, band_width, scale, _p(loss), loss_stride, _p(dfx), _p(it), M, _p(ws),
                                      int(nbytes), st), "npp_cx_fwd_bwd_groups")
    return dfx


def cx_fwd_bwd_flat(fx, fy, yact, dz, N_total, band_width, scale, loss, loss_stride=1, it=None, M=0):
    """The contextual core with dL/dx written straight into the trunk's flat bf16 gradient tensor dz, gated by [yact > 0] (yact: the
    tapped layer's flat fp16 output; both of geometry N_total x C x H x W) -- no fp32 gradient tensor, no npp_trunk_grad_in launch.
    it / M: sample groups of a stacked launch (cx_fwd_bwd_groups)."""
    N, Cc, _, ws, nbytes, st = _cx_intake(fx, fy)
    H, W = fx.shape[2:]
    key2 = (fx.device, "dxh", N * Cc * H * W, st.value)
    dxh = _cx_ws.get(key2)
    if dxh is None:
        dxh = _cx_ws[key2] = torch.empty(N * Cc * H * W, dtype=torch.float32, device=fx.device)
    check(lib().npp_cx_fwd_bwd_flat(_p(fx), _p(fy), N, Cc, H, W, band_width, scale, _p(loss), loss_stride, _p(dxh), _p(yact), _p(dz),
                                    N_total, _p(it), M, _p(ws), int(nbytes), st), "npp_cx_fwd_bwd_flat")


def mlp_bwd_patch_stack(dpred, pred, M, K, wb, params, actF, dzF, dx_a, dx_b, cmasks, row0, n_p, P, it, width=NPP_WIDTH):
    check(lib(width).npp_mlp_bwd_patch_stack(_p(dpred), _p(pred), pred.shape[1], M, K, width, _p(wb), wb.stride(0), _p(params),
                                             params.stride(0), _p(actF), actF.stride(0), _p(dzF), dzF.stride(0), _p(dx_a), _p(dx_b),
                                             0 if dx_b is None else dx_b.stride(0), _p(cmasks), cmasks.stride(0), row0, n_p, P, _p(it),
                                             _stream()), "npp_mlp_bwd_patch_stack", width)


def mlp_wgrad_stack(dzF, actF, Bp, M, K, ksplit, gslabs, it, width=NPP_WIDTH):
    check(lib(width).npp_mlp_wgrad_stack(_p(dzF), dzF.stride(0), _p(actF), actF.stride(0), Bp, M, K, width, ksplit, _p(gslabs),
                                         gslabs.stride(0), _p(it), _stream()), "npp_mlp_wgrad_stack", width)


def adam_step_net_pack_stack(p, m, v, n, gslabs, n_slabs, slab_stride, lat, lat_m, lat_v, dlat, n_lat, zero, M, K, wf, wb, it,
                             pl_partials, loss_cur, width=NPP_WIDTH, b1=0.9, b2=0.999, eps=1e-8):
    """p / m / v (M, stride) blobs, gslabs (M, n_slabs * slab_stride), lat.. (M, >= n_lat), zero (M, n_zero): image m's idle accumulators."""
    check(lib(width).npp_adam_step_net_pack_stack(_p(p), _p(m), _p(v), p.stride(0), _p(gslabs), n, n_slabs, slab_stride, gslabs.stride(0),
                                                  _p(lat), _p(lat_m), _p(lat_v), _p(dlat), n_lat, lat.stride(0), _p(zero),
                                                  zero.shape[1], zero.stride(0), b1, b2, eps, M, K, width, _p(wf), wf.stride(0), _p(wb),
                                                  wb.stride(0), _p(pl_partials), pl_partials.stride(0), _p(loss_cur), _p(it), _stream()),
          "npp_adam_step_net_pack_stack", width)
