"""Host-side mirror of the reference's model plumbing for the hot path:
create_npp_net (models/helpers.py:75-175), render (:41-62), the Adam + LR rule of
NPP_completion/train.py:253-263, with the state kept in device buffers that the HIP
kernels read directly.  Nothing here computes; it owns memory and calls the C ABI."""
import os

import numpy as np
import torch

from . import ops
from ._lib import EmbedCfg, param_layout, NPP_E, NPP_WIDTH

LATENT_ALPHA_INIT = 2.3841858e-07   # logit(0.5) in fp32 (robust_loss_pytorch/util.py:75-83)


def _pair(v):
    """One number or a pair -> (float, float)."""
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 2)
    if a.size != 2:
        raise ValueError(f"expected one number or a pair, got {v!r}")
    return float(a[0]), float(a[1])


def _pixel_coords(coords):
    """render() / render_fp32() take pixel indices; positions go through render_at()."""
    if not (isinstance(coords, torch.Tensor) and coords.dtype == torch.int32):
        raise TypeError(f"coords: expected an int32 tensor, got {getattr(coords, 'dtype', type(coords))}")
    return coords


def canvas_coords(size, origin=(0.0, 0.0), scale=(1.0, 1.0), start=0, n=None):
    """The fit-frame positions of canvas pixels [start, start + n) (row-major) of a size = (H', W') canvas, (n, 2) float32 [y, x]:
    y = y0 + i / sy, x = x0 + j / sx as the grid launches form them -- an IEEE fp32 quotient, then a separate fp32 add.  So
    NPPNet.render_at(canvas_coords(...)) is render_grid(...) bit for bit, and at an integer scale S the positions of pixels
    (S i, S j) are the integers (y0 + i, x0 + j) exactly."""
    Hc, Wc = (int(s) for s in size)
    n = Hc * Wc - int(start) if n is None else int(n)
    p = np.arange(int(start), int(start) + n, dtype=np.int64)
    sy, sx = (np.float32(s) for s in _pair(scale))
    y0, x0 = (np.float32(o) for o in _pair(origin))
    y = y0 + (p // Wc).astype(np.float32) / sy
    x = x0 + (p % Wc).astype(np.float32) / sx
    return np.stack([y, x], 1).astype(np.float32)


class NPPNet:
    """NPP_Net (K>1) / NPP_Net_top1 (K==1) with its embedders, optimiser state and the
    adaptive pixel-loss latents (the reference's module-level `adaptive_pix`,
    models/helpers.py:8-9), all resident on one GPU.

    state_dict()/load_state_dict() use the reference's tensor names and layouts
    (models/networks.py:40-49): the blob is the reference's tensors back to back.
    """

    def __init__(self, angles_deg, periods, freqs, res, params=None, device="cuda", ksplit=None,
                 lrate=5e-4, lrate_decay=500, offsets=(0.0, -1.0, 1.0, 0.5, -0.5), width=NPP_WIDTH, loss_type="robust_loss_adaptive", out_act=1,
                 precision="bf16"):
        """precision: the arithmetic of the MLP's TRAINING launches.  'bf16' (default): the fused bf16 chain with its 8-bit / 16-bit
        stash.  'fp32': the exact chain -- forward with an fp32 stash, data-gradient chain and weight gradients on
        v_mfma_f32_32x32x2_f32 (npp_mlp_fwd32_train / npp_mlp_bwd32 / npp_mlp_wgrad32), the reference's own arithmetic type; Adam is
        npp_adam_step_net on the fp32 master weights either way.  An fp32 net renders (render_image / psnr of a fit) through
        render_fp32, render() stays the bf16 chain on packs refreshed when the weights have changed, and npp_tune("stash8") has
        no effect on it.
        loss_type: --loss_type of options/arg_config.py:34 (models/mse_calculator.py:19-23): 'robust_loss_adaptive' (default), 'l2',
        'robust_loss' (the two non-adaptive forms leave the adaptive latents untouched: no gradient reaches them)."""
        self.loss_type, self.quad = loss_type, ops.quad_coef(loss_type)
        if out_act not in (1, 2):
            raise ValueError("out_act: 1 (sigmoid, --normalize_type 1) or 2 (tanh, --normalize_type 2: images in [-1, 1]; helpers.py:55-58)")
        self.out_act = int(out_act)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision {precision!r}: 'bf16' (fused bf16 chain) or 'fp32' (exact fp32 training chain)")
        self.precision = precision
        self.cfg = EmbedCfg.make(angles_deg, periods, freqs, res, offsets)
        self.K = int(self.cfg.K)
        self.width = int(width)      # 256 (BASELINE configs) or 512 (the reference's default --netwidth): one fused library each
        self.device = ops.select_device(device)
        self.layout, self.n_params = param_layout(self.K, self.width)
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        # adaptive_pix latents: [latent_alpha(3) | latent_scale(3)]  (adaptive.py:146-181)
        self.latents = torch.tensor([LATENT_ALPHA_INIT] * 3 + [0.0] * 3, dtype=torch.float32, device=self.device)
        self.lat_m = torch.zeros_like(self.latents)
        self.lat_v = torch.zeros_like(self.latents)
        self.dlatent = torch.zeros(6, dtype=torch.float32, device=self.device)
        # two loss accumulators used alternately: the fused Adam launch clears the idle one, so the
        # value of the finished iteration stays readable and zero_grad() needs no fill kernels
        self._loss_bufs = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._loss_idx = 0
        self._clean = False
        self.spline, self.n_knots, self.x_scale = ops.load_spline(self.device)
        self.ksplit = int(ksplit) if ksplit else ops.auto_ksplit(self.K, self.device, self.width)   # None / 0: one round of workgroups
        self.lrate, self.lrate_decay = float(lrate), int(lrate_decay)
        self.lr = float(lrate)
        self.global_step = 0        # train.py:337
        self.lr_clock = True        # False: the LR clock never advances (NPP_segmentation/train.py:408: `global_step += 1` sits
                                    # outside the loop there, so that task trains at a constant lrate) -- reproduced, not fixed
        self.opt_step = 0           # Adam's per-parameter step count
        self.wf = torch.zeros(ops.pack_bytes(self.K, 0, self.width), dtype=torch.uint8, device=self.device)
        self.wb = torch.zeros(ops.pack_bytes(self.K, 1, self.width), dtype=torch.uint8, device=self.device)
        self._ws = {}
        self.fused_repack = True    # False: Adam and the weight re-pack as two launches (comparator of the fused adam_pack launch)
        if precision == "fp32":
            self.fused_repack = False   # npp_adam_step_net on the fp32 master weights, then the fp32 packs are rebuilt
            self._w32b, self._wf_stamp = None, None
        if params is not None:
            self.load_state_dict(params)

    # ---- parameters -----------------------------------------------------------------
    def load_state_dict(self, sd):
        flat = np.zeros(self.n_params, np.float32)
        for name, off, rows, cols in self.layout:
            a = sd[name]
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            if a.size != rows * cols:
                raise ValueError(f"{name}: expected {rows}x{cols}, got {a.shape}")
            flat[off:off + rows * cols] = a.astype(np.float32).reshape(-1)
        self.params.copy_(torch.from_numpy(flat))
        self.repack()

    def _named(self, flat):
        """A host blob as a reference-named dict: weights (rows, cols), biases flat."""
        out = {}
        for name, off, rows, cols in self.layout:
            a = flat[off:off + rows * cols]
            out[name] = a.reshape(rows, cols).copy() if name.endswith("weight") else a.copy()
        return out

    def state_dict(self):
        return self._named(self.params.detach().cpu().numpy())

    def _slab_sum(self, gslabs):
        """The gradient blob a slab buffer holds: the sum of its split-K slabs (slab stride = n_params rounded up to 4)."""
        return gslabs.view(self.ksplit, -1)[:, :self.n_params].sum(0)

    def grads(self):
        """Sum of the split-K slabs, as a reference-named dict (for tests)."""
        return self._named(self._slab_sum(self._ws_last["gslabs"]).cpu().numpy())

    def repack(self):
        if self.precision == "fp32":
            # both fp32 packs now; the bf16 packs of render() lazily (_wf_pack)
            self._w32_stamp = None
            self._w32_pack()
            self._w32b = ops.pack_weights32_bwd(self.params, self.K, self._w32b, self.width)
            return
        ops.pack_weights(self.params, self.K, self.wf, self.wb, self.width)

    def _wf_pack(self):
        """The bf16 forward pack render() / render_at / render_grid read.  A bf16 net keeps it current in its Adam launch; an fp32 net
        rebuilds it (and wb) here when the parameters have changed since it was made, as _w32_pack does."""
        if self.precision == "fp32":
            stamp = (self.opt_step, self.params._version)
            if self._wf_stamp != stamp:
                ops.pack_weights(self.params, self.K, self.wf, self.wb, self.width)
                self._wf_stamp = stamp
        return self.wf

    # ---- workspaces -----------------------------------------------------------------
    def workspace(self, Bp):
        ws = self._ws.get(Bp)
        if ws is None:
            fp32 = self.precision == "fp32"      # actT / dzT then hold the fp32 stash / pre-activation gradients
            s = (ops.train_workspace32 if fp32 else ops.train_workspace)(self.K, Bp, self.ksplit, self.width)
            dev = self.device
            ws = {
                "actT": torch.empty(s[1], dtype=torch.uint8, device=dev),
                "dzT": torch.empty(s[2], dtype=torch.uint8, device=dev),
                "gslabs": torch.empty(s[3] // 4, dtype=torch.float32, device=dev),
                "pred": torch.empty((Bp, 3), dtype=torch.float32, device=dev),
                "dpred": torch.zeros((Bp, 3), dtype=torch.float32, device=dev),
            }
            self._ws[Bp] = ws
        self._ws_last = ws
        return ws

    def clear_dpred_tail(self, Bp, n_rows):
        """Rows >= n_rows of workspace Bp's dL/dpred never receive a gradient: cleared when the batch's row count changes."""
        ws = self._ws[Bp]
        if ws.get("n_rows") != n_rows:
            ws["dpred"][n_rows:].zero_()
            ws["n_rows"] = n_rows

    # ---- the path ---------------------------------------------------------------------
    def _render(self, src, precision, total=None, chunk_rows=None, inside=None, empty_ok=False, supersample=1):
        """The one render path (ops.render on the pack of `precision`).  src an (n, 2) int32 / float32 tensor: padded to whole 64-row
        tiles -> (n, 3).  src a function (start, n) -> ops.grid_arg / ops.view_arg with total canvas pixels: launches of at most
        chunk_rows chain rows, i.e. max(1, chunk_rows // supersample^2) pixels -> (total, 3) (and their inside bytes into `inside`)."""
        ss = ops.check_supersample(supersample)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision {precision!r}: 'bf16' (fused chain) or 'fp32' (exact chain)")
        if total is None and empty_ok and src.shape[0] == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self.device)
        pack = self._w32_pack() if precision == "fp32" else self._wf_pack()
        kw = dict(precision=precision, out_act=self.out_act, width=self.width)
        if total is None:
            n = src.shape[0]
            bp = ops.pad_rows(n)
            if bp != n:
                src = torch.cat([src, src.new_zeros((bp - n, 2))], 0)
            return ops.render(src.contiguous(), self.cfg, pack, self.params, **kw)[:n]
        out = torch.empty((total, 3), dtype=torch.float32, device=self.device)
        chunk = max(1, chunk_rows // (ss * ss))
        for s0 in range(0, total, chunk):
            n = min(chunk, total - s0)
            ops.render(src(s0, n), self.cfg, pack, self.params, out=out[s0:s0 + n],
                       inside=None if inside is None else inside[s0:s0 + n], supersample=ss, **kw)
        return out

    @staticmethod
    def _canvas(size, chunk_rows):
        Hc, Wc = (int(s) for s in size)
        if Hc < 1 or Wc < 1:
            raise ValueError(f"size {tuple(size)}: both sides must be >= 1")
        if int(chunk_rows) < 1:
            raise ValueError(f"chunk_rows {chunk_rows} must be >= 1")
        return Hc, Wc, int(chunk_rows)

    def render(self, coords):
        """render(None, emb[coords], args, **render_kwargs) of the reference (helpers.py:41-62)
        for arbitrary pixel coordinates; no gradient state is kept (train.py:277-309)."""
        return self._render(_pixel_coords(coords), "bf16")

    def render_fp32(self, coords):
        """The same render in EXACT fp32 (BASELINE config c4): fused chain on v_mfma_f32_32x32x2_f32 (npp_mlp_fwd32), the
        reference's own arithmetic type -- no bf16 operand rounding.  The fp32 weight pack is rebuilt when the parameters have
        changed since the last call."""
        return self._render(_pixel_coords(coords), "fp32")

    # ---- rendering at continuous positions (include/npp_hip.h "continuous coordinates") -------------------------------
    def _w32_pack(self):
        """The fp32 weight pack of the exact chain (render_fp32, render_at / render_grid in fp32), rebuilt when the parameters have
        changed since it was made."""
        stamp = (self.opt_step, self.params._version)
        if getattr(self, "_w32_stamp", None) != stamp:
            self._w32 = ops.pack_weights32(self.params, self.K, getattr(self, "_w32", None), self.width)
            self._w32_stamp = stamp
        return self._w32

    def render_at(self, coords, precision="bf16"):
        """The network at arbitrary real positions: coords (N, 2) [row y, col x] in the fit's pixel frame (sub-pixel, negative and
        past the border alike; a tensor or an array, converted to float32) -> (N, 3) on the device.  precision: 'bf16' (the fused
        chain of render()) or 'fp32' (the exact chain of render_fp32())."""
        c = torch.as_tensor(coords).to(device=self.device, dtype=torch.float32)
        if c.dim() != 2 or c.shape[1] != 2:
            raise ValueError(f"coords: expected (N, 2), got {tuple(c.shape)}")
        return self._render(c, precision, empty_ok=True)

    def render_grid(self, size, origin=(0.0, 0.0), scale=(1.0, 1.0), precision="bf16", chunk_rows=1 << 22, supersample=1):
        """A canvas of size = (H', W') pixels whose pixel (i, j) is the network at (y0 + i / sy, x0 + j / sx) of the fit's frame
        (origin = (y0, x0); scale = (sy, sx) canvas pixels per fit pixel, or one number for both) -> (H', W', 3) float32 on the
        device.  Chunked grid launches of at most chunk_rows pixels: no coordinate buffer is ever built.  Scale 1 at origin 0 is
        render() of the full int32 grid bit for bit; at an integer scale S, pixel (S i, S j) is pixel (i, j) of scale 1.
        supersample = S in (1, 2, 4, 8): every pixel is the mean of S x S samples spread evenly over its footprint (offsets
        (2 a + 1) / (2 S) - 0.5 of a pixel), averaged inside the launch -- antialiasing for a canvas coarser than the fit, at S^2
        times the chain rows and no extra memory; chunk_rows keeps bounding the rows of a launch, and the result does not depend on it.
        supersample = "adaptive" is one S for the whole canvas, view.supersample_for_density(max(1 / sy, 1 / sx)), the choice of
        `render --supersample auto`: a grid's density is the same at every pixel, so there is nothing to adapt (render_view is
        where the classes differ)."""
        Hc, Wc, chunk = self._canvas(size, chunk_rows)
        o, s = _pair(origin), _pair(scale)
        if isinstance(supersample, str) and supersample == "adaptive":
            from . import view
            supersample = view.supersample_for_density(max(1.0 / s[0], 1.0 / s[1]))
        return self._render(lambda s0, n: ops.grid_arg(s0, n, Wc, o, s), precision, Hc * Wc, chunk,
                            supersample=supersample).view(Hc, Wc, 3)

    def render_view(self, size, M, precision="bf16", chunk_rows=1 << 22, return_inside=False, supersample=1, return_classes=False):
        """render_grid under a projective map (view.py): pixel (i, j) of the size = (H', W') canvas is the network at
        ((m0 i + m1 j) + m2, (m3 i + m4 j) + m5) / ((m6 i + m7 j) + m8) of the fit's frame, M the row-major 3 x 3 map, converted to
        float32 once -> (H', W', 3) float32 on the device, and with return_inside also (H', W') uint8: 0 the pixel is not in view
        (behind the map's horizon or at a non-finite position; it renders zero), 1 in view, 3 in view and inside the fit's image
        rectangle.  Chunked view launches, no coordinate buffer.  The affine map [[1/sy, 0, y0], [0, 1/sx, x0], [0, 0, 1]] with
        power-of-two scales is render_grid bit for bit.  A non-finite or singular M raises ValueError before any launch.
        supersample = S as in render_grid, the sample positions going through the map; a sample that is not in view does not count,
        and the inside bytes stay those of the pixel centres (a pixel whose centre is not in view renders zero).
        supersample = "adaptive": every pixel gets the S its own footprint asks for (the rule of "auto" at the pixel centre, exact:
        include/npp_hip.h "adaptive supersampling") and is bit for bit the pixel of render_view(supersample=that S).  One class
        launch over the canvas, then per class S the row-major list of its pixels in listed launches of at most
        max(1, chunk_rows // S^2) pixels; an empty class launches nothing, a pixel not in view (class 0) is +0 with byte 0, and the
        result does not depend on chunk_rows.  return_classes adds the (H', W') uint8 class map (0, 1, 2, 4, 8) as the last result
        (of a uniform render: S where the pixel is in view)."""
        from . import view
        Hc, Wc, chunk = self._canvas(size, chunk_rows)
        m32 = view.check_matrix(M).astype(np.float32)
        if isinstance(supersample, str) and supersample == "adaptive":
            return self._render_view_adaptive(Hc, Wc, m32, precision, chunk, return_inside, return_classes)
        inside = torch.empty(Hc * Wc, dtype=torch.uint8, device=self.device) if return_inside or return_classes else None
        out = self._render(lambda s0, n: ops.view_arg(s0, n, Wc, m32), precision, Hc * Wc, chunk, inside,
                           supersample=supersample).view(Hc, Wc, 3)
        res = (out,) + ((inside.view(Hc, Wc),) if return_inside else ())
        if return_classes:
            res += ((inside.view(Hc, Wc) != 0).to(torch.uint8) * ops.check_supersample(supersample),)
        return res if len(res) > 1 else out

    def _render_view_adaptive(self, Hc, Wc, m32, precision, chunk_rows, return_inside, return_classes):
        """render_view(supersample="adaptive") behind its argument checks."""
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision {precision!r}: 'bf16' (fused chain) or 'fp32' (exact chain)")
        total = Hc * Wc
        whole = ops.view_arg(0, total, Wc, m32)
        cls = torch.empty(total, dtype=torch.uint8, device=self.device)
        ops.view_ss_classes(whole, (self.cfg.H, self.cfg.W), cls)
        out = torch.zeros((total, 3), dtype=torch.float32, device=self.device)
        inside = torch.zeros(total, dtype=torch.uint8, device=self.device)
        pack = self._w32_pack() if precision == "fp32" else self._wf_pack()
        for ss in ops.SUPERSAMPLES:
            pix = torch.nonzero(cls == ss).view(-1)             # row-major; its length is read by the host here
            chunk = max(1, chunk_rows // (ss * ss))
            for s0 in range(0, int(pix.shape[0]), chunk):
                ops.render(whole, self.cfg, pack, self.params, precision=precision, out=out, inside=inside, out_act=self.out_act,
                           width=self.width, supersample=ss, pixels=pix[s0:s0 + chunk])
        res = (out.view(Hc, Wc, 3),) + ((inside.view(Hc, Wc),) if return_inside else ()) + ((cls.view(Hc, Wc),) if return_classes else ())
        return res if len(res) > 1 else res[0]

    # ---- model file (modelfile.py) ---------------------------------------------------------
    def embedder_config(self):
        """(angles_deg (K, 2), periods (K, 2), freqs (10,), freq_offsets (5,), res (H, W)) as the embedder was built with."""
        c = self.cfg
        ang = np.array([[c.angles_deg[k][o] for o in range(2)] for k in range(self.K)], np.float32)
        per = np.array([[c.periods[k][o] for o in range(2)] for k in range(self.K)], np.float32)
        return ang, per, np.array(list(c.freqs), np.float32), np.array(list(c.offsets), np.float32), (int(c.H), int(c.W))

    def save(self, path, **meta):
        """Write the network as a model file (modelfile.py: weights under the reference's names, adaptive latents, embedder
        configuration; meta: optional strings such as task / image / iterations)."""
        from . import modelfile
        ang, per, freqs, offs, res = self.embedder_config()
        modelfile.write(path, self.state_dict(), self.latents.detach().cpu().numpy(), ang, per, freqs, res, self.width,
                        out_act=self.out_act, freq_offsets=offs, **meta)

    @classmethod
    def load(cls, path, device="cuda"):
        """An NPPNet from a model file, ready to render (no optimiser state: a fresh Adam if it were trained on).  .meta holds the
        file's string metadata.  ValueError for a file that is not a model file this build reads."""
        from . import modelfile
        from ._lib import FUSED_WIDTHS
        d = modelfile.read(path)
        if d["width"] not in FUSED_WIDTHS:
            raise ValueError(f"{path}: width {d['width']} has no fused library (built: {FUSED_WIDTHS})")
        net = cls(d["angles_deg"], d["periods"], d["freqs"], d["res"], params=d["params"], device=device,
                  offsets=tuple(float(o) for o in d["freq_offsets"]), width=d["width"], out_act=d["out_act"])
        net.latents.copy_(torch.from_numpy(d["latents"]).to(net.device))
        net.meta = dict(d["meta"])
        return net

    def forward_train(self, coords_padded):
        """Forward with stashes; coords must already be padded to a multiple of 64 rows."""
        ws = self.workspace(coords_padded.shape[0])
        if self.precision == "fp32":
            return ops.mlp_fwd32_train(coords_padded, self.cfg, self._w32_pack(), self.params, ws["pred"], ws["actT"], self.out_act, self.width)
        ops.mlp_fwd(coords_padded, self.cfg, self.wf, self.params, ws["pred"], ws["actT"], self.width, out_act=self.out_act)
        return ws["pred"]

    def backward(self, Bp, patch=None):
        """loss.backward() through the MLP: consumes ws['dpred'] (rows beyond the batch 0).  patch = (dx_a, dx_b, fmask, rmask,
        row0, n_p, k, P, comp): the patch rows' dL/dpred is formed inside the launch from the patch losses' image gradients."""
        ws = self._ws[Bp]
        if self.precision == "fp32":
            if patch is not None:
                raise ValueError("precision='fp32': the patch-folded backward launch has no fp32 form (use npp_patch_compose_bwd, then backward(Bp))")
            if self._w32b is None:
                self.repack()
            ops.mlp_bwd32(ws["dpred"], ws["pred"], self.K, self._w32b, self.params, ws["actT"], ws["dzT"], self.width, out_act=self.out_act)
            ops.mlp_wgrad32(ws["dzT"], ws["actT"], self.cfg, Bp, self.K, self.ksplit, ws["gslabs"], self.width)
            return
        if patch is not None:
            ops.mlp_bwd_patch(ws["dpred"], ws["pred"], self.K, self.wb, self.params, ws["actT"], ws["dzT"], *patch, width=self.width, out_act=self.out_act)
        else:
            ops.mlp_bwd(ws["dpred"], ws["pred"], self.K, self.wb, self.params, ws["actT"], ws["dzT"], self.width, out_act=self.out_act)
        ops.mlp_wgrad(ws["dzT"], ws["actT"], Bp, self.K, self.ksplit, ws["gslabs"], self.width)

    # ---- stash audit: what the iteration's 8-bit stash did, read back from the workspace -------------------
    def stash_census(self, Bp, n_rows):
        """Census of the 8-bit stash the last forward_train / backward of workspace Bp left (npp_stash8_census): {array name:
        {"format", "features", "elements", "zero", "subnormal", "at_max", "nonfinite", "exp_hist"}} for rows < n_rows; the per-tile
        scale summary of dzF stays in .last_tile_scale.  Call it before anything overwrites the stash (stash_gap does)."""
        ops.refuse_stash_audit(self.precision)
        ws = self._ws[Bp]
        if "census" not in ws:
            ws["census"] = ops.stash8_census(ws["actT"], ws["dzT"], Bp, n_rows, self.K, None, self.width)
        else:
            ops.stash8_census(ws["actT"], ws["dzT"], Bp, n_rows, self.K, ws["census"], self.width)
        arrays, self.last_tile_scale = ops.census_decode(ws["census"].cpu().numpy(), self.K, self.width)
        return arrays

    def stash_gap(self, Bp, coords):
        """How far the weight gradients of this iteration (the slabs backward(Bp) left: what Adam will read) are from the 16-bit
        stash's: {tensor name: rel_l2(g8, g16)} under the reference's state_dict names.  The 16-bit leg re-runs the iteration's own
        launches with npp_tune("stash8") = 0 -- forward_train on `coords` (the padded rows of the batch: identical pred), the plain
        backward on the retained dL/dpred (complete after a patch-folded backward), the weight gradient into a second slab buffer
        this net allocates once -- so pred, dpred, the slabs and the loss words are as the iteration left them; the stash is not
        (take stash_census first).  The switch is process-wide for the duration of the three enqueues: not for fits on other host
        threads of this process."""
        ops.refuse_stash_audit(self.precision)
        ws = self._ws[Bp]
        if "gslabs16" not in ws:
            ws["gslabs16"] = torch.empty_like(ws["gslabs"])
        old = ops.tune("stash8", 0)
        try:
            ops.mlp_fwd(coords, self.cfg, self.wf, self.params, ws["pred"], ws["actT"], self.width, out_act=self.out_act)
            ops.mlp_bwd(ws["dpred"], ws["pred"], self.K, self.wb, self.params, ws["actT"], ws["dzT"], self.width, out_act=self.out_act)
            ops.mlp_wgrad(ws["dzT"], ws["actT"], Bp, self.K, self.ksplit, ws["gslabs16"], self.width)
        finally:
            ops.tune("stash8", old)
        self._ws_gap = ws
        g8 = self._slab_sum(ws["gslabs"]).double()      # the sums grads() forms, then float64
        g16 = self._slab_sum(ws["gslabs16"]).double()
        d = g8 - g16
        num = torch.stack([torch.linalg.vector_norm(d[off:off + rows * cols]) for _, off, rows, cols in self.layout])
        den = torch.stack([torch.linalg.vector_norm(g16[off:off + rows * cols]) for _, off, rows, cols in self.layout])
        gap = (num / den.clamp_min(1e-30)).cpu().numpy()
        return {name: float(gap[i]) for i, (name, *_r) in enumerate(self.layout)}

    def stash_gap_grads16(self):
        """The 16-bit leg's gradients of the last stash_gap(), in the form of grads() (for tests)."""
        return self._named(self._slab_sum(self._ws_gap["gslabs16"]).cpu().numpy())

    def pixel_loss(self, Bp, n_rows, gt, mask=None, weight=1.0):
        """img2mse on the first n_rows rows of the current prediction (train.py:195);
        writes dL/dpred for those rows and accumulates the latent gradients."""
        ws = self._ws[Bp]
        ops.pixel_loss(ws["pred"][:n_rows], gt, mask, self.latents, self.spline, self.n_knots, self.x_scale,
                       weight, self.loss_buf, ws["dpred"][:n_rows], self.dlatent, quad=self.quad)

    def pixel_loss_args(self, Bp, n_rows, gt, mask=None, weight=1.0):
        """The argument tuple of pixel_loss() for a launch that carries the loss along (ops.trunk_patch_in(loss=...))."""
        ws = self._ws[Bp]
        if getattr(self, "_pl_scratch", None) is None and ops.DETERMINISTIC and self.fused_repack:
            # the launch leaves its per-block partial sums here; the fused Adam launch of the iteration (_adam) adds them in block
            # order: bit-reproducible sums at no cost (include/npp_hip.h npp_pixel_loss_args.scratch)
            self._pl_scratch = torch.zeros(ops.PIXEL_LOSS_SCRATCH, dtype=torch.float32, device=self.device)
        return (ws["pred"][:n_rows], gt, mask, self.latents, self.spline, self.n_knots, self.x_scale, weight, self.loss_buf,
                ws["dpred"][:n_rows], self.dlatent, getattr(self, "_pl_scratch", None), self.quad)

    def optimizer_step(self, Bp):
        """optimizer.step() + the LR rule of train.py:253-263 + global_step += 1 (:337)."""
        ws = self._ws[Bp]
        idle = self._loss_bufs[1 - self._loss_idx:2 - self._loss_idx]
        self._adam(ws["gslabs"], self.ksplit, ws["gslabs"].numel() // self.ksplit, idle)
        self.optimizer_advance()
        if not self.fused_repack:
            self.repack()                # after the advance: the fp32 packs are stamped with the step count they belong to

    # ---- the same step for a captured iteration (fit.CompletionFit(graph_iteration=True)): launch and host record apart ----
    def step_words(self):
        """(step_size, 1 / sqrt(1 - b2^t)) of the NEXT optimizer step as npp_adam_step_net_pack would compute them from (lr, opt_step + 1):
        what the caller writes into the device words of optimizer_launch_dev() before the launch runs."""
        return ops.adam_words(self.lr, self.opt_step + 1)

    def optimizer_launch_dev(self, Bp, hp):
        """The launch of optimizer_step() with its step-dependent scalars read from the device words hp[0:2] (step_words()): nothing
        on the host changes, so a capture may record it and a graph replay it; optimizer_advance() is the host half."""
        if not self.fused_repack:
            raise ValueError("optimizer_launch_dev: the fused Adam + re-pack launch only (precision='bf16', fused_repack)")
        ws = self._ws[Bp]
        gslabs = ws["gslabs"]
        idle = self._loss_bufs[1 - self._loss_idx:2 - self._loss_idx]
        ops.adam_step_net_pack_dev(self.params, self.m, self.v, gslabs, self.ksplit, gslabs.numel() // self.ksplit, self.latents, self.lat_m,
                                   self.lat_v, self.dlatent, idle, hp, self.K, self.wf, self.wb, self.width,
                                   pl_partials=getattr(self, "_pl_scratch", None), loss_cur=self.loss_buf)

    def optimizer_advance(self):
        """What optimizer_step() leaves on the host: the step count, the LR rule of train.py:253-263, global_step (:337)."""
        self.opt_step += 1
        self.lr = ops.lr_rule(self.lrate, self.lrate_decay, self.global_step)
        if self.lr_clock:
            self.global_step += 1
        self._clean = True

    def _adam(self, gslabs, n_slabs, stride, idle):
        """The launch of optimizer.step() number opt_step + 1 over the blob + latents: with the re-pack of the bf16 MFMA packs
        in it (fused_repack, default), or npp_adam_step_net alone (the comparator: optimizer_step() re-packs after it).  The
        caller advances the host record (optimizer_advance)."""
        if self.fused_repack:
            # (the pixel-loss launch of a folded iteration left its block partials in _pl_scratch: summed here in block order;
            #  the buffer's count word is zero whenever no such launch ran since the last step)
            ops.adam_step_net_pack(self.params, self.m, self.v, gslabs, n_slabs, stride, self.latents, self.lat_m, self.lat_v,
                                   self.dlatent, idle, self.lr, self.opt_step + 1, self.K, self.wf, self.wb, self.width,
                                   pl_partials=getattr(self, "_pl_scratch", None), loss_cur=self.loss_buf)
        else:
            ops.adam_step_net(self.params, self.m, self.v, gslabs, n_slabs, stride, self.latents, self.lat_m, self.lat_v,
                              self.dlatent, idle, self.lr, self.opt_step + 1)

    @property
    def loss_buf(self):
        """Accumulator of the current iteration's pixel loss (1 float on the device)."""
        return self._loss_bufs[self._loss_idx:self._loss_idx + 1]

    def zero_grad(self, force=False):
        """optimizer.zero_grad() (train.py:192).  After optimizer_step() the latent gradient and the
        idle loss accumulator are already zero: switch to it instead of launching fill kernels."""
        if self._clean and not force:
            self._loss_idx ^= 1
        else:
            self.dlatent.zero_()
            self.loss_buf.zero_()
        self._clean = False
