"""The per-image optimisation loop of NPP_completion/train.py:133-337, host side.

One CompletionFit owns one image on one GPU: the masked input, the train/val pixel
split (loaders/loaders.py:107-108), the NPPNet state and the NumPy RNG whose call order
follows the reference (np.random.choice over i_train per iteration, train.py:172).  All
arithmetic of an iteration runs in libnpp_hip.so; this file samples indices, gathers the
ground-truth colours (torch indexing: glue) and sequences the kernels.
"""
import math

import os

import numpy as np
import torch

from . import ops
from .audit import AuditSchedule, saturated, refuse as refuse_audit
from .model import NPPNet
from .sampler import GridPatchSampler
from .losses import ContextualLoss, LPIPS


def _hand_over(v, stream):
    """The tensors of a batch materialised on the sampler stream are read on `stream`: the allocator must not recycle them before."""
    if isinstance(v, torch.Tensor):
        v.record_stream(stream)
    elif isinstance(v, dict):
        for x in v.values():
            _hand_over(x, stream)
    elif isinstance(v, (list, tuple)):
        for x in v:
            _hand_over(x, stream)


def refuse_graph_iteration(precision, trunk_precision, task, style_weight, exc, flag=False):
    """graph_iteration is built for the default arithmetic of the completion and segmentation tasks: everything else is refused by
    name (exc: ValueError for the constructor, SystemExit for the command line; flag: name the switches as flags)."""
    a = (lambda k, v: f"--{k} {v}") if flag else (lambda k, v: f"{k}={v!r}")
    me = "--graph_iteration" if flag else "graph_iteration=True"
    if precision != "bf16":
        raise exc(f"{me} with {a('precision', precision)}: the exact-fp32 chain is a diagnostic mode and runs launch by launch "
                  f"(precision 'bf16' only)")
    if trunk_precision != "fp16":
        raise exc(f"{me} with {a('trunk_precision', trunk_precision)}: the exact-fp32 trunks are a diagnostic mode and run launch by "
                  f"launch (trunk_precision 'fp16' only)")
    if task == "remapping":
        raise exc(f"{me} with {a('task', task)}: the style head still allocates per iteration and its side-stream question is open "
                  f"(DESIGN.md section 4); completion and segmentation only")
    if style_weight is not None:
        raise exc(f"{me} with {a('style_weight', style_weight)}: the style term is not built into the captured iteration")


class CompletionFit:
    def __init__(self, img, mask, angles_deg, periods, freqs, params, device="cuda", N_rand=8192,
                 ksplit=None, seed=0, lrate=5e-4, lrate_decay=500, valid_mask=None, shifts=None,
                 patch_size=None, patch_num=2, num_real_patch_per_sample=3, invalid_ratio=0.3,
                 contextual_weight=1e-3, perceptual_weight=1e-3, use_comp=True, patch_size_decay=2000,
                 vgg19_state_dict=None, vgg16_state_dict=None, lpips_lin_weights=None, rng_mode="reference",
                 prefetch=0, use_perceptual_loss=True, task="completion", clear_mask=None, style_weight=None,
                 vgg16_style_state_dict=None, masked_img=None, width=256, no_reg_sampling=False, use_patch_weight=False,
                 no_pix_loss=False, use_contextual_loss=True, loss_type="robust_loss_adaptive", use_adaptive_perceptual_loss=True, normalize_type=1,
                 precision="bf16", trunk_precision="fp16", graph_iteration=False, stash_audit=0, trunk_audit=0):
        """img (H,W,3) float in [0,1]; mask (H,W,1) 1 = known (loaders.py:92-101).
        precision: the arithmetic of the coordinate MLP's training launches, 'bf16' (default) or 'fp32' (NPPNet(precision=...): the
        exact fp32 chain, the reference's own arithmetic; the iteration then takes the unfolded launch sequence -- fold_launches =
        False -- and the evaluation renders in fp32).  It is the MLP's precision only.
        trunk_precision: the arithmetic of the VGG trunks of the patch losses, 'fp16' (default: losses.HipTrunk) or 'fp32'
        (losses.HipTrunk32, exact fp32 convolutions; independent of `precision`).  A diagnostic mode: the iteration forms the fp32
        batch with npp_patch_compose_fwd, runs the pixel loss as its own launch and the LPIPS branch launch by launch (lp_graph = False).
        normalize_type: --normalize_type (arg_config.py:31): 1 = sigmoid output, 2 = tanh output (helpers.py:55-58).  The reference
        rescales ONLY its evaluation image to [-1, 1] under 2 (loaders.py:56,111); the loop still trains on masked_img in [0, 1]
        (train.py:173) -- reproduced as it is: pass `img` already rescaled if the evaluation should see it that way.
        width: --netwidth, 256 (BASELINE configs) or 512 (the reference's default, arg_config.py:57); `params` must match.
        use_adaptive_perceptual_loss: False = LPIPS(use_robust=False) in the loop (arg_config.py:78, train.py:241-246).
        loss_type: --loss_type (arg_config.py:34; models/mse_calculator.py:19-23): 'robust_loss_adaptive' | 'l2' | 'robust_loss'.
        Ablation switches of arg_config.py:78-92: no_reg_sampling (random real patches), use_patch_weight (1/d lattice weights:
        weighted-sum forms of the contextual and LPIPS terms, train.py:224-250), no_pix_loss (:197), use_contextual_loss.
        masked_img = img * mask is what the loop trains on (train.py:173).
        rng_mode: "reference" (default) keeps the reference's NumPy random stream call by call
        (np.random.uniform, np.random.choice(replace=False) for the patch centres and the N_rand pixel rows:
        train.py:172, sampler.py:260,324) -- each choice permutes its whole population, 2.7 ms of host time per
        iteration at 512^2, three times the device time of the iteration.  The stream comes from the library's own
        MT19937 (host_rng.NativeRandomState: bit-identical to np.random.RandomState(seed), GIL-free); "numpy" uses NumPy's
        generator itself.  "fast" draws the same uniform without-replacement samples with np.random.Generator.choice
        (O(size)): same distribution, different stream.
        prefetch: > 0 runs the host half of the sampler (draw_batch) that many iterations ahead on a producer thread --
        it never reads network state, so the stream and the results are unchanged; with the native generator the draws
        overlap the training loop instead of preceding it.
        "device" draws on the GPU (dev_sampler.DeviceDraws; models/sampler.py:242-354 and train.py:172 as two launches on the
        sampler stream): Philox4x32-10 keyed by `seed`, every draw a pure function of (seed, draw index) -- its own stream, the
        same distribution; no host arithmetic per draw, so no producer thread (prefetch must be 0).
        graph_iteration: True replays the device side of an iteration (step_from) as ONE captured HIP graph per iteration shape
        instead of enqueuing its launches (_step_from_graph): the bits of the launch-by-launch loop at one graph launch of host
        time per iteration.  Built for the default arithmetic (precision='bf16', trunk_precision='fp16') of the completion and
        segmentation tasks without a style term; the other modes are refused by name.
        stash_audit: N > 0 audits the 8-bit training stash on every N-th iteration of step_full() (0, the default: never;
        audit_next() arms one iteration): between the weight-gradient and the optimiser launch the iteration's stash is counted
        (NPPNet.stash_census) and its weight gradients are compared with the 16-bit stash's (NPPNet.stash_gap).  Reports collect in
        .stash_audits (the last MAX_STASH_AUDITS) and .last_stash_audit.  Nothing the optimiser reads is touched: an audited fit
        ends with the bits of an unaudited one.  Refused by name for precision='fp32' and under npp_tune("stash8") = 0.
        trunk_audit: N > 0 audits the fp16 VGG trunks of the patch losses on every N-th iteration (0, the default: never;
        audit_trunk_next() arms one iteration): behind the backward launch and in front of the optimiser
        launches every tensor the iteration's trunks stored is counted (HipTrunk.census) and each patch-loss term that ran is run
        again on exact-fp32 twins of the trunks (_trunk_audit).  Reports collect in .trunk_audits (the last MAX_TRUNK_AUDITS) and
        .last_trunk_audit.  Nothing the optimiser reads is written: an audited fit ends with the bits of an unaudited one.
        Refused by name for trunk_precision='fp32' and for a fit without patch losses (shifts=None)."""
        for kind, every in (("trunk", int(trunk_audit)), ("stash", int(stash_audit))):
            if every < 0:
                raise ValueError(f"{kind}_audit must be >= 0 (0: never)")
            if every:
                refuse_audit(kind, capturing=False, precision=precision, trunk_precision=trunk_precision, patch_losses=shifts is not None)
        self._audits = {"trunk": AuditSchedule(trunk_audit, self.MAX_TRUNK_AUDITS), "stash": AuditSchedule(stash_audit, self.MAX_STASH_AUDITS)}
        # what the fp32 twins of the trunk audit are built from: the caller's own objects, by reference (the shared weight cache is
        # keyed by the state dict's identity)
        self._trunk_sd = dict(vgg19=vgg19_state_dict, vgg16=vgg16_state_dict, lins=lpips_lin_weights, style=vgg16_style_state_dict)
        self._twins, self._audit_xy, self._audit_loss, self.trunk_audit_tensors = {}, {}, None, None
        if rng_mode not in ("reference", "numpy", "fast", "device"):
            raise ValueError("rng_mode must be 'reference', 'numpy', 'fast' or 'device'")
        if rng_mode == "device" and int(prefetch) > 0:
            raise ValueError("rng_mode='device' with prefetch > 0: the draws run on the GPU, there is no producer thread to run ahead "
                             "(pass prefetch=0)")
        if rng_mode == "device" and no_reg_sampling:
            raise ValueError("rng_mode='device' with no_reg_sampling=True: the random-patch ablation is not built for the device draws")
        if trunk_precision not in ("fp16", "fp32"):
            raise ValueError("trunk_precision must be 'fp16' or 'fp32'")
        self.trunk_precision = trunk_precision
        if task not in ("completion", "remapping", "segmentation"):
            raise ValueError("task must be 'completion', 'remapping' or 'segmentation'")
        self.graph_iteration = bool(graph_iteration)
        if self.graph_iteration:
            refuse_graph_iteration(precision, trunk_precision, task, style_weight, ValueError)
        # False: the folded launches as separate ones (npp_pixel_loss, npp_patch_compose_bwd: the comparator of
        # tests/test_gpu_parity.py::test_folded_launches_equal_the_separate_ones).  Measured and removed in round 5 (they are in the
        # history of rounds 3-4, profiles/r03_rejected_experiments.txt #2 #5): the pixel rows as a row group of their own on a side
        # stream (0.742 -> 0.762 ms) and the next iteration's real-patch trunk pass prefetched on a side stream (0.767 -> 0.776 ms).
        self.fold_launches = True
        img = np.asarray(img, np.float32)
        mask = np.asarray(mask, np.float32).reshape(img.shape[0], img.shape[1], 1)
        self.H, self.W = img.shape[:2]
        self.device = ops.select_device(device)
        valid = np.ones_like(mask) if valid_mask is None else np.asarray(valid_mask, np.float32).reshape(mask.shape)
        self.task = task
        if task in ("completion", "segmentation"):
            # segmentation (NPP_segmentation/train.py:62-157): the same loop with the initial PERIODIC region as the known mask
            # and the masked-blurred image as the image trained and sampled on -- the caller passes them as `mask` and
            # `masked_img` (io.load_npp_segmentation)
            mask = mask * valid
            # loaders.py:107-108: np.nonzero order (row-major) for both splits
            self.i_train = np.stack(np.nonzero(mask[..., 0] * valid[..., 0]), 1).astype(np.int32)
            self.i_val = np.stack(np.nonzero((1 - mask[..., 0]) * valid[..., 0]), 1).astype(np.int32)
            pixel_mask = None                                        # gt_mask = ones (train.py:176)
            # masked_img is what the loop trains and samples patches on (train.py:173; the sampler gets masked_img): the file
            # as loaded when the caller has it (it need not equal gt * mask, e.g. inputs without a clean ground truth)
            train_img = img * mask if masked_img is None else np.asarray(masked_img, np.float32).reshape(img.shape)
        else:
            # NPP_remapping: the whole valid image is trained on (loaders.py:279), the 'val' pool and the sampler mask are the
            # CLEAR (non-blurry) region (:280; NPP_remapping/train.py:147-155), and the pixel loss weighs blurry pixels 0.3
            # through gt_mask = clear_mask (train.py:203; models/mse_calculator.py:17)
            if clear_mask is None:
                raise ValueError("task='remapping' needs clear_mask (H,W[,1]): 1 = sharp region (NPP_remapping/blur_detection.py)")
            mask = np.asarray(clear_mask, np.float32).reshape(mask.shape) * valid
            self.i_train = np.stack(np.nonzero(valid[..., 0]), 1).astype(np.int32)
            self.i_val = np.stack(np.nonzero(mask[..., 0] * valid[..., 0]), 1).astype(np.int32)
            pixel_mask = mask
            train_img = img
        self.pix_w = 0.0 if no_pix_loss else 1.0                      # train.py:197-198 `loss = 0`: the pixel term weighs nothing
        self.use_patch_weight, self.use_contextual_loss = bool(use_patch_weight), bool(use_contextual_loss)
        self.lp_robust = bool(use_adaptive_perceptual_loss)
        self.img = torch.from_numpy(img).to(self.device)
        self.mask = torch.from_numpy(mask).to(self.device)
        self.masked_img = torch.from_numpy(np.ascontiguousarray(train_img, np.float32)).to(self.device).contiguous()
        self.pixel_mask = None if pixel_mask is None else torch.from_numpy(pixel_mask[..., 0].copy()).to(self.device)
        self.net = NPPNet(angles_deg, periods, freqs, (self.H, self.W), params=params, device=self.device,
                          ksplit=ksplit, lrate=lrate, lrate_decay=lrate_decay, width=width, loss_type=loss_type,
                          out_act=int(normalize_type), precision=precision)
        self.precision = precision
        if precision == "fp32":
            self.fold_launches = False                             # npp_pixel_loss, npp_trunk_patch_in, npp_patch_compose_bwd, backward
        if task == "segmentation":
            self.net.lr_clock = False                              # NPP_segmentation/train.py:408 (see NPPNet.lr_clock)
        self.N_rand = int(min(N_rand, self.i_train.shape[0]))
        self.rng_mode, self.seed = rng_mode, int(seed)
        if rng_mode == "reference":
            from .host_rng import NativeRandomState
            self.rng = NativeRandomState(seed)
        else:
            self.rng = np.random.RandomState(self.seed & 0xFFFFFFFF if rng_mode == "device" else seed)   # (device: a 64-bit key, no host stream)
        self._dev_draws = None                                    # rng_mode "device": the two launches (dev_sampler.DeviceDraws), on first use
        self.fast_rng = np.random.default_rng(seed) if rng_mode == "fast" else None
        self._prefetch, self._producer, self._queue, self._stop = int(prefetch), None, None, False
        self._ahead, self._s_smp, self.side_sampler = None, None, True   # device half of the sampler one iteration ahead (step_full)
        self._draw_iter = 0                                       # iterations drawn so far (== self.iteration without prefetch)
        self.i_train_dev = torch.from_numpy(self.i_train).to(self.device)
        yy, xx = np.meshgrid(np.arange(self.H, dtype=np.int32), np.arange(self.W, dtype=np.int32), indexing="ij")
        self.i_all_dev = torch.from_numpy(np.stack([yy, xx], -1).reshape(-1, 2)).to(self.device)
        self.iteration = 0
        # ---- patch losses (train.py:50-51,126-130): only when the periodicity shifts are given
        self.patch_sampler = None
        if shifts is not None:
            self.patch_size = int(patch_size) if patch_size else int(np.clip(max(np.asarray(periods).reshape(-1, 2)[0])
                                                                  + (32 - max(np.asarray(periods).reshape(-1, 2)[0]) % 32), 64, 160))
            self.patch_num = int(patch_num)
            self.topk, self.invalid_ratio = int(num_real_patch_per_sample), float(invalid_ratio)
            self.cx_w, self.lp_w, self.use_comp = float(contextual_weight), float(perceptual_weight), bool(use_comp)
            self.use_perceptual_loss = bool(use_perceptual_loss)             # options/arg_config.py use_perceptual_loss
            self.patch_size_decay = int(patch_size_decay)
            self.patch_sampler = GridPatchSampler(
                img=self.masked_img[None], mask=self.mask[None], N_samples=self.patch_num, patch_size=self.patch_size,
                height=self.H, width=self.W, pool_train=self.i_train, pool_val=self.i_val, selected_shifts=shifts,
                no_reg_sampling=bool(no_reg_sampling), rng=self.rng, fast_rng=self.fast_rng)
            self.contextualLoss = ContextualLoss(use_vgg=True, vgg_state_dict=vgg19_state_dict, device=self.device,
                                                 trunk_precision=trunk_precision).to(self.device)
            self.percepLoss = LPIPS(net="vgg", lin_weights=lpips_lin_weights, vgg_state_dict=vgg16_state_dict,
                                    device=self.device, trunk_precision=trunk_precision)
            self.style, self.style_w = None, 0.0
            if style_weight is not None or task == "remapping":
                from .losses import StyleLoss
                self.style = StyleLoss(vgg_state_dict=vgg16_style_state_dict, device=self.device, trunk_precision=trunk_precision)
                self.style_w = 1.0 if style_weight is None else float(style_weight)        # arg_config.py: style_weight 1
            self.last_source, self.skipped = None, 0
            self._xy, self._xy_key, self._xy_bufs = None, None, {}
            # the LPIPS branch of a 'same' iteration as ONE captured HIP graph (lpips_branch); lp_graph = False keeps the launches
            self._lp_graphs, self.lp_graph = {}, trunk_precision == "fp16"
            self._s_lp = torch.cuda.Stream(self.device)
            self.patch_loss_buf = torch.zeros(1, dtype=torch.float32, device=self.device)
        # ---- graph_iteration (see _step_from_graph): captured iterations by key, the two sets of batch buffers per batch shape, the
        # scalar record (device words + a small ring of pinned words, each guarded by the event behind the iteration that read it)
        self._it_graphs, self._it_stats, self._graph_ok = {}, {"captured": 0, "replayed": 0, "eager": 0}, True
        self._sets, self._wset, self._it_shape, self._s_it = {}, 0, None, None
        if self.graph_iteration:
            self._rec = torch.zeros(4, dtype=torch.float32, device=self.device)
            self._rec_pin = torch.zeros((self._REC_SLOTS, 4), dtype=torch.float32).pin_memory()
            self._rec_np, self._rec_ev, self._rec_i = self._rec_pin.numpy(), [None] * self._REC_SLOTS, 0

    MAX_STASH_AUDITS = 4096   # reports kept in .stash_audits (a deque: the oldest go first)
    MAX_TRUNK_AUDITS = 4096   # reports kept in .trunk_audits
    _REC_SLOTS = 32           # pinned copies of the scalar record in flight (the host may enqueue that many iterations ahead)
    MAX_ITER_GRAPHS = 40      # live captured iterations (3 sources x 3 k x 2 buffer sets x 2 loss accumulators at most per shape)

    @property
    def graph_stats(self):
        """graph_iteration: {"captured": graphs captured so far, "replayed": iterations run as a graph replay, "eager": iterations run
        launch by launch (the first uses of a key, keys met while no capture is possible)}; skipped iterations count nowhere."""
        return dict(self._it_stats)

    stash_audit = property(lambda self: self._audits["stash"].every)      # (the schedules under their public names)
    trunk_audit = property(lambda self: self._audits["trunk"].every)
    stash_audits = property(lambda self: self._audits["stash"].reports)
    trunk_audits = property(lambda self: self._audits["trunk"].reports)
    last_stash_audit = property(lambda self: self._audits["stash"].last)
    last_trunk_audit = property(lambda self: self._audits["trunk"].last)

    def _audit_due(self):
        """The audits of the iteration about to run: a tuple of "trunk" / "stash" (empty: none)."""
        return tuple(kind for kind, sched in self._audits.items() if sched.due(self.iteration))

    def _run_audits(self, due, b, grads16):
        """The audits of the iteration in flight, in front of its optimiser launches: the latents and the slabs are the iteration's."""
        if "trunk" in due and grads16:
            self._trunk_audit(b, grads16)
        if "stash" in due:
            self._stash_audit(b)

    # ---- stash audit ------------------------------------------------------------------------------
    def audit_next(self):
        """Arm the stash audit for the next iteration that runs (a skipped iteration leaves it armed)."""
        ops.refuse_stash_audit(self.precision, capturing=False)
        self._audits["stash"].arm()

    def _stash_audit(self, b):
        """The audit of the iteration in flight, behind its weight-gradient launch and in front of its optimiser launch: census
        first (the 16-bit leg of the gap overwrites the stash), then the gap.  Reads its results back: synchronises."""
        net = self.net
        census = net.stash_census(b["bp"], b["n"])
        gap = net.stash_gap(b["bp"], b["coords"])
        worst = max(gap, key=gap.get)
        rep = {"iteration": int(self.iteration), "source": b["source"], "rows": int(b["n"]), "census": census,
               "tile_scale": dict(net.last_tile_scale), "grad_gap": gap, "worst": [worst, gap[worst]],
               "flags": ["saturated"] if saturated(census.values()) else []}
        return self._audits["stash"].record(rep)

    # ---- trunk audit -------------------------------------------------------------------------------
    def audit_trunk_next(self):
        """Arm the trunk audit for the next iteration that runs (a skipped iteration leaves it armed)."""
        ops.refuse_trunk_audit(self.trunk_precision, capturing=False, patch_losses=self.patch_sampler is not None)
        self._audits["trunk"].arm()

    def _trunk_twin(self, term):
        """The exact-fp32 twin of one patch-loss term, built on first use from the state dicts the fit was given."""
        tw = self._twins.get(term)
        if tw is None:
            sd = self._trunk_sd
            if term == "contextual":
                tw = ContextualLoss(use_vgg=True, vgg_state_dict=sd["vgg19"], device=self.device, trunk_precision="fp32").to(self.device)
            elif term == "lpips":
                tw = LPIPS(net="vgg", lin_weights=sd["lins"], vgg_state_dict=sd["vgg16"], device=self.device, trunk_precision="fp32")
            else:
                from .losses import StyleLoss
                tw = StyleLoss(vgg_state_dict=sd["style"], device=self.device, trunk_precision="fp32")
            self._twins[term] = tw
        return tw

    def _trunk_audit(self, b, grads):
        """The trunk audit of the iteration in flight, behind its backward launch and in front of its optimiser launches (the
        adaptive latents are still the ones its terms used).  grads: {term: the patch gradient dL/dxy the term returned} for the
        terms that ran ("contextual", "lpips" on 'same' iterations, "style" where the fit has one) -- the 16-bit leg.  The fp32 leg:
        the batch composed again from the iteration's prediction (npp_patch_compose_fwd into a buffer of the audit's own), the
        term's exact-fp32 twin with the fit's current latents and the iteration's scale, writing into a scratch loss word and the
        twin's own latent gradients.  Per term: dx_gap = rel_l2(dx16[:nk], dx32[:nk]), the census of every stored layer with the
        ReLU gates the two trunks disagree on, feat_gap = rel_l2(fp16 layer, fp32 layer) over the kept images, and the layer with
        the largest share of flipped gates.  Reported, not judged; "saturated" is exact (a value at 65504 or a non-finite one
        exists).  Reads its results back: synchronises."""
        ops.refuse_trunk_audit(self.trunk_precision, patch_losses=self.patch_sampler is not None)
        net, P, n_p, k, n_pix, n, raw = self.net, b["P"], b["n_p"], b["k"], b["n_pix"], b["n"], b["raw"]
        nk = n_p * k
        comp = self.use_comp and b["source"] == "val"
        xy = self._audit_xy.get((nk, P))
        if xy is None:
            if len(self._audit_xy) >= 8:
                self._audit_xy.clear()
            xy = self._audit_xy[(nk, P)] = torch.empty((2 * nk, 3, P, P), dtype=torch.float32, device=self.device)
        if self._audit_loss is None:
            self._audit_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        pred = net.workspace(b["bp"])["pred"]
        ops.patch_compose_fwd(pred[n_pix:n], raw["fake"], raw["fmask"], raw["real"], raw["rmask"], n_p, k, P, comp, xy)
        weight = b.get("weight")
        terms, kept = {}, {"xy": xy, "dx16": {}, "dx32": {}}
        for term, dx16 in grads.items():
            tw = self._trunk_twin(term)
            if term == "contextual":
                t16 = self.contextualLoss.hip_trunk
                dx32 = tw.fused(xy, nk, self.cx_w, self._audit_loss, weight=weight)
            elif term == "lpips":
                t16 = self.percepLoss.hip_trunk
                tw._lat.copy_(self.percepLoss._lat)
                tw.zero_latent_grads()
                dx32 = tw.fused(xy, nk, self.lp_w * (nk if weight is not None else 1), self._audit_loss, normalize=True,
                                use_robust=self.lp_robust)
            else:
                t16 = self.style.hip_trunk
                tw._lat.copy_(self.style._lat)
                tw.zero_latent_grads()
                dx32 = tw.fused(xy, nk, self.style_w, self._audit_loss)
            t32 = tw.hip_trunk
            layers = t16.census(ref=t32)
            gaps = [ops.rel_l2(dx16[:nk], dx32[:nk])]
            names = t16.layer_names()
            for j, (y, c, H, W) in enumerate(t16._geom):
                gaps.append(ops.rel_l2(ops.trunk_export(y, t16._N, nk, c, H, W, is_f16=True), t32._acts[j][:nk]))
            gaps = torch.stack(gaps).cpu().numpy()
            for name in layers:
                layers[name]["feat_gap"] = float(gaps[1 + names.index(name)]) if name in names else None
            worst_layer = max(names, key=lambda nm: layers[nm]["gate_flips"] / max(layers[nm]["elements"], 1))
            terms[term] = {"dx_gap": float(gaps[0]), "layers": layers, "worst_layer": worst_layer}
            kept["dx16"][term], kept["dx32"][term] = dx16, dx32
        worst = max(terms, key=lambda t: terms[t]["dx_gap"])
        rep = {"iteration": int(self.iteration), "source": b["source"], "patches": int(nk), "terms": terms,
               "worst": [worst, terms[worst]["dx_gap"]], "flags": ["saturated"] if any(ops.trunk_census_flags(t["layers"]) for t in terms.values()) else []}
        self.trunk_audit_tensors = kept                          # (device tensors of the newest audit: xy, both legs' dL/dxy; for tests)
        return self._audits["trunk"].record(rep)

    def lpips_branch(self, xy, nk, scale, loss_buf):
        """percepLoss.fused(xy, nk, scale, loss_buf) on the CURRENT stream (the loop's side stream).  The branch is 46 launches at the
        latency floor -- VGG16 on four 96 x 96 patches, 5 heads, the data-gradient pass -- and its 0.39 ms of host enqueue time made the
        'same' iterations host-bound (0.71 ms of enqueue against 0.60 ms of device time for the other sources).  From its third use on a
        given set of buffers it is therefore replayed as ONE captured HIP graph (torch.cuda.CUDAGraph over the same launches: arguments
        and buffers are fixed -- xy / loss_buf / latents are persistent tensors, scale and n_p k part of the key)."""
        lp = self.percepLoss
        # (every address and scalar a captured launch holds is part of the key: re-homed latents or buffers get a capture of their own)
        # -- incl. the stream (the heads' accumulators are per stream) and the trunk's choice of kernel forms
        key = (xy.data_ptr(), loss_buf.data_ptr(), int(nk), float(scale), self.lp_robust, lp._lat.data_ptr(), lp._dlat.data_ptr(),
               lp.lins[0].data_ptr(), lp.grouped_heads, lp.flat_tap_grads, int(lp.hip_trunk.fuse_pairs), lp.hip_trunk.fold_pool_bwd,
               lp.hip_trunk.fold_pool_fwd, ops._stream().value) if self.lp_graph else None
        ent = self._lp_graphs.get(key) if self.lp_graph else None
        if ent is not None and ent[0] is not None:
            ent[0].replay()
            lp.touched = lp.touched or self.lp_robust
            return ent[1]
        out = lp.fused(xy, nk, scale, loss_buf, normalize=True, use_robust=self.lp_robust)
        if not self.lp_graph:
            return out
        uses = 1 if ent is None else ent[2] + 1
        if ent is None and len(self._lp_graphs) >= 8:          # each capture keeps a private pool (taps + gradients): bound their number
            self._lp_graphs.pop(next(iter(self._lp_graphs)))
        self._lp_graphs[key] = (None, None, uses)
        if uses == 2:                                           # two eager passes have warmed every buffer / workspace: capture for the next use
            s = torch.cuda.current_stream(self.device)
            g = torch.cuda.CUDAGraph()
            try:                                                # (a capture only RECORDS the launches: nothing runs, no state changes)
                with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                    gout = lp.fused(xy, nk, scale, loss_buf, normalize=True, use_robust=self.lp_robust)
            except Exception as e:                             # a runtime that cannot capture: stay eager, say so once
                import warnings
                warnings.warn(f"npp_amd.fit: LPIPS branch not captured as a HIP graph ({e}); keeping the launch-by-launch form")
                self.lp_graph = self._graph_ok = False            # (nor a whole iteration: graph_iteration stays launch by launch, too)
                return out
            self._lp_graphs[key] = (g, gout, uses)
        return out

    # ---- sampling (train.py:172-181) -------------------------------------------------
    def draw_pixels(self):
        """np.random.choice(n_train, N_rand, replace=False) (train.py:172): host indices."""
        if self.fast_rng is not None:
            return self.fast_rng.choice(self.i_train.shape[0], size=self.N_rand, replace=False)
        return self.rng.choice(self.i_train.shape[0], size=[self.N_rand], replace=False)

    def sample_pixels(self):
        """-> coords (N_rand,2) on device."""
        return self.i_train_dev[ops.h2d(self.draw_pixels(), self.device)]

    def gather_gt(self, coords):
        return self.masked_img[coords[:, 0].long(), coords[:, 1].long()].contiguous()

    # ---- one optimisation iteration (pixel loss; patch losses are added by the caller) ----
    def step(self, coords=None, extra_coords=None, patch_loss=None):
        """coords: pixel-loss rows (sampled when None).  extra_coords: rows of the predicted
        patches appended after them (train.py:181); patch_loss(pred_patch_rows, dpred_patch_rows)
        must fill dL/dpred for those rows and return nothing (its kernels accumulate)."""
        net = self.net
        if coords is None:
            coords = self.sample_pixels()
        n_pix = coords.shape[0]
        allc = coords if extra_coords is None else torch.cat([coords, extra_coords], 0)
        n = allc.shape[0]
        bp = ops.pad_rows(n)
        if bp != n:
            allc = torch.cat([allc, allc.new_zeros((bp - n, 2))], 0)
        ws = net.workspace(bp)
        net.zero_grad()                                  # optimizer.zero_grad() (train.py:192)
        pred = net.forward_train(allc.contiguous())
        if n_pix < bp:
            ws["dpred"][n_pix:].zero_()
        gt = self.gather_gt(coords)
        net.pixel_loss(bp, n_pix, gt)                    # img2mse(pred[:N_rand], gt, ...) (train.py:195)
        if patch_loss is not None:
            patch_loss(pred[n_pix:n], ws["dpred"][n_pix:n])
        net.backward(bp)                                 # loss.backward()
        net.optimizer_step(bp)                           # optimizer.step() + LR rule + global_step
        self.iteration += 1
        return net.loss_buf

    # ---- one iteration of the complete loop body, train.py:133-264 ------------------------
    def step_full(self):
        """Patch sampling -> pixel sampling -> fused forward -> pixel loss + contextual loss
        (+ LPIPS when patch_source == 'same') -> backward -> Adam.  Returns False when the
        sampler found no valid real patch: the iteration is skipped BEFORE zero_grad and
        global_step is not advanced (train.py:160-161)."""
        assert self.patch_sampler is not None, "construct CompletionFit with shifts=... for the patch losses"
        if self.rng_mode == "device":
            return self._step_full_device()
        if self._prefetch > 0:
            if self._producer is None:
                self._start_producer()
            d = self._queue.get()
            if isinstance(d, BaseException):
                raise d
        else:
            d = self.draw_batch()
        if self._prefetch > 0 and self.side_sampler:
            # With the producer thread the draws run ahead anyway; the sampler's DEVICE half (one upload, the crop gather, the row
            # assembly: ~35 us of launches) then runs ahead too, on a side stream under the previous iteration's kernels instead of
            # in front of this one's (round 5: end to end 0.683 -> 0.65 ms at c2).  It reads constants only (image, mask, pools).
            cur = self._ahead if self._ahead is not None else self._materialise_ahead(d)
            nxt_d = d if self._ahead is not None else self._next_draw()
            self._ahead = None                                    # consumed: a step that raises must not be replayed by the next call
            d, batch, ev = cur
            self.last_draw = d
            self.iteration += 1
            try:
                if batch is not None:
                    torch.cuda.current_stream(self.device).wait_event(ev)
                    self.step_from(batch)
                else:
                    self.skipped += 1
            finally:
                # the draw already taken from the queue belongs to the NEXT iteration whatever happened to this one: a caller that
                # catches the exception and goes on keeps the reference's random stream (as StackedFit.step_full does)
                self._ahead = self._materialise_ahead(nxt_d)      # (behind this iteration's launches in the host's order)
            return batch is not None
        self.last_draw = d                                        # host-side record of this iteration's draws (tests, logging)
        batch = self.materialise_batch(d)
        self.iteration += 1
        if batch is None:
            self.skipped += 1
            return False
        self.step_from(batch)
        return True

    def _step_full_device(self):
        """step_full() of rng_mode "device": the draws are launches on the sampler stream.  Iteration i + 1 is materialised there
        (record read, crop gather, pixel rows, row assembly) right behind the launches of iteration i, and the decision of
        iteration i + 2 is enqueued behind that -- so the host's read of (source, k) waits on work enqueued a whole iteration
        earlier and the main stream never waits for a draw that has not long run."""
        cur = self._ahead if self._ahead is not None else self._materialise_device()
        self._ahead = None
        d, batch, ev = cur
        self.last_draw = d
        self.iteration += 1
        try:
            if batch is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
                self.step_from(batch)
            else:
                self.skipped += 1
        finally:
            self._ahead = self._materialise_device()              # (the draw index has advanced whatever happened to this iteration)
        return batch is not None

    def device_draws(self):
        if self._dev_draws is None:
            from .dev_sampler import DeviceDraws
            self._dev_draws = DeviceDraws([self])
        return self._dev_draws

    def _materialise_device(self):
        """The next draw + its batch on the sampler stream -> (d, batch | None, event), then the decision launch of the draw after
        it (unless a patch-size decay comes first)."""
        dd = self.device_draws()
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(dd.stream):
            d = self.draw_batch()
            b = self.materialise_batch(d)
            ev = torch.cuda.Event()
            ev.record(dd.stream)
            dd.launch_ahead()
        self._hand_over_batch(b, main)
        return d, b, ev

    def _hand_over_batch(self, b, main):
        st = None if b is None else b.get("set")
        if st is None:
            _hand_over(b, main)
        elif not st["handed"]:                                    # persistent buffers (graph_iteration): once, not per iteration
            _hand_over([v for v in st.values() if isinstance(v, torch.Tensor)], main)
            st["handed"] = True

    def _next_draw(self):
        d = self._queue.get()
        if isinstance(d, BaseException):
            raise d
        return d

    def _materialise_ahead(self, d):
        """materialise_batch(d) on the sampler's own stream -> (d, batch | None, event); the batch's tensors are handed to the main
        stream (record_stream: the allocator must not recycle them while the iteration still reads them)."""
        if d["k"] == 0:
            return d, None, None
        main = torch.cuda.current_stream(self.device)
        if self._s_smp is None:
            self._s_smp = torch.cuda.Stream(self.device)
            self._s_smp.wait_stream(main)                         # the constructor's uploads
        with torch.cuda.stream(self._s_smp):
            b = self.materialise_batch(d)
            ev = torch.cuda.Event()
            ev.record(self._s_smp)
        self._hand_over_batch(b, main)
        return d, b, ev

    def decay_due(self):
        """Whether the NEXT draw_batch() halves the patch size first (train.py:137-141: by iteration index, trange(start=1))."""
        i = self._draw_iter + 1
        return (self.patch_sampler is not None and i % self.patch_size_decay == 0 and i != 1 and self.patch_size > 31
                and getattr(self, "_decayed_at", None) != i)

    def apply_decay(self):
        """The patch-size decay of the next iteration, now (a StackedFit re-forms around the new batch shape before it draws)."""
        self._decayed_at = self._draw_iter + 1
        self.patch_size //= 2
        self.patch_num *= 2
        self.patch_sampler.reset_patchsize(None, None, self.patch_size, self.patch_num)
        self.patch_sampler.reset_pool(self.i_train, self.i_val)

    # ---- host half of one iteration's sampling (no device work: may run ahead on the producer thread) -------------
    def draw_batch(self):
        """train.py:137-141 (patch-size decay, by iteration index), :152-157 (sample_patches) and :172 (pixel draw), in the
        reference's RNG order.  One call per loop iteration, including the ones that end up skipped."""
        if self.decay_due():
            self.apply_decay()
        if self.rng_mode == "device":
            # the record of the decision launch (enqueued by the previous materialisation, or now) and, for a draw that is not
            # skipped, the pixel-row launch -- both on the sampler stream; the caller's stream waits for them
            dd = self.device_draws()
            cur = torch.cuda.current_stream(self.device)
            d = dd.take()[0]
            d["n_p"] = self.patch_num
            if d["k"] > 0:
                with torch.cuda.stream(dd.stream):
                    pix = torch.empty((1, self.N_rand), dtype=torch.int64, device=self.device)
                    d["pix"] = dd.pixels([d], pix)[0]
            if cur != dd.stream:
                cur.wait_stream(dd.stream)
            return d
        self._draw_iter += 1
        d = self.patch_sampler.draw(topk=self.topk, invalid_ratio=self.invalid_ratio)
        d["n_p"] = self.patch_num
        if d["k"] > 0:
            d["pix"] = self.draw_pixels()                         # the reference `continue`s before this draw when k == 0
        return d

    def materialise_batch(self, d, out=None):
        """Device half: crops, coordinates, ground-truth colours of a draw_batch().  None when no valid real patch exists.
        out: dict(coords, gt, crops, cmasks[, pmask]) of preallocated buffers (this image's slices of a StackedFit's arrays)."""
        # (want_tuple=False: the loop reads the contiguous crops of last_raw; the reference-shaped views / tiled copies of the
        #  8-tuple would cost two more launches per iteration)
        if d["k"] == 0:
            return None
        st = None
        if out is None and self.graph_iteration:                  # a captured iteration reads its batch at fixed addresses
            st = out = self._batch_set(d)
        # ONE host -> device transfer per iteration: [pixel-row indices (int64) | patch centres (int32)] through one pinned block
        if d.get("device"):                                       # rng_mode "device": both are where the launches wrote them
            pix_dev, cen_dev = d["pix"], d["cen_dev"]
        else:
            pix = np.ascontiguousarray(d["pix"], np.int64)
            cen = self.patch_sampler.centres_i32(d)
            blob = np.concatenate([pix.view(np.uint8).reshape(-1), cen.view(np.uint8).reshape(-1)])
            blob_dev = ops.h2d(blob, self.device)
            pix_dev = blob_dev[:pix.nbytes].view(torch.int64)
            cen_dev = blob_dev[pix.nbytes:].view(torch.int32).reshape(-1, 2)
        _, _, _, _, _, source, k, weight = self.patch_sampler.materialise(d, want_coords=False, want_tuple=False, cen_dev=cen_dev,
                                                                          crops_out=None if out is None else (out["crops"], out["cmasks"]))
        # coordinates of all rows (N_rand pixel rows, then the fake patches' rows, zero padding) + the pixel rows' colours:
        # one launch (npp_batch_assemble) instead of two index gathers, two concatenations and the colour / mask gathers
        n_pix, P, n_p = d["pix"].shape[0], d["P"], d["cen"].shape[0]
        n = n_pix + n_p * P * P
        bp = ops.pad_rows(n)
        allc, gt, pm = ops.batch_assemble(self.i_train_dev, pix_dev, self.patch_sampler.last_cen_dev, P, bp,
                                          self.masked_img, self.pixel_mask,
                                          out=None if out is None else (out["coords"], out["gt"], out.get("pmask")))
        w_dev = None
        if self.use_patch_weight and d["weights"] is not None:
            # (device draws: the record's weights, copied out of the record ring on the sampler stream)
            w_dev = d["w_dev"].clone() if d.get("device") else ops.h2d(np.ascontiguousarray(d["weights"], np.float32), self.device)
            if st is not None:
                w_dev = st["weight"][:w_dev.numel()].copy_(w_dev.reshape(-1)).view(w_dev.shape)
        return dict(set=st, coords=allc, n_pix=n_pix, n=n, bp=bp, gt=gt, source=source, k=k, P=P, n_p=d["n_p"],
                    raw=self.patch_sampler.last_raw, pmask=pm, weight=w_dev)

    def sample_batch(self):
        """Host-side sampling of one iteration + its device half.  None when no valid real patch exists."""
        return self.materialise_batch(self.draw_batch())

    def _start_producer(self):
        import queue
        import threading
        self._queue = queue.Queue(maxsize=self._prefetch)

        def run():
            try:
                while not self._stop:
                    d = self.draw_batch()
                    while not self._stop:
                        try:
                            self._queue.put(d, timeout=0.1)
                            break
                        except queue.Full:
                            continue
            except BaseException as e:                            # surface sampler errors in the training thread
                self._queue.put(e)
        self._producer = threading.Thread(target=run, name="npp-sampler", daemon=True)
        self._producer.start()

    def close(self):
        """Stop the producer thread (if any)."""
        self._stop = True
        if self._producer is not None:
            self._producer.join(timeout=2.0)
            self._producer = None

    def __del__(self):
        self._stop = True

    def step_from(self, b):
        """Device side of one iteration (everything after sampling), train.py:183-264, as explicit kernel
        launches (no autograd): fused forward -> pixel loss -> patch plumbing (npp_patch_compose_fwd) -> VGG19 trunk
        -> contextual loss core -> trunk data-gradient (-> the same through VGG16 / LPIPS head on 'same' iterations)
        -> npp_patch_compose_bwd -> backward chain + wgrad -> Adam."""
        ops.check_current(self.device)
        if self.graph_iteration:
            return self._step_from_graph(b)
        self._select_xy(b["n_p"] * b["k"], b["P"])
        self.net.zero_grad()
        if self.percepLoss.touched:
            self.percepLoss.zero_latent_grads()
        self._launch_iteration(b, audit=self._audit_due())

    def _select_xy(self, nk, P):
        key = (nk, P)
        if self._xy_key != key:                                   # one fp32 batch buffer per (n_p k, P): fixed addresses (see lpips_branch)
            if key not in self._xy_bufs:
                if len(self._xy_bufs) >= 8:                       # (the patch size changes every patch_size_decay iterations)
                    self._xy_bufs.clear()
                    self._lp_graphs.clear()
                    self._drop_graphs()                           # (captured iterations hold the buffers' addresses too)
                self._xy_bufs[key] = torch.empty((2 * nk, 3, P, P), dtype=torch.float32, device=self.device)
            self._xy, self._xy_key = self._xy_bufs[key], key

    def _launch_iteration(self, b, hp=None, capture=False, audit=()):
        """The launches of one iteration behind zero_grad(), on the current stream (+ the LPIPS side stream).  hp None: the loop's
        form -- step-dependent scalars as kernel arguments, the host's counters advanced on the way.  hp = the scalar record on the
        device (graph_iteration): the same launches with the optimisers' scalars read from hp[0:2] (network + pixel-loss latents)
        and hp[2:4] (LPIPS latents) and NO step counter touched -- what a capture records (capture=True: the LPIPS branch as its
        launches, too; outside a capture it goes through lpips_branch exactly as in the loop's form: a launch-by-launch iteration
        of a graph-mode fit is the eager iteration launch for launch)."""
        audit_trunk = "trunk" in audit
        self.last_source = source = b["source"]
        net, P, n_p, k, n_pix, n, bp = self.net, b["P"], b["n_p"], b["k"], b["n_pix"], b["n"], b["bp"]
        raw = b["raw"]
        comp = self.use_comp and source == "val"                 # train.py:230-231
        nk = n_p * k
        with_lp = source == "same" and self.use_perceptual_loss
        cx = self.contextualLoss
        xy = self._xy if (with_lp or self.style is not None) else None      # fp32 batch only when another trunk reads it
        sc, sh = cx.input_norm()
        main = torch.cuda.current_stream(self.device)
        t32 = self.trunk_precision == "fp32"
        fold = self.fold_launches and not t32                    # (the bf16 MLP keeps its patch-folded backward launch: fold_bwd below)
        fold_bwd = self.fold_launches
        if t32:
            xy = self._xy                                         # the fp32 batch is what the fp32 trunks read
        ws = net.workspace(bp)
        pred = net.forward_train(b["coords"])
        net.clear_dpred_tail(bp, n)
        # The consumers of the prediction are independent and each under-fills the chip (small grids, dependent
        # launches): on 'same' iterations the LPIPS branch runs on a side stream next to the contextual branch and
        # joins before npp_patch_compose_bwd (1.30 -> 1.17 ms).  Measured negative (event record / wait costs more than is
        # hidden): the 12 us pixel loss on a side stream (0.742 -> 0.762 ms per 'val' iteration); the real half of the
        # contextual batch through its own trunk instance on a side stream beside the MLP forward (0.767 -> 0.776 ms).
        # one launch: the adaptive pixel loss of the pixel rows + patch plumbing -> the contextual trunk's flat fp16 input
        # (normalised), the patch-loss accumulator cleared on the way (fold_launches = False: the separate launches, kept as
        # the comparator of tests/test_gpu_parity.py and for A/B timing)
        if not fold:
            net.pixel_loss(bp, n_pix, b["gt"], mask=b.get("pmask"), weight=self.pix_w)
        # Iterations whose other consumers need no fp32 copy of the batch ('val' / 'train' without a style term): the patch plumbing
        # and the pixel loss ride inside the trunk's first launch (ops.conv_pair_fwd_patch) -- no npp_trunk_patch_in launch at all
        x0_src = None
        if t32:                                                   # npp_patch_compose_fwd -> the fp32 batch; no flat trunk input
            ops.patch_compose_fwd(pred[n_pix:n], raw["fake"], raw["fmask"], raw["real"], raw["rmask"], n_p, k, P, comp, xy)
            self.patch_loss_buf.zero_()
        elif fold and xy is None and self.use_contextual_loss and cx.hip_trunk.can_compose_input(P, P):
            x0_src = dict(patch=(pred[n_pix:n], raw["fake"], raw["fmask"], raw["real"], raw["rmask"], n_p, k, P, comp),
                          zero=self.patch_loss_buf, loss=net.pixel_loss_args(bp, n_pix, b["gt"], mask=b.get("pmask"), weight=self.pix_w))
        else:
            ops.trunk_patch_in(pred[n_pix:n], raw["fake"], raw["fmask"], raw["real"], raw["rmask"], n_p, k, P, comp, sc, sh,
                               cx.hip_trunk.input_buffer(2 * nk, P, P), xy, self.patch_loss_buf, which=0,
                               loss=net.pixel_loss_args(bp, n_pix, b["gt"], mask=b.get("pmask"), weight=self.pix_w) if fold else None)
        dx_b = None
        # use_patch_weight (train.py:224-250): contextual term sum_i -log(cx_i w_i + 1e-5) (the core's weighted form), LPIPS term
        # sum_i d_i w_i -- on 'same' iterations the weights are all 1 (sampler.py:338), i.e. nk times the mean
        weight = b.get("weight")
        if with_lp:                                                                                 # train.py:241-250
            self._s_lp.wait_stream(main)
            with torch.cuda.stream(self._s_lp):
                if not capture and not audit_trunk:
                    dx_b = self.lpips_branch(xy, nk, self.lp_w * (nk if weight is not None else 1), self.patch_loss_buf)
                else:                                             # (inside a capture the branch is recorded as its launches, not as
                    #                                               a replay of its own graph; a trunk audit reads what THIS pass of
                    #                                               the trunk stored: the same launches, outside lpips_branch's graphs)
                    dx_b = self.percepLoss.fused(xy, nk, self.lp_w * (nk if weight is not None else 1), self.patch_loss_buf,
                                                 normalize=True, use_robust=self.lp_robust)
        # the backward chain that follows streams this pack: requested into L2 early (bf16 chain only)
        cx.hip_trunk.final_next_pack = net.wb if net.precision == "bf16" else None
        if self.use_contextual_loss and t32:
            dx_a = cx.fused(xy, nk, self.cx_w, self.patch_loss_buf, weight=weight)
        elif self.use_contextual_loss:
            dx_a = cx.fused((2 * nk, 3, P, P), nk, self.cx_w, self.patch_loss_buf, weight=weight, x0_ready=True, x0_src=x0_src)   # train.py:238-239
        else:                                                                                       # ablation: no contextual term
            dx_a = torch.zeros((2 * nk, 3, P, P), dtype=torch.float32, device=self.device)
        if dx_b is not None:
            main.wait_stream(self._s_lp)
        grads16 = {}
        if audit_trunk:                                           # each term's patch gradient as the term returned it
            if self.use_contextual_loss:
                grads16["contextual"] = dx_a
            if dx_b is not None:                                  # (a copy where the style term is added in place below)
                grads16["lpips"] = dx_b.clone() if self.style is not None else dx_b
        if self.style is not None:                                                                  # NPP_remapping/train.py:253-261
            self.style.zero_latent_grads()
            dx_s = self.style.fused(xy, nk, self.style_w, self.patch_loss_buf)
            if audit_trunk:
                grads16["style"] = dx_s
            dx_b = dx_s if dx_b is None else dx_b.add_(dx_s)
        self.last_patch_loss = self.patch_loss_buf
        lr_used = net.lr
        if hp is not None:                                        # (graph_iteration: bf16 MLP, fp16 trunks, folded launches, no style term)
            net.backward(bp, patch=(dx_a, dx_b, raw["fmask"], raw["rmask"], n_pix, n_p, k, P, comp))
            self._run_audits(audit, b, grads16)
            net.optimizer_launch_dev(bp, hp[0:2])
            if self.percepLoss.touched:
                self.percepLoss.adam_launch_dev(hp[2:4])
            return
        # npp_patch_compose_bwd folded into the backward launch: dL/dpred of the patch rows is formed (and written) there
        if fold_bwd:
            net.backward(bp, patch=(dx_a, dx_b, raw["fmask"], raw["rmask"], n_pix, n_p, k, P, comp))
        else:
            ops.patch_compose_bwd(dx_a, dx_b, raw["fmask"], raw["rmask"], n_p, k, P, comp, ws["dpred"][n_pix:n])
            net.backward(bp)
        self._run_audits(audit, b, grads16)
        net.optimizer_step(bp)
        if self.percepLoss.touched:                               # only 'same' iterations give them a gradient
            self.percepLoss.adam_step(lr_used)
        if self.style is not None:                                # the style latents are in the same optimiser (helpers.py:153-159)
            self.style.adam_step(lr_used)

    # ---- graph_iteration: the device side of an iteration as one captured HIP graph --------------------------------------
    def _batch_set(self, d):
        """The persistent buffers the next batch is materialised into (materialise_batch(out=...), the StackedFit form).  Two sets
        per batch shape where the sampler's device half runs an iteration ahead on its own stream (producer thread, device draws):
        the stream that fills a set first waits for the iteration that read it last.  One set where the batch is formed on the
        loop's own stream, in order.  The sets of an earlier patch size stay allocated (a fit sees three sizes at most)."""
        P, n_p, n_pix = d["P"], d["n_p"], self.N_rand
        sets = self._sets.get((P, n_p))
        if sets is None:
            bp, nc, dev, f32 = ops.pad_rows(n_pix + n_p * P * P), n_p * (1 + self.topk), self.device, torch.float32
            sets = self._sets[(P, n_p)] = [dict(
                idx=i, coords=torch.zeros((bp, 2), dtype=torch.int32, device=dev), gt=torch.zeros((n_pix, 3), dtype=f32, device=dev),
                crops=torch.zeros((nc, 3, P, P), dtype=f32, device=dev), cmasks=torch.zeros((nc, 1, P, P), dtype=f32, device=dev),
                weight=torch.zeros(n_p * self.topk, dtype=f32, device=dev), free=None, handed=False) for i in range(2)]
        ahead = self.rng_mode == "device" or (self._prefetch > 0 and self.side_sampler)
        st = sets[self._wset if ahead else 0]
        if ahead:
            self._wset ^= 1
            if st["free"] is not None:
                torch.cuda.current_stream(self.device).wait_event(st["free"])
        return st

    def _drop_graphs(self, keep=None):
        """Release captured iterations (all, or those `keep` rejects) with their private pools -- behind everything enqueued."""
        gone = [k for k in self._it_graphs if keep is None or not keep(k)]
        if any(self._it_graphs[k][0] is not None for k in gone):
            torch.cuda.synchronize(self.device)
        for k in gone:
            del self._it_graphs[k]

    def _step_from_graph(self, b):
        """step_from() of graph_iteration=True.  A stream capture cannot begin on the default stream: called there, the iteration
        runs on a stream of the fit's own, joined on both sides (a loop that wants the bare graph launch runs under
        torch.cuda.stream(...), as train.py does)."""
        main = torch.cuda.current_stream(self.device)
        if main != torch.cuda.default_stream(self.device):
            return self._graph_iteration(b, main)
        if self._s_it is None:
            self._s_it = torch.cuda.Stream(self.device)
        self._s_it.wait_stream(main)
        with torch.cuda.stream(self._s_it):
            self._graph_iteration(b, self._s_it)
        main.wait_stream(self._s_it)

    def _graph_iteration(self, b, stream):
        """One iteration on `stream` (not the default stream): what alternates or changes from step to step stays OUTSIDE the graph --
        zero_grad()'s switch of the loss accumulator (a host index: the accumulator is part of the key), the fill of the LPIPS
        latents' gradient after a 'same' iteration, the dpred tail rule, and the scalar record: (step_size, 1 / sqrt(1 - b2^t)) of
        the network's and of the LPIPS latents' optimiser, computed on the host exactly as the argument forms of the launches do
        (ops.adam_words) and copied into four device words in front of the replay.  Then ONE replay of the graph of this key -- or,
        for the first two uses of a key, the same launches eagerly (_launch_iteration(hp=record)); the second use also captures
        them (a capture only records).  Afterwards the host's counters are advanced once, as the eager loop leaves them."""
        net, lp, cx = self.net, self.percepLoss, self.contextualLoss.hip_trunk
        source, P, n_p, k, n, bp = b["source"], b["P"], b["n_p"], b["k"], b["n"], b["bp"]
        nk = n_p * k
        if self._it_shape != (P, n_p):                            # patch-size decay: the graphs of the old shape go
            self._drop_graphs(keep=lambda key: key[0] == (P, n_p))
            self._it_shape = (P, n_p)
        self._select_xy(nk, P)
        net.zero_grad()
        if lp.touched:
            lp.zero_latent_grads()
        ws = net.workspace(bp)
        net.clear_dpred_tail(bp, n)
        with_lp = source == "same" and self.use_perceptual_loss
        comp = self.use_comp and source == "val"
        # ---- the scalar record
        i = self._rec_i
        self._rec_i = (i + 1) % self._REC_SLOTS
        if self._rec_ev[i] is not None:
            self._rec_ev[i].synchronize()                         # (long complete unless the host runs _REC_SLOTS iterations ahead)
        w = self._rec_np[i]
        w[0], w[1] = net.step_words()
        w[2], w[3] = lp.step_words(net.lr)
        self._rec.copy_(self._rec_pin[i], non_blocking=True)
        # ---- every address and scalar a captured launch holds: shape, k, source (-> comp, LPIPS branch), buffer set, loss accumulator,
        # fp32 batch buffer, stream (per-stream workspaces), and the switches lpips_branch's key carries
        st = b["set"]
        key = ((P, n_p), k, source, comp, with_lp, st["idx"], st["coords"].data_ptr(), net._loss_idx, self._xy.data_ptr(), ws["pred"].data_ptr(),
               b.get("weight") is not None, self.lp_robust, lp._lat.data_ptr(), lp.grouped_heads, lp.flat_tap_grads,
               int(lp.hip_trunk.fuse_pairs), lp.hip_trunk.fold_pool_bwd, lp.hip_trunk.fold_pool_fwd, int(cx.fuse_pairs), cx.fold_pool_bwd,
               cx.fold_pool_fwd, ops.DETERMINISTIC, stream.cuda_stream)
        ent = self._it_graphs.get(key)
        due = self._audit_due()
        if due:
            # an audited iteration runs launch by launch (the audit sits between two of its launches and reads back on the host);
            # it is no use of the key: captures and replays go on around it as if it had not been audited
            self._launch_iteration(b, hp=self._rec, audit=due)
            self._it_stats["eager"] += 1
        elif ent is not None and ent[0] is not None:
            ent[0].replay()
            self._it_stats["replayed"] += 1
            self.last_source, self.last_patch_loss = source, self.patch_loss_buf
            if with_lp and self.lp_robust:
                lp.touched = True
        else:
            self._launch_iteration(b, hp=self._rec)
            self._it_stats["eager"] += 1
            uses = 1 if ent is None else ent[1] + 1
            if ent is None and len(self._it_graphs) >= self.MAX_ITER_GRAPHS:   # each capture keeps a private pool: bound their number
                oldest = next(iter(self._it_graphs))
                self._drop_graphs(keep=lambda key_: key_ != oldest)
            self._it_graphs[key] = (None, uses)
            if uses == 2 and self._graph_ok:                      # two eager passes have created every lazy workspace: capture for the next
                g = torch.cuda.CUDAGraph()
                try:                                              # (a capture only RECORDS: nothing runs, no counter moves)
                    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                        self._launch_iteration(b, hp=self._rec, capture=True)
                except Exception as e:                            # a runtime that cannot capture: stay eager, say so once
                    import warnings
                    warnings.warn(f"npp_amd.fit: iteration not captured as a HIP graph ({e}); keeping the launch-by-launch form")
                    self._graph_ok = self.lp_graph = False          # (the LPIPS branch would fail, and warn, the same way)
                else:
                    self._it_graphs[key] = (g, uses)
                    self._it_stats["captured"] += 1
        # ---- the host's side of optimizer.step(): what the eager loop leaves
        net.optimizer_advance()
        if lp.touched:
            lp.adam_advance()
        ev = torch.cuda.Event()
        ev.record(stream)
        self._rec_ev[i] = st["free"] = ev

    # ---- checkpoint / resume (the reference has none: start = 0, helpers.py:166) ----------------
    def state_dict(self):
        """Everything that determines the continuation of the fit: parameters + Adam moments + step counters of the network and
        of every adaptive-loss latent group, the LR clock, the patch-size schedule and the position of the random streams.
        Host tensors / NumPy arrays; not available while a producer thread is running ahead (prefetch > 0)."""
        if self._producer is not None:
            raise RuntimeError("state_dict() with an active producer thread: the random stream is ahead of the fit; use prefetch=0")
        net = self.net
        sd = {"net": {k: getattr(net, k).detach().cpu().clone() for k in ("params", "m", "v", "latents", "lat_m", "lat_v")},
              "net_steps": (net.global_step, net.opt_step, net.lr), "iteration": self.iteration, "draw_iter": self._draw_iter,
              "rng_mode": self.rng_mode,
              "skipped": getattr(self, "skipped", 0), "rng": self.rng.get_state(),
              "fast_rng": None if self.fast_rng is None else self.fast_rng.bit_generator.state}
        if self.rng_mode == "device":
            # t, the index of the next draw the LOOP takes: a draw materialised ahead (step_full) is not part of the state -- it is a
            # pure function of (seed, t) and is drawn again.  (The patch-size decay it may have applied already is: decayed_at.)
            sd["t"] = sd["draw_iter"] = self._draw_iter - (1 if self._ahead is not None else 0)
            sd["decayed_at"] = getattr(self, "_decayed_at", None)
        if self.patch_sampler is not None:
            sd["patch"] = (self.patch_size, self.patch_num)
            lp = self.percepLoss
            sd["lpips"] = {"latents": [t.cpu().clone() for t in lp.latents], "m": [t.cpu().clone() for t in lp.lat_m],
                           "v": [t.cpu().clone() for t in lp.lat_v], "step": lp.lat_step}
            if self.style is not None:
                st = self.style
                sd["style"] = {"latents": [t.cpu().clone() for t in st.latents], "m": [t.cpu().clone() for t in st.lat_m],
                               "v": [t.cpu().clone() for t in st.lat_v], "step": st.lat_step}
        return sd

    def load_state_dict(self, sd):
        if self._producer is not None:
            raise RuntimeError("load_state_dict() with an active producer thread")
        if self.rng_mode == "device" and sd.get("rng_mode") != "device":
            raise ValueError("load_state_dict: a rng_mode='device' fit continues a device-mode fit's sequence only")
        net = self.net
        for k, v in sd["net"].items():
            getattr(net, k).copy_(v.to(self.device))
        net.global_step, net.opt_step, net.lr = sd["net_steps"]
        net.repack()
        net._clean = False
        self.iteration, self._draw_iter, self.skipped = sd["iteration"], sd["draw_iter"], sd["skipped"]
        if self.rng_mode == "device":
            self._draw_iter, self._ahead, self._decayed_at = sd["t"], None, sd.get("decayed_at")
        self.rng.set_state(sd["rng"])
        if self.fast_rng is not None and sd["fast_rng"] is not None:
            self.fast_rng.bit_generator.state = sd["fast_rng"]
        if self.patch_sampler is not None and "patch" in sd:
            if (self.patch_size, self.patch_num) != tuple(sd["patch"]):
                self.patch_size, self.patch_num = sd["patch"]
                self.patch_sampler.reset_patchsize(None, None, self.patch_size, self.patch_num)
                self.patch_sampler.reset_pool(self.i_train, self.i_val)
            for obj, key in ((self.percepLoss, "lpips"), (self.style, "style")):
                if obj is not None and key in sd:
                    for dst, src in zip(obj.latents, sd[key]["latents"]):
                        dst.copy_(src.to(self.device))
                    for dst, src in zip(obj.lat_m, sd[key]["m"]):
                        dst.copy_(src.to(self.device))
                    for dst, src in zip(obj.lat_v, sd[key]["v"]):
                        dst.copy_(src.to(self.device))
                    obj.lat_step = sd[key]["step"]

    # ---- evaluation (train.py:270-331) -----------------------------------------------
    @torch.no_grad()
    def render_image(self):
        """Full H x W grid through the fused forward: the 'fitted pixels/s' pass."""
        render = self.net.render_fp32 if self.net.precision == "fp32" else self.net.render
        return render(self.i_all_dev).reshape(self.H, self.W, 3)

    def save_model(self, path, **meta):
        """The fitted network as a model file (modelfile.py), for render.py / NPPNet.load: weights, adaptive latents, embedder
        configuration, plus the task and the iteration count as metadata.  Not a checkpoint: state_dict() is the one to resume from."""
        self.net.save(path, **{"task": self.task, "iterations": self.iteration, **meta})

    def psnr(self, region="known"):
        """-10 log10 MSE over known / unknown pixels against the clean image."""
        pred = self.render_image()
        m = self.mask if region == "known" else (1.0 - self.mask)
        d2 = ((pred - self.img) ** 2) * m
        mse = d2.sum() / (m.sum() * 3).clamp_min(1.0)
        return float(-10.0 * math.log10(max(float(mse), 1e-20)))
