"""Completion driver: what `python NPP_completion/train.py --datadir D --basedir B --p_topk K` does (run_completion.sh:13),
on the HIP path.

    python -m npp_amd.train --datadir data/completion/detected/<name> --basedir ./results --p_topk 3

Reads config.odgt + PNGs (npp_amd.io), builds the net with torch's default nn.Linear init and Gaussian Fourier
frequencies drawn from torch's global generator like the reference (models/embedder.py:26, models/networks.py:40-49;
seed with --seed), runs N_iters iterations of the complete loop body (CompletionFit.step_full) and writes
results/<expname>_top<K>/<name>/testset_<iter>/*.png every --i_testset iterations (train.py:270-328).
Flags keep the reference's names and defaults (options/arg_config.py:10-36,55-100), --netwidth included: the default is the
reference's 512 (the second fused build, libnpp_hip_w512.so); BASELINE.json's configurations are --netwidth 256.
"""
import argparse
import collections
import functools
import os
import time

import numpy as np
import torch

from .audit import at_limits, audit_dumps, refuse as refuse_audit


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="completion", choices=["completion", "remapping", "segmentation"],
                    help="completion: NPP_completion/train.py; remapping: NPP_remapping/train.py (whole image trained, blur-detected clear "
                         "mask as sampler / pixel-weight mask, Gram style loss; its defaults: contextual_weight 0.01, style_weight 1, no LPIPS); "
                         "segmentation: NPP_segmentation/train.py (fit on the masked-blurred image with the initial periodic region as "
                         "the known mask, constant LR, contextual_weight 0.005, no LPIPS, 601 iterations, then the L1 + LPIPS(alex) "
                         "criteria; needs period_mask.png / non_period_mask.png beside config.odgt)")
    ap.add_argument("--alexnet", default=None, help="torchvision alexnet state_dict (.pth) for the segmentation criterion")
    ap.add_argument("--lpips_alex_lin", default=None, help="lpips weights/v0.1/alex.pth (segmentation criterion)")
    ap.add_argument("--l1_thresh", type=float, default=0.15)
    ap.add_argument("--lpips_thresh", type=float, default=0.3)
    ap.add_argument("--lpips_layers", type=int, default=1)
    ap.add_argument("--blur_thresh", type=float, default=50)
    ap.add_argument("--blur_detection", default="host", choices=["host", "gpu"],
                    help="remapping: where the clear / blurry mask (NPP_remapping/blur_detection.py) is computed.  host: io.get_blur_map "
                         "(one batched LAPACK SVD per image row); gpu: npp_amd.blur on --device (the same mask)")
    ap.add_argument("--components", default="host", choices=["host", "gpu"],
                    help="segmentation: where the connected-component work runs -- the per-pixel half of the SLIC connectivity repair "
                         "(init_segment.enforce_connectivity) and the hole filling / small-object removal of the final non-periodic mask.  "
                         "host: SciPy (default); gpu: npp_amd.regions on --device (the same labels and masks)")
    ap.add_argument("--init_segmentation", default="auto", choices=["file", "auto", "compute"],
                    help="segmentation: where the initial periodic / non-periodic masks (loaders.py:162-205) come from.  file: "
                         "period_mask.png / non_period_mask.png next to config.odgt; compute: npp_amd.init_segment (SLIC superpixels on "
                         "the GPU, mixture model and graph cut on the host); auto: the files when both exist, else computed")
    ap.add_argument("--nb_classes", type=int, default=3, help="classes of the initial segmentation (arg_config.py:210)")
    ap.add_argument("--sp_size", type=int, default=20, help="superpixel size of the initial segmentation (arg_config.py:212)")
    ap.add_argument("--sp_regul", type=float, default=0.1, help="superpixel regularisation of the initial segmentation (arg_config.py:214)")
    ap.add_argument("--contextual_weight", type=float, default=None)
    ap.add_argument("--style_weight", type=float, default=1.0)
    ap.add_argument("--datadir", required=True)
    ap.add_argument("--basedir", default="./results")
    ap.add_argument("--expname", default="completion")
    ap.add_argument("--p_topk", type=int, default=3)
    ap.add_argument("--N_iters", type=int, default=None, help="default 2001 (completion, arg_config.py) / 2801 (remapping, NPP_remapping)")
    ap.add_argument("--N_rand", type=int, default=8192)
    ap.add_argument("--lrate", type=float, default=5e-4)
    ap.add_argument("--lrate_decay", type=int, default=500)
    ap.add_argument("--netwidth", type=int, default=512, help="512: the reference's default (arg_config.py:57); 256: the BASELINE.json configurations")
    ap.add_argument("--netdepth", type=int, default=8)
    ap.add_argument("--activation", default="snake")
    ap.add_argument("--loss_type", default="robust_loss_adaptive")
    ap.add_argument("--normalize_type", type=int, default=1)
    # the reference's ablation switches (arg_config.py:78-92), with its store_false / store_true quirks kept
    ap.add_argument("--no_reg_sampling", action="store_true", help="real patches drawn at random instead of along the lattice (sampler.py:219-228)")
    ap.add_argument("--use_comp", action="store_false", help="(store_false) pass it to NOT paste the known region into 'val' patches")
    ap.add_argument("--use_perceptual_loss", action="store_true",
                    help="toggles the task's default: completion has LPIPS on 'same' iterations ON (store_false there, :84), "
                         "segmentation / remapping have it OFF (store_true, :190,274)")
    ap.add_argument("--perceptual_weight", type=float, default=1e-3)
    ap.add_argument("--use_contextual_loss", action="store_false", help="(store_false) pass it to drop the contextual term")
    ap.add_argument("--use_adaptive_perceptual_loss", action="store_false",
                    help="(store_false, as in arg_config.py:78) given: LPIPS(use_robust=False) in the loop instead of the adaptive-robust head")
    ap.add_argument("--use_patch_weight", action="store_true", help="1/d lattice weights on the patch terms (train.py:224-250)")
    ap.add_argument("--no_pix_loss", action="store_true", help="no pixel loss (train.py:197-198)")
    ap.add_argument("--patch_num", type=int, default=2)
    ap.add_argument("--num_real_patch_per_sample", type=int, default=3)
    ap.add_argument("--invalid_ratio", type=float, default=0.3)
    ap.add_argument("--patch_size_decay", type=int, default=2000)
    ap.add_argument("--i_testset", type=int, default=None, help="default 500 (completion) / 400 (remapping)")
    ap.add_argument("--i_print", type=int, default=500)
    ap.add_argument("--invalid_as_unknown", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rng_mode", default="reference", choices=["reference", "numpy", "fast", "device"],
                    help="reference: NumPy's stream from the native generator; numpy: NumPy itself; fast: O(size) draws, other stream; "
                         "device: the draws run as two GPU launches (Philox4x32-10 of seed and draw index; no producer thread)")
    ap.add_argument("--prefetch", type=int, default=8, help="iterations of sampler draws prepared ahead on a producer thread "
                                                            "(not with --rng_mode device, which has no host draws to prepare)")
    ap.add_argument("--vgg19", default=None, help="torchvision vgg19 state_dict (.pth) for the contextual loss trunk")
    ap.add_argument("--vgg16", default=None, help="torchvision vgg16 state_dict (.pth) for the LPIPS trunk")
    ap.add_argument("--lpips_lin", default=None, help="lpips weights/v0.1/vgg.pth (the five 1x1 lin layers)")
    ap.add_argument("--random-trunks", action="store_true",
                    help="run WITHOUT pretrained VGG19 / VGG16 / LPIPS-lin weights (fixed-seed random trunks: synthetic and bench "
                         "runs only -- the losses then differ from the reference's)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"],
                    help="arithmetic of the coordinate MLP's training launches: bf16 (default: the fused bf16 chain) or fp32 (the exact "
                         "fp32 chain -- the reference's own arithmetic, ~1/16 of the MFMA rate; the MLP only, see --trunk_precision)")
    ap.add_argument("--trunk_precision", default="fp16", choices=["fp16", "fp32"],
                    help="arithmetic of the VGG trunks of the patch losses: fp16 (default: fp16 activations, bf16 gradients) or fp32 (exact "
                         "fp32 convolutions -- with --precision fp32 the whole iteration runs in the reference's arithmetic; a diagnostic "
                         "mode, not stacked)")
    ap.add_argument("--graph_iteration", action="store_true",
                    help="replay the device side of every iteration as ONE captured HIP graph per iteration shape instead of enqueuing "
                         "its launches (CompletionFit(graph_iteration=True)): same bits, one graph launch of host time per iteration; "
                         "completion / segmentation with --precision bf16 --trunk_precision fp16, not stacked")
    ap.add_argument("--audit_stash", type=int, default=0, metavar="N",
                    help="audit the 8-bit training stash on every N-th iteration (0, default: never; CompletionFit(stash_audit=N)): "
                         "codes at the formats' limits and the distance of the iteration's weight gradients to the 16-bit stash's, one "
                         "[STASH] line per audit and stash_audit.json in the image's result directory; --precision bf16 with the "
                         "8-bit stash only, not stacked")
    ap.add_argument("--audit_trunk", type=int, default=0, metavar="N",
                    help="audit the fp16 VGG trunks of the patch losses on every N-th iteration (0, default: never; "
                         "CompletionFit(trunk_audit=N)): values at fp16's limits and flipped ReLU gates per stored layer, and the distance "
                         "of each term's patch gradient to the exact-fp32 trunks', one [TRUNK] line per audit and trunk_audit.json in "
                         "the image's result directory; --trunk_precision fp16 only, not stacked")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--save_model", action="store_true",
                    help="after a successful fit, write the network as model.npz into the image's result directory (npp_amd.render reads it)")
    ap.add_argument("--eval_metrics", action="store_true",
                    help="every [EVAL] line also carries the SSIM of the known and the unknown region, and the last report (PSNR, SSIM, "
                         "MAE over all / known / unknown, npp_amd.metrics.report of the image as pred_rgb_img.png holds it) is written "
                         "as metrics.json into the image's result directory (npp_amd.evaluate reproduces it from the files)")
    ap.add_argument("--eval_lpips", default=None, choices=["vgg", "alex"],
                    help="with --eval_metrics: the report also carries LPIPS on this net (npp_amd.metrics.LPIPSMetric: per region the "
                         "mean of the distance map, per image the scalar form) and every [EVAL] line the LPIPS of the known and the "
                         "unknown region; vgg takes --vgg16 / --lpips_lin, alex --alexnet / --lpips_alex_lin")
    return ap.parse_args(argv)


def default_linear_init(layout, n_params, seed):
    """torch nn.Linear default init per tensor of the blob (kaiming_uniform(a=sqrt 5) weight, uniform bias), drawn
    tensor by tensor in state_dict order from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    fan_in = {}
    for name, off, rows, cols in layout:
        if name.endswith("weight"):
            fan_in[name[:-7]] = cols
            bound = 1.0 / np.sqrt(cols)                       # kaiming_uniform with a = sqrt(5): sqrt(6 / ((1 + 5) fan_in))
            sd[name] = ((torch.rand(rows, cols, generator=g) * 2 - 1) * bound).numpy()
        else:
            bound = 1.0 / np.sqrt(fan_in[name[:-5]])
            sd[name] = ((torch.rand(rows * cols, generator=g) * 2 - 1) * bound).numpy()
    return sd


class _Job:
    """One image's fit between _prepare() and _finish(): arguments, loaded data, the CompletionFit, its output directory and the
    PNG writer thread."""
    pass


def _prepare(argv=None, stacked=False):
    """Everything `main` does before the loop (NPP_completion/train.py:28-131): flags, data, output directory, network init, the
    fit object.  -> _Job, or None when the result directory already exists (train.py:42-44).  stacked: the fit will ride in a
    StackedFit (which draws for every image itself: no producer thread)."""
    plan = _plan(argv)
    return None if plan is None else _build(plan, stacked)


def _plan(argv=None):
    """The side-effect-free half of _prepare: flags, the loaded detection, the output directory's NAME.  Creates nothing and touches
    no GPU memory, so a directory run can plan every image, group them by batch shape, and create an image's result directory only
    when its group starts fitting.  -> _Job without a fit, or None when the result directory already exists (train.py:42-44)."""
    args = parse(argv)
    if args.N_iters is None:
        args.N_iters = {"remapping": 2801, "segmentation": 601}.get(args.task, 2001)     # arg_config.py:96,202,289
    if args.i_testset is None:
        args.i_testset = {"remapping": 400, "segmentation": 600}.get(args.task, 500)
    if args.netwidth not in (256, 512):
        raise SystemExit("the fused chain is built for --netwidth 256 (BASELINE.json) and 512 (the reference's default)")
    refused = [n for n, bad in (("--netdepth != 8", args.netdepth != 8), ("--activation != snake", args.activation != "snake"),
                                ("--loss_type not in robust_loss_adaptive / l2 / robust_loss", args.loss_type not in ("robust_loss_adaptive", "l2", "robust_loss")),
                                ("--normalize_type not in 1 / 2", args.normalize_type not in (1, 2)),
                                ) if bad]
    if refused:
        raise SystemExit(f"{refused}: ablation switches of options/arg_config.py that the fused loop is not built for (D = 8, snake, sigmoid / tanh output); other widths / depths / activations run through reference_api.NPP_Net (dense.py)")
    if args.eval_metrics and args.normalize_type != 1:
        raise SystemExit("--eval_metrics judges images in [0, 1] (SSIM's data range is 1): --normalize_type 1 only")
    if args.eval_lpips is not None and not args.eval_metrics:
        raise SystemExit("--eval_lpips adds LPIPS to the report of --eval_metrics: give --eval_metrics as well")
    if args.graph_iteration:
        from .fit import refuse_graph_iteration
        refuse_graph_iteration(args.precision, args.trunk_precision, args.task, None, SystemExit, flag=True)
    for a in AUDITS:
        if getattr(args, a.flag[2:]) < 0:
            raise SystemExit(f"{a.flag} N: N >= 0 (0: never)")
        if getattr(args, a.flag[2:]):
            refuse_audit(a.kind, SystemExit, flag=True, capturing=False, precision=args.precision, trunk_precision=args.trunk_precision)
    seg_task = args.task == "segmentation"
    from . import weights
    names = ["vgg19"] + ([] if seg_task else ["vgg16"]) + (["alexnet"] if seg_task else [])    # remapping: VGG16 is the style trunk
    names += [n for n in ({"vgg": "vgg16", "alex": "alexnet"}.get(args.eval_lpips),) if n is not None and n not in names]
    weights.resolve(args, names, args.random_trunks)
    torch.cuda.set_device(torch.device(args.device))
    from . import io as nio
    from ._lib import param_layout
    from .fit import CompletionFit
    remap = args.task == "remapping"
    seg = args.task == "segmentation"
    name = os.path.basename(os.path.normpath(args.datadir))
    expname = args.expname if not ((remap or seg) and args.expname == "completion") else args.task
    outroot = os.path.join(args.basedir, f"{expname}_top{args.p_topk}", name)
    if os.path.exists(outroot):                                                             # train.py:42-44: results are never overwritten
        print(f"{args.task.capitalize()}: file exists, exit!!")
        return None
    if remap:
        d = nio.load_npp_remapping(args.datadir, args.p_topk, args.blur_thresh,
                                   blur_device=args.device if args.blur_detection == "gpu" else None)
        d["mask"], d["masked_img"] = d["clear_mask"], d["img"]
    elif seg:
        # (the masks are computed here, not in _build: they are part of the loaded data, and no directory is needed for them)
        d = nio.load_npp_segmentation(args.datadir, args.p_topk, init_seg=None if args.init_segmentation == "file" else args.init_segmentation,
                                      nb_classes=args.nb_classes, sp_size=args.sp_size, sp_regul=args.sp_regul, seed=args.seed,
                                      device=args.device, cc_device=args.device if args.components == "gpu" else None)
        d["mask"], d["masked_img"] = d["period_mask"], d["blur_img"]
    else:
        # --normalize_type 2: tanh output; the reference rescales only the evaluation image (loaders.py:111), training stays on
        # masked_img in [0, 1] (train.py:173) -- reproduced, not fixed
        d = nio.load_npp_completion(args.datadir, args.p_topk, args.invalid_as_unknown, normalize_type=args.normalize_type)
    plan = _Job()
    plan.args, plan.d, plan.outroot, plan.name, plan.remap, plan.seg, plan.fit = args, d, outroot, name, remap, seg, None
    return plan


def _build(plan, stacked=False):
    """The other half: the result directory (from here on a failure removes it again) and the CompletionFit."""
    from . import weights
    from . import io as nio
    from ._lib import param_layout
    from .fit import CompletionFit
    args, d, outroot, name, remap, seg = plan.args, plan.d, plan.outroot, plan.name, plan.remap, plan.seg
    os.makedirs(outroot, exist_ok=True)
    if seg:                                                  # loaders.py:208-212: white = non-periodic in the initial segmentation
        nio.imsave(os.path.join(outroot, "segment_init.png"), np.repeat(np.asarray(d["non_period_mask"] > 0, np.float64), 3, 2))
        print(f"initial segmentation ({d['init_seg_source']}): {float((d['period_mask'] > 0).mean()):.3f} of the image periodic")
    print("Loaded NPP", d["img"].shape, args.datadir)
    print("selected_angles: " + str(np.asarray(d["angles"]).tolist()))
    print("selected_periods: " + str(np.asarray(d["periods"]).tolist()))
    K = len(d["angles"])
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    freqs = (torch.normal(mean=0.0, std=1.0, size=(10, 1)) * 10).reshape(-1).numpy()       # embedder.py:26
    layout, n_params = param_layout(K, args.netwidth)
    params = default_linear_init(layout, n_params, args.seed)

    load = weights.load_state_dict                           # (one read per file and process: shared dicts -> shared packed trunk weights)
    lin = None if (args.random_trunks and args.lpips_lin is None and args.vgg16 is None) else weights.lpips_lin("vgg", args.lpips_lin)
    try:
        if args.audit_trunk and d["shifts"] is None:
            refuse_audit("trunk", SystemExit, flag=True, capturing=False, trunk_precision=args.trunk_precision, patch_losses=False)
        fit = CompletionFit(d["img"], d["mask"], d["angles"], d["periods"], freqs, params, device=args.device, N_rand=args.N_rand,
                            seed=args.seed, lrate=args.lrate, lrate_decay=args.lrate_decay, valid_mask=d["valid_mask"],
                            shifts=d["shifts"], patch_size=d["patch_size"], patch_num=args.patch_num,
                            num_real_patch_per_sample=args.num_real_patch_per_sample, invalid_ratio=args.invalid_ratio,
                            patch_size_decay=args.patch_size_decay, vgg19_state_dict=load(args.vgg19),
                            # --vgg16: the LPIPS trunk (completion) or the STYLE trunk of the remapping task (models/style_loss.py:11,
                            # VGG16FeatureExtractor; LPIPS is off there, NPP_remapping/train.py:253-261)
                            vgg16_state_dict=None if remap else load(args.vgg16),
                            vgg16_style_state_dict=load(args.vgg16) if remap else None,
                            lpips_lin_weights=lin, rng_mode=args.rng_mode, prefetch=0 if (stacked or args.rng_mode == "device") else args.prefetch,
                            task=args.task, clear_mask=d["clear_mask"] if remap else None,
                            masked_img=None if remap else d.get("masked_img"),
                            contextual_weight=args.contextual_weight if args.contextual_weight is not None else (0.01 if remap else (0.005 if seg else 1e-3)),
                            style_weight=args.style_weight if remap else None,
                            use_perceptual_loss=(not (remap or seg)) != args.use_perceptual_loss, perceptual_weight=args.perceptual_weight,
                            use_comp=args.use_comp, no_reg_sampling=args.no_reg_sampling, use_patch_weight=args.use_patch_weight,
                            no_pix_loss=args.no_pix_loss, use_contextual_loss=args.use_contextual_loss, width=args.netwidth,
                            loss_type=args.loss_type, use_adaptive_perceptual_loss=args.use_adaptive_perceptual_loss,
                            normalize_type=args.normalize_type, precision=args.precision,
                            trunk_precision=args.trunk_precision, graph_iteration=args.graph_iteration,
                            stash_audit=args.audit_stash, trunk_audit=args.audit_trunk)
    except BaseException:
        import shutil
        shutil.rmtree(outroot, ignore_errors=True)          # (nothing was fitted: a re-run must not take the directory for a result)
        raise
    # the six PNGs of a test set take ~150 ms to encode (zlib, GIL released): written behind the loop, joined before returning
    from concurrent.futures import ThreadPoolExecutor
    job = plan
    job.args, job.fit, job.d, job.outroot, job.seg, job.load, job.weights, job.nio = args, fit, d, outroot, seg, load, weights, nio
    job.writer, job.pending, job.t0, job.name = ThreadPoolExecutor(1), [], time.time(), name
    job.metrics = None                                       # --eval_metrics: the report of the newest test set
    job.lpips = None                                         # --eval_lpips: its LPIPSMetric
    job.audit_printed = {a.kind: 0 for a in AUDITS}          # --audit_stash / --audit_trunk: iteration of the newest [STASH] / [TRUNK] line
    if args.eval_lpips is not None:
        # (the state dict is the one object weights.load_state_dict gave the fit's own trunks: with --eval_lpips vgg and an fp32 LPIPS
        # trunk in the loop the metric finds that trunk's packed weights; there is no second copy)
        try:
            from .evaluate import lpips_metric
            job.lpips = lpips_metric(args.eval_lpips, args, args.lpips_lin if args.eval_lpips == "vgg" else args.lpips_alex_lin, args.device)
        except BaseException:
            import shutil
            fit.close()
            shutil.rmtree(outroot, ignore_errors=True)
            raise
    return job


def _metrics_report(job, pred_dev, i):
    """--eval_metrics: npp_amd.metrics.report of the rendered image as dump_testset writes it (8 bits, invalid pixels black), computed
    where the render and the fit's copy of the ground truth lie -- nothing is copied to the host but the partial sums -- plus the
    iteration."""
    from . import metrics
    d = job.d
    rep = metrics.report(metrics.quantised(pred_dev, d["mask"], d["valid_mask"]), job.fit.img, d["mask"], d["valid_mask"], device=pred_dev.device,
                         **({} if job.lpips is None else {"lpips": job.lpips}))
    rep["iteration"] = int(i)
    return rep


def _finish(job, failed):
    """The end of a fit, successful or not: producer thread stopped, queued PNG writers awaited; a fit that died mid-loop must not
    leave an output directory behind that a re-run would take for a finished one (`file exists, exit!!`) -- but an interrupted one
    (Ctrl-C) keeps the test sets it has already written.  Raises a writer's error when the loop itself succeeded."""
    write_error = None
    job.fit.close()                                         # the sampler's producer thread
    if failed is None and job.args.save_model:              # --save_model: the fitted network, before the fit is released
        try:
            job.fit.save_model(os.path.join(job.outroot, "model.npz"), image=job.name, iterations=job.args.N_iters - 1)
        except Exception as e:
            write_error = e
            print(f"[WARN] writing the model file failed: {e}")
    if failed is None and job.args.eval_metrics:            # --eval_metrics: the newest report (the final image's when no test set fell due)
        try:
            from .evaluate import dumps
            rep = job.metrics if job.metrics is not None else _metrics_report(job, job.fit.render_image(), job.args.N_iters - 1)
            with open(os.path.join(job.outroot, "metrics.json"), "w") as f:
                f.write(dumps(rep) + "\n")
        except Exception as e:
            write_error = write_error or e
            print(f"[WARN] writing metrics.json failed: {e}")
    for a in AUDITS:                                        # --audit_stash / --audit_trunk: every report, behind the format they speak of
        if failed is None and getattr(job.args, a.flag[2:], 0):
            try:
                with open(os.path.join(job.outroot, a.file), "w") as f:
                    f.write(audit_dumps(f"{a.kind}_format", getattr(job.fit, f"{a.kind}_audits"), a.format(job.fit)) + "\n")
            except Exception as e:
                write_error = write_error or e
                print(f"[WARN] writing {a.file} failed: {e}")
    # first the writers: a queued dump_testset re-creates its directory (os.makedirs(..., exist_ok=True)), so nothing is
    # removed while one may still run
    for p in job.pending:
        if not p.cancel():
            try:
                p.result()
            except Exception as e:
                write_error = write_error or e
                print(f"[WARN] writing a test set failed: {e}")
    job.writer.shutdown(wait=True)
    if (failed is not None and not isinstance(failed, KeyboardInterrupt)) or write_error is not None:
        import shutil
        shutil.rmtree(job.outroot, ignore_errors=True)
    if write_error is not None and failed is None:          # the loop itself succeeded: a lost output is still a failed run
        raise write_error


def main(argv=None):
    job = _prepare(argv)
    if job is None:
        return None
    failed = None
    try:
        _loop(job)
    except BaseException as e:
        failed = e
        raise
    finally:
        _finish(job, failed)
    return job.fit


def _loop(job):
    """The loop of one image, trange(start = 1, N_iters).  --graph_iteration: on a stream of its own -- a stream capture cannot begin
    on the default stream, where the fit would carry every iteration over to a side stream and back -- joined with the default
    stream on both sides, and the counts of fit.graph_stats once at the end."""
    fit = job.fit
    if not fit.graph_iteration:
        for i in range(1, job.args.N_iters):
            fit.step_full()
            _after_iteration(job, i)
        return
    cur = torch.cuda.current_stream(fit.device)
    s = torch.cuda.Stream(fit.device)
    s.wait_stream(cur)
    try:
        with torch.cuda.stream(s):
            for i in range(1, job.args.N_iters):
                fit.step_full()
                _after_iteration(job, i)
    finally:
        cur.wait_stream(s)
    st = fit.graph_stats
    print(f"[GRAPH] {st['replayed']} iterations replayed from {st['captured']} captured graphs, {st['eager']} launch by launch, "
          f"{fit.skipped} skipped")


def stack_key(job):
    """Fits that can share one launch sequence (stack.StackedFit): same network shape, batch shape, loss switches and schedule."""
    a, f = job.args, job.fit
    if (f.patch_sampler is None or f.use_patch_weight or not f.use_contextual_loss or f.net.out_act != 1 or f.net.precision != "bf16"
            or f.trunk_precision != "fp16" or f.graph_iteration or f.stash_audit or f.trunk_audit):       # (an audit needs the fit's own launch sequence)
        return None
    return (a.task, f.style is not None, f.style_w, f.pixel_mask is not None, f.net.K, f.net.width, f.N_rand, f.patch_size, f.patch_num, f.topk, f.net.quad, f.pix_w, f.use_comp, f.cx_w, f.lp_w,
            f.lp_robust, f.use_perceptual_loss, f.rng_mode, a.N_iters, a.i_testset, a.i_print, a.patch_size_decay, str(f.device))


def plan_key(plan):
    """stack_key's refinement that needs no fit: every flag that shapes the loop + what the detection fixes (K, patch size).  Plans of
    one key build fits of one stack_key (checked again on the built fits)."""
    a, d = plan.args, plan.d
    flags = tuple(sorted((k, str(v)) for k, v in vars(a).items() if k not in ("datadir", "expname", "seed")))
    return (flags, len(d["angles"]), d["patch_size"], tuple(np.asarray(d["img"]).shape))


class FitResult:
    """What a directory run keeps of a finished fit.  The fit itself -- weights, stashes, the trunks' activation buffers, captured
    LPIPS graphs -- is released with its group: device memory no longer grows with the number of images of a rank."""

    def __init__(self, job):
        f = job.fit
        self.name, self.outroot = job.name, job.outroot
        self.patch_size, self.patch_num, self.skipped = f.patch_size, f.patch_num, f.skipped
        self.psnr_known, self.psnr_unknown = f.psnr("known"), f.psnr("unknown")
        self.opt_step = f.net.opt_step
        self.has_style, self.style_lat_step = f.style is not None, (f.style.lat_step if f.style is not None else None)
        self.has_pixel_mask = f.pixel_mask is not None

    def psnr(self, region="known"):
        return self.psnr_known if region == "known" else self.psnr_unknown

    def close(self):
        pass


def main_stacked(argvs, max_stack=8):
    """Several images' fits in ONE launch sequence per group (stack.StackedFit): what `python -m npp_amd.run` does when a rank has
    more than one image (run_completion.sh:8-14 loops them serially; the fits are independent -- own weights, Adam state, random
    stream -- so the image becomes a grid dimension: 1.4 x the rows per second of the serial loop at 8 images per GPU).  Images group by
    batch shape (plan_key / stack_key: detected periods give patch sizes 64 .. 160, loaders.py:133-134); a group of one runs the
    plain loop.  Every image is PLANNED first (flags, detection: no directory, no device memory); an image's result directory is
    created and its fit built when its group starts, a failure -- of the plan, of the build, of the loop -- is recorded for the
    images it concerns only, and a group's fits are released before the next group is built.
    -> list of FitResult (None for skipped / failed outputs), in the order of argvs; main_stacked.last_error holds the first failure,
    main_stacked.errors the failure per argv (None where there was none)."""
    from .stack import StackedFit
    n = len(argvs)
    plans, errors, results = [None] * n, [None] * n, [None] * n
    for idx, a in enumerate(argvs):
        try:
            plans[idx] = _plan(a)
        except (Exception, SystemExit) as e:                                                # noqa: B014  (one image's bad flag / detection)
            errors[idx] = e
            print(f"[stack] {a}: not fitted ({type(e).__name__}: {e})")
    groups = {}
    for idx, plan in enumerate(plans):
        if plan is not None:
            groups.setdefault(plan_key(plan), []).append(idx)
    for key, members in groups.items():
        for c0 in range(0, len(members), max_stack):
            chunk_idx = members[c0:c0 + max_stack]
            jobs = []                                                                       # (idx, job) of the images whose fit was built
            for idx in chunk_idx:
                try:
                    jobs.append((idx, _build(plans[idx], stacked=len(chunk_idx) > 1)))
                except Exception as e:
                    import shutil
                    shutil.rmtree(plans[idx].outroot, ignore_errors=True)                   # (it did not exist when the image was planned)
                    errors[idx] = e
                    print(f"[stack] {plans[idx].name}: not fitted ({type(e).__name__}: {e})")
            if not jobs:
                continue
            chunk = [j for _, j in jobs]
            failed, st = None, None
            try:
                keys = {stack_key(j) for j in chunk}
                if len(chunk) == 1 or len(keys) != 1 or None in keys:
                    for job in chunk:
                        _loop(job)
                else:
                    st = StackedFit([j.fit for j in chunk])
                    print(f"[stack] {len(chunk)} images per launch sequence: {[j.name for j in chunk]} (patch size {st.P}, wgrad split-K {st.ksplit})")
                    for i in range(1, chunk[0].args.N_iters):
                        if st.shape_change_due():                                           # patch-size decay (train.py:137-141): new batch shape
                            st = st.restacked()
                        st.step_full()
                        for job in chunk:
                            _after_iteration(job, i)
            except BaseException as e:                                                      # noqa: B902
                failed = e
                if not isinstance(e, KeyboardInterrupt):
                    import traceback
                    traceback.print_exc()
                    print(f"[stack] group {[j.name for j in chunk]} FAILED ({type(e).__name__}: {e})")
            finally:
                if st is not None:
                    st.close()                                                              # its draw threads; the fits' own close() follows
                for idx, job in jobs:
                    try:
                        if failed is None:
                            results[idx] = FitResult(job)
                        _finish(job, failed)
                    except Exception as e:                                                  # a lost output of one image
                        errors[idx] = errors[idx] or e
                        results[idx] = None
                    if failed is not None:
                        errors[idx] = errors[idx] or failed
                        results[idx] = None
                    job.fit = None                                                          # release the group's device memory ...
                del st, chunk, jobs
                if torch.cuda.is_available():
                    torch.cuda.empty_cache()                                                # ... before the next group allocates its own
            if isinstance(failed, KeyboardInterrupt):
                raise failed
    main_stacked.errors = errors
    main_stacked.last_error = next((e for e in errors if e is not None), None)
    return results


def stash_format(width):
    """What --audit_stash audits, in words a log can carry: the first entry of stash_audit.json."""
    return {"stash": "8-bit (npp_tune stash8 = 1)", "layer_inputs": "fp8 e4m3 (OCP), largest finite 448, saturating conversion",
            "pre_activation_gradients": "bf8 e5m2, largest finite 57344, saturating conversion, scaled per 64-row tile by a power of two "
                                        "from max |dL/draw| of the tile",
            "weight_gradients": "block-scaled fp8 MFMA, fp32 accumulate", "compared_with": "16-bit stash (fp16 z, bf16 gradients, bf16 MFMA)",
            "width": int(width)}


def stash_line(rep):
    """The [STASH] line of one audit report."""
    cen, ts = rep["census"], rep["tile_scale"]
    at_max, nonfinite = at_limits(cen.values())
    return (f"[STASH] it {rep['iteration']} ({rep['source']}, {rep['rows']} rows): worst gap {rep['worst'][0]} {rep['worst'][1]:.3e}, "
            f"at_max {at_max}, nonfinite {nonfinite}, tile scale 2^{ts['scale_min'] - 127}..2^{ts['scale_max'] - 127}"
            + ("".join(f" [{f}]" for f in rep["flags"])))


def trunk_format():
    """What --audit_trunk audits, in words a log can carry: the first entry of trunk_audit.json."""
    return {"trunks": "frozen VGG stacks of the patch losses (contextual VGG19[0:18], LPIPS VGG16, style VGG16[0:17])",
            "forward": "fp16 activations and weights, fp32 accumulation, saturated at +-65504 without a flag",
            "gradients": "bf16, ReLU gates taken from the fp16 activations",
            "counted": "every stored layer over the images that carry a gradient: interior positions, true channels",
            "compared_with": "exact-fp32 trunks on the same weights (trunk_precision fp32)"}


def trunk_line(rep):
    """The [TRUNK] line of one audit report: the worst patch-gradient gap, the layer with the largest share of flipped gates over
    all terms, and the values at fp16's limits over all layers."""
    layers = [(t, n, L) for t, T in rep["terms"].items() for n, L in T["layers"].items()]
    at_max, nonfinite = at_limits(L for _, _, L in layers)
    _, wl, wL = max(layers, key=lambda e: e[2]["gate_flips"] / max(e[2]["elements"], 1))
    return (f"[TRUNK] it {rep['iteration']} ({rep['source']}, {rep['patches']} patches): worst gap {rep['worst'][0]} {rep['worst'][1]:.1e}, "
            f"gate flips {100.0 * wL['gate_flips'] / max(wL['elements'], 1):.2f} % at {wl}, at_max {at_max}, nonfinite {nonfinite}"
            + ("".join(f" [{f}]" for f in rep["flags"])))


# the audits of the command line, one row each: kind, flag, file in the result directory, format(fit), line(report)
stash_audit_dumps, trunk_audit_dumps = functools.partial(audit_dumps, "stash_format"), functools.partial(audit_dumps, "trunk_format")   # (reports, fmt)
Audit = collections.namedtuple("Audit", "kind flag file format line")
AUDITS = (Audit("stash", "--audit_stash", "stash_audit.json", lambda fit: stash_format(fit.net.width), stash_line),
          Audit("trunk", "--audit_trunk", "trunk_audit.json", lambda fit: trunk_format(), trunk_line))


def _after_iteration(job, i):
    """What follows optimizer.step() in the reference's loop body at iteration i: the periodic evaluation dump (train.py:270-331;
    segmentation: NPP_segmentation/train.py:337-406) and the progress line."""
    args, fit, d, outroot, seg, load, weights, nio, writer, pending, t0 = (job.args, job.fit, job.d, job.outroot, job.seg, job.load,
                                                                           job.weights, job.nio, job.writer, job.pending, job.t0)
    if i % args.i_testset == 0:
        pred_dev = fit.render_image()
        pred = pred_dev.cpu().numpy()
        os.makedirs(os.path.join(outroot, f"testset_{i:06d}"), exist_ok=True)
        pending.append(writer.submit(nio.dump_testset, os.path.join(outroot, f"testset_{i:06d}"), pred, d["img"], d["masked_img"], d["mask"],
                                     d["valid_mask"]))
        line = f"[EVAL] iter {i}: PSNR known {fit.psnr('known'):.2f} dB, unknown {fit.psnr('unknown'):.2f} dB"
        if args.eval_metrics:
            job.metrics = _metrics_report(job, pred_dev, i)
            line += ", SSIM known {} unknown {}".format(*("n/a" if job.metrics[r]["ssim"] is None else f"{job.metrics[r]['ssim']:.4f}"
                                                           for r in ("known", "unknown")))
            if job.lpips is not None:
                line += ", LPIPS known {} unknown {}".format(*("n/a" if job.metrics[r]["lpips"] is None else f"{job.metrics[r]['lpips']:.4f}"
                                                                for r in ("known", "unknown")))
        print(line)
        if seg:                                                                         # NPP_segmentation/train.py:337-406
            from . import segment
            alex = segment.AlexFeatures(load(args.alexnet), device=args.device)
            lins = weights.lpips_lin("alex", args.lpips_alex_lin)
            r = segment.segmentation_eval(pred * d["valid_mask"], d["blur_img"], d["valid_mask"], d["non_period_mask"], alex, lins,
                                          args.l1_thresh, args.lpips_thresh, args.lpips_layers,
                                          final_mask="gpu" if args.components == "gpu" else "host")
            tdir = os.path.join(outroot, f"testset_{i:06d}")
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt                                             # single-channel plt.imsave: viridis, autoscaled (:356-389)
            plt.imsave(os.path.join(tdir, "l1_diff_img.png"), r["l1_img"])
            plt.imsave(os.path.join(tdir, "l1_img_mask.png"), ~r["l1_mask"])
            for j, m in enumerate(r["lpips_maps"]):
                plt.imsave(os.path.join(tdir, f"lpips_diff_img_{j}.png"), m)
                plt.imsave(os.path.join(tdir, f"lpips_img_mask_{j}.png"), ~(m < args.lpips_thresh))
            nio.imsave(os.path.join(tdir, "non_period_mask_final.png"), np.repeat(r["non_period_mask_final"].astype(np.float64), 3, 2))
            m = r["non_period_mask_final"].astype(np.float64)
            vis = d["img"] * 0.7 + 0.3 * (np.array([0.0, 1.0, 0.0]) * m + d["img"] * (1 - m))    # :396-404
            nio.imsave(os.path.join(tdir, "segment.png"), vis * d["valid_mask"])
            fit.segmentation = r
    for a in AUDITS:
        rep = getattr(fit, f"last_{a.kind}_audit", None)
        if rep is not None and rep["iteration"] > job.audit_printed[a.kind]:
            job.audit_printed[a.kind] = rep["iteration"]
            print(a.line(rep))
    if i % args.i_print == 0:
        print(f"[TRAIN] Iter: {i} Loss: {float(fit.net.loss_buf[0]):.6f} Patch Loss: {float(fit.last_patch_loss[0]):.6f} "
              f"({(time.time() - t0) / i * 1e3:.2f} ms/iter, skipped {fit.skipped})")


if __name__ == "__main__":
    main()
