"""A/B of two builds of the library on the exact-fp32 chains (csrc/npp_chain32.h: npp_mlp_fwd32.hip, npp_mlp_train32.hip,
npp_light.hip): same bits, same speed.  The builds are switched through NPP_LIB_PATH (and NPP_LIB_PATH_W512 for the sibling
libnpp_hip_w512.so), one fresh process per run (profiles/chain32_resource_usage.txt, profiles/chain32_time.txt).

    python tools/chain32_check.py ab --parent PARENT/libnpp_hip.so --out DIR     # the driver: everything below, tables on stdout;
                                                                                 # exit status 1 if a hash differs or a head median
                                                                                 # lies outside the span of the parent's own runs
    python tools/chain32_check.py bits       # worker: SHA-256 of what the fp32 chains compute, one "name hash" line each
    python tools/chain32_check.py time       # worker: median us of every launch of the chains, one "name median_us ..." line each

bits: (a) ranking fits in fp32 -- nine candidates, 64 iterations x 2048 rows (32-row workgroups; params, latents, every iteration's
loss words, the score triples), the same nine for 8 iterations x 8192 rows (64-row workgroups), rank_images on three ragged images
(the _det and _multi forms); (b) one training step of NPPNet(precision="fp32") at K = 1 and K = 3, width 256, 677 rows (pred, stash,
dz, gradient slabs, params after the optimiser step); (c) fp32 renders of a 48 x 40 grid at supersample 1 and 2 and one view render.
time: each launch alone on one stream, TIME_LAUNCHES of it between a pair of device events, TIME_WINDOWS windows after TIME_WARMUP
launches."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TIME_LAUNCHES, TIME_WINDOWS, TIME_WARMUP = 200, 25, 50
WORKER_TIMEOUT = 420


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def dev_sha(*tensors):
    return sha(*[t.detach().cpu().numpy() for t in tensors])


def nine_candidates(H):
    from npp_amd import synthetic as syn
    angles, periods, shifts = syn.synthetic_periodicity(H, 3)
    return [(angles[i % 3] + 3.0 * (i // 3), periods[i % 3] * (1.0 + 0.11 * (i // 3)), shifts[i % 3]) for i in range(9)]


def image_and_rows(H, Wd=None, seed=0, hole=(40, 88, 36, 92)):
    import numpy as np
    from npp_amd import synthetic as syn
    Wd = Wd or H
    img, _ = syn.synthetic_image(max(H, Wd), noise=0.01, seed=seed)
    img = img[:H, :Wd]
    pseudo = np.ones((H, Wd), np.float32)
    pseudo[hole[0]:hole[1], hole[2]:hole[3]] = 0
    return img, np.stack(np.nonzero(pseudo), 1), np.stack(np.nonzero(1 - pseudo), 1)


def fit_net(K, dev, width=256):
    import oracle
    from npp_amd.model import NPPNet
    H = 256
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    return NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=oracle.init_params(K, W=width, seed=0), device=dev, ksplit=3,
                  width=width, precision="fp32")


def fit_batch(n, H=256):
    import numpy as np
    rng = np.random.RandomState(5)
    Bp = (n + 63) // 64 * 64
    cp = np.zeros((Bp, 2), np.int32)
    cp[:n] = np.stack([rng.randint(0, H, n), rng.randint(0, H, n)], 1)
    return cp, np.random.RandomState(2).rand(n, 3).astype(np.float32)


def bits():
    import numpy as np
    import torch
    from npp_amd import ops
    from npp_amd import synthetic as syn
    from npp_amd.light import ProposalRanker, rank_images
    assert ops.DETERMINISTIC
    dev = torch.device("cuda", 0)
    H = 128

    # (a) ranking fits
    def fit(tag, cands, n_iters, n_rand):
        img, i_train, i_val = image_and_rows(H)
        rk = ProposalRanker(img, i_train, i_val, device=dev, N_iters=n_iters, N_rand=n_rand, precision="fp32", record_losses=True)
        blocks = ops.light_part_blocks(len(cands), n_rand)
        nets = rk.fit_candidates([(a, p) for a, p, _ in cands])           # what ProposalRanker.rank does, with the nets in hand
        details = [rk.score(net) for net in nets]
        torch.cuda.synchronize()
        print(f"{tag}.rows_per_wg {n_rand // blocks}")
        print(f"{tag}.losses {dev_sha(*rk.loss_log)}")
        print(f"{tag}.scores {sha(np.asarray(details, np.float64))}")
        print(f"{tag}.params {dev_sha(*[net.params for net in nets])}")
        print(f"{tag}.latents {dev_sha(*[net.latents for net in nets])}")

    c9 = nine_candidates(H)
    fit("a.fp32.nine.2048", c9, 64, 2048)
    fit("a.fp32.nine.8192", c9, 8, 8192)
    angles, periods, shifts = syn.synthetic_periodicity(128, 1)
    rankers, cand_lists = [], []
    for i, (h, w, ncand) in enumerate([(128, 128, 3), (96, 144, 2), (128, 128, 3)]):
        img, i_train, i_val = image_and_rows(h, w, seed=i, hole=(30 + 5 * i, 70, 40, 80 + 4 * i))
        rankers.append(ProposalRanker(img, i_train, i_val, device=dev, N_iters=64, N_rand=1024, precision="fp32"))
        cand_lists.append([(angles[0] + 7.0 * j, periods[0] * (1.0 + 0.23 * j), shifts[0]) for j in range(ncand)])
    out = rank_images(rankers, cand_lists, topk=10)
    torch.cuda.synchronize()
    print(f"a.fp32.ragged3.details {sha(*[np.asarray(det, np.float64) for _, _, det in out])}")
    print(f"a.fp32.ragged3.order {sha(*[np.asarray(o, np.int64) for _, o, _ in out])}")

    # (b) one training step of the coordinate MLP
    n = 677
    cp, gt = fit_batch(n)
    for K in (1, 3):
        net = fit_net(K, dev)
        Bp = cp.shape[0]
        net.zero_grad()
        pred = net.forward_train(torch.from_numpy(cp).to(dev))
        ws = net.workspace(Bp)
        ws["dpred"].zero_()
        net.pixel_loss(Bp, n, torch.from_numpy(gt).to(dev))
        net.backward(Bp)
        torch.cuda.synchronize()
        tag = f"b.fp32.step.K{K}"
        print(f"{tag}.pred {dev_sha(pred)}")
        print(f"{tag}.stash {dev_sha(ws['actT'])}")
        print(f"{tag}.dz {dev_sha(ws['dzT'])}")
        print(f"{tag}.gslabs {dev_sha(ws['gslabs'])}")
        net.optimizer_step(Bp)
        torch.cuda.synchronize()
        print(f"{tag}.params {dev_sha(net.params)}")

    # (c) renders
    net = fit_net(3, dev)
    for ss in (1, 2):
        print(f"c.fp32.grid48x40.ss{ss} {dev_sha(net.render_grid((48, 40), origin=(3.25, -2.5), scale=(0.5, 0.75), precision='fp32', supersample=ss))}")
    M = np.array([[1.9, 0.2, -4.0], [-0.1, 2.1, 7.0], [1e-3, -2e-3, 1.0]])
    img, inside = net.render_view((48, 40), M, precision="fp32", return_inside=True)
    print(f"c.fp32.view48x40 {dev_sha(img, inside)}")


def time_launches():
    import numpy as np
    import torch
    from npp_amd import ops
    from npp_amd.light import NPPNetLightBatch, default_light_init
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    calls = []

    # the ranking fits' chains: 9 candidates x 2048 rows (32-row workgroups), 3 x 16448 (64-row workgroups)
    H = 512
    freqs = (rng.randn(10) * 10).astype(np.float32)
    for C_, B in ((9, 2048), (3, 16448)):
        cands = [(a, p) for a, p, _ in nine_candidates(H)][:C_]
        net = NPPNetLightBatch(cands, freqs, (H, H), default_light_init(256, 4), device=dev, fused=True, precision="fp32")
        coords = torch.from_numpy(np.stack([rng.randint(0, H, B), rng.randint(0, H, B)], 1).astype(np.int32)).to(dev)
        tabs = [n_.embed(coords) for n_ in net.nets]
        x_pos, x_per = tabs[0][0].contiguous(), torch.stack([t[1] for t in tabs]).contiguous()
        gt = torch.from_numpy(rng.rand(B, 3).astype(np.float32)).to(dev)
        for _ in range(2):                                            # the packs, the workspace, every code object
            net.train_step(x_pos, x_per, gt)
        ws = net._ws[("fused", B)]
        rows = B // ops.light_part_blocks(C_, B)
        calls.append((f"light_fwd_kernel<{rows // 32}>", lambda net=net, ws=ws, x_per=x_per, x_pos=x_pos: ops.light_fwd(
            net._desc, net.params, net._pack, x_per, x_pos, ws["stash"], ws["pred"])))
        calls.append((f"light_bwd_kernel<{rows // 32}>", lambda net=net, ws=ws, gt=gt: ops.light_bwd_det(
            net._desc, net.params, net._pack, ws["stash"], ws["pred"], ws["draw"], ws["dstash"], gt, net.latents, net.spline, net.n_knots,
            net.x_scale, ws["part"])))

    # the coordinate MLP: render, forward with stash, data gradients at 16384 rows (one 64-row tile per CU), both widths
    Bp = 16384
    ci = torch.from_numpy(np.stack([rng.randint(0, 256, Bp), rng.randint(0, 256, Bp)], 1).astype(np.int32)).to(dev)
    out = torch.empty((Bp, 3), dtype=torch.float32, device=dev)
    for K, width in ((3, 256), (1, 256), (3, 512)):
        net = fit_net(K, dev, width)
        net.forward_train(ci)
        ws = net.workspace(Bp)
        net.pixel_loss(Bp, Bp, torch.rand((Bp, 3), device=dev))
        net.backward(Bp)
        w32, w32b = net._w32_pack(), ops.pack_weights32_bwd(net.params, K, None, width)
        tag = f"K{K}.W{width}"
        kw = dict(precision="fp32", out_act=net.out_act, width=width)
        calls.append((f"mlp_fwd32_kernel.points.{tag}", lambda net=net, w32=w32, kw=kw: ops.render(ci, net.cfg, w32, net.params, out=out, **kw)))
        calls.append((f"mlp_fwd32_kernel.grid.{tag}", lambda net=net, w32=w32, kw=kw: ops.render(
            ops.grid_arg(0, Bp, 128, (0.25, 0.5), (0.5, 0.5)), net.cfg, w32, net.params, out=out, **kw)))
        calls.append((f"mlp_fwd32_kernel.stash.{tag}", lambda net=net, w32=w32, ws=ws, width=width: ops.mlp_fwd32_train(
            ci, net.cfg, w32, net.params, ws["pred"], ws["actT"], net.out_act, width)))
        calls.append((f"mlp_bwd32_kernel.{tag}", lambda net=net, w32b=w32b, ws=ws, K=K, width=width: ops.mlp_bwd32(
            ws["dpred"], ws["pred"], K, w32b, net.params, ws["actT"], ws["dzT"], width, net.out_act)))

    for name, call in calls:
        for _ in range(TIME_WARMUP):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(TIME_WINDOWS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(TIME_LAUNCHES):
                call()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / TIME_LAUNCHES)
        print(f"{name} median_us {statistics.median(us):.3f} min_us {min(us):.3f} max_us {max(us):.3f}", flush=True)


def child(mode, lib):
    env = dict(os.environ)
    for var, name in (("NPP_LIB_PATH", "libnpp_hip.so"), ("NPP_LIB_PATH_W512", "libnpp_hip_w512.so")):
        env.pop(var, None)
        if lib:
            env[var] = os.path.join(os.path.dirname(lib), name)
    p = subprocess.run(["timeout", "-k", "10", str(WORKER_TIMEOUT), sys.executable, os.path.abspath(__file__), mode], env=env,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{mode} worker failed with status {p.returncode} (library: {lib or 'in-tree'}); nothing more is started")
    print(f"[{mode} worker done, library: {lib or 'in-tree'}]", file=sys.stderr, flush=True)
    return p.stdout


def ab(parent, out_dir, rounds, skip_time):
    os.makedirs(out_dir, exist_ok=True)
    cols = [dict(l.split() for l in child("bits", lib).splitlines() if len(l.split()) == 2) for lib in (parent, parent, None)]
    lines = ["quantity                         parent run 1       parent run 2       head"]
    equal = True
    for k in sorted(cols[0]):
        v = [c.get(k, "missing") for c in cols]
        equal &= v[0] == v[1] == v[2]
        lines.append(f"{k:<32} {v[0]:<18} {v[1]:<18} {v[2]:<18}" + ("" if v[0] == v[1] == v[2] else "  <- DIFFERENT"))
    lines.append("all three columns equal" if equal else "COLUMNS DIFFER")
    open(os.path.join(out_dir, "chain32_bits.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    if skip_time:
        return equal
    # parent (A), parent again (A'), head (B), interleaved: one fresh process each, `rounds` times
    builds = ("parent A", "parent A'", "head")
    med, kerns = {k: {} for k in builds}, []
    for _ in range(rounds):
        for k, lib in (("parent A", parent), ("head", None), ("parent A'", parent)):
            for l in child("time", lib).splitlines():
                w = l.split()
                if len(w) >= 3 and w[1] == "median_us":
                    med[k].setdefault(w[0], []).append(float(w[2]))
                    if w[0] not in kerns:
                        kerns.append(w[0])
    lines = [f"median us per launch over {TIME_WINDOWS} windows of {TIME_LAUNCHES} launches, one fresh process per entry, builds interleaved"]
    inside = True
    for kern in kerns:
        for k in builds:
            v = med[k][kern]
            lines.append(f"{kern:<34} {k:<10} {[round(x, 2) for x in v]}  median {statistics.median(v):.2f}")
        both = med["parent A"][kern] + med["parent A'"][kern]
        h = statistics.median(med["head"][kern])
        ok = min(both) <= h <= max(both)
        inside &= ok
        lines.append(f"  parent's own runs span [{min(both):.2f}, {max(both):.2f}]; head's median {h:.2f} " + ("inside" if ok else "OUTSIDE"))
    lines.append("every head median inside the parent's span" if inside else "SOME HEAD MEDIAN OUTSIDE THE PARENT'S SPAN")
    open(os.path.join(out_dir, "chain32_time.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return equal and inside


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "bits", "time"])
    ap.add_argument("--parent", help="libnpp_hip.so of the parent commit's build (libnpp_hip_w512.so next to it)")
    ap.add_argument("--out", default="chain32_ab")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-time", action="store_true", help="ab: the bits table only (for a head whose device code is the parent's in every kernel)")
    a = ap.parse_args()
    if a.mode == "bits":
        bits()
    elif a.mode == "time":
        time_launches()
    else:
        if not a.parent or not os.path.exists(a.parent):
            raise SystemExit("--parent: the parent build's libnpp_hip.so")
        sys.exit(0 if ab(os.path.abspath(a.parent), a.out, a.rounds, a.skip_time) else 1)
