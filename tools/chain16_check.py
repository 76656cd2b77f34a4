"""A/B of two builds of the library on the candidate-ranking fits' 16-bit chains (csrc/npp_light16.hip): same bits, same speed.
The builds are switched through NPP_LIB_PATH, one fresh process per run (profiles/chain16_resource_usage.txt, profiles/chain16_time.txt).

    python tools/chain16_check.py ab --parent PARENT/libnpp_hip.so --out DIR     # the driver: everything below, tables on stdout
    python tools/chain16_check.py bits       # worker: SHA-256 of what the ranking fits compute, one "name hash" line each
    python tools/chain16_check.py time       # worker: median us of the forward / backward launch at 9 candidates x 2048 rows

bits: nine candidates in bf16, 64 iterations x 2048 rows (params, latents, every iteration's loss words, the score triples);
carry_latents on three; rank_images on three ragged images (the _det and _multi forms of the launches).
time: the two launches alone on one stream, TIME_LAUNCHES of each between a pair of device events, TIME_WINDOWS windows."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TIME_LAUNCHES, TIME_WINDOWS = 200, 25


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


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


def bits():
    import numpy as np
    import torch
    from npp_amd import ops
    from npp_amd import synthetic as syn
    from npp_amd.light import ProposalRanker, rank_images
    assert ops.DETERMINISTIC
    dev = torch.device("cuda", 0)
    H = 128

    def fit(tag, cands, **kw):
        img, i_train, i_val = image_and_rows(H)
        rk = ProposalRanker(img, i_train, i_val, device=dev, N_iters=64, N_rand=2048, precision="bf16", record_losses=True, **kw)
        nets = rk.fit_candidates([(a, p) for a, p, _ in cands])           # what ProposalRanker.rank does, with the nets in hand
        details = [rk.score(net) for net in nets]
        torch.cuda.synchronize()
        print(f"{tag}.losses {sha(*[l.cpu().numpy() for l in rk.loss_log])}")
        print(f"{tag}.scores {sha(np.asarray(details, np.float64))}")
        print(f"{tag}.params {sha(*[net.params.cpu().numpy() for net in nets])}")
        print(f"{tag}.latents {sha(*[net.latents.cpu().numpy() for net in nets])}")

    c9 = nine_candidates(H)
    fit("ii_iii.bf16.nine", c9)
    fit("iv.bf16.carry3", c9[:3], carry_latents=True)
    # v: three ragged images searched together (npp_light16_fwd_multi / _bwd_det / _adam_pack_det), chained and independent
    angles, periods, shifts = syn.synthetic_periodicity(128, 1)
    for carry in (False, True):
        rankers, cand_lists = [], []
        for i, (h, w, ncand) in enumerate([(128, 128, 3), (96, 144, 2), (128, 128, 3)]):
            img, i_train, i_val = image_and_rows(h, w, seed=i, hole=(30 + 5 * i, 70, 40, 80 + 4 * i))
            rankers.append(ProposalRanker(img, i_train, i_val, device=dev, N_iters=64, N_rand=1024, carry_latents=carry, precision="bf16"))
            cand_lists.append([(angles[0] + 7.0 * j, periods[0] * (1.0 + 0.23 * j), shifts[0]) for j in range(ncand)])
        out = rank_images(rankers, cand_lists, topk=10)
        torch.cuda.synchronize()
        print(f"v.bf16.carry{int(carry)}.details {sha(*[np.asarray(det, np.float64) for _, _, det in out])}")
        print(f"v.bf16.carry{int(carry)}.order {sha(*[np.asarray(o, np.int64) for _, o, _ in out])}")


def time_launches():
    import numpy as np
    import torch
    from npp_amd import ops
    from npp_amd.light import NPPNetLightBatch, default_light_init
    dev = torch.device("cuda", 0)
    H, C, B = 512, 9, 2048
    rng = np.random.RandomState(0)
    cands = [(a, p) for a, p, _ in nine_candidates(H)]
    freqs = (rng.randn(10) * 10).astype(np.float32)
    net = NPPNetLightBatch(cands, freqs, (H, H), default_light_init(256, 4), device=dev, fused=True, precision="bf16")
    coords = torch.from_numpy(np.stack([rng.randint(0, H, 4 * B), rng.randint(0, H, 4 * B)], 1).astype(np.int32)).to(dev)
    tabs = [n_.embed(coords) for n_ in net.nets]
    x_pos, x_per = tabs[0][0].contiguous(), torch.stack([t[1] for t in tabs]).contiguous()
    gt = torch.from_numpy(rng.rand(B, 3).astype(np.float32)).to(dev)
    idx = torch.from_numpy(rng.permutation(4 * B)[:B]).to(dev)
    for _ in range(3):                                            # the packs, the workspace, every code object
        net.train_step(x_pos, x_per, gt, idx=idx)
    ws = net._ws[("bf16", B)]
    fwd = ops.light16_fwd(net._desc, net.params, net._pack16, x_per, x_pos, ws["actF"], ws["pred"], idx=idx, bind=True)
    bwd = ops.light16_bwd_det(net._desc, net.params, net._pack16, ws["actF"], ws["pred"], ws["dzF"], gt, net.latents, net.spline, net.n_knots,
                              net.x_scale, ws["part"], bind=True)
    for name, call in (("fwd", fwd), ("bwd", bwd)):
        for _ in range(50):
            ops.check(call(), name)
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
        print(f"{name} median_us {statistics.median(us):.3f} min_us {min(us):.3f} max_us {max(us):.3f}")


def child(mode, lib):
    env = dict(os.environ)
    if lib:
        env["NPP_LIB_PATH"] = lib
    else:
        env.pop("NPP_LIB_PATH", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{mode} worker failed with status {p.returncode} (library: {lib or 'in-tree'}); nothing more is started")
    return p.stdout


def ab(parent, out_dir, rounds):
    os.makedirs(out_dir, exist_ok=True)
    cols = [dict(l.split() for l in child("bits", lib).splitlines() if len(l.split()) == 2) for lib in (parent, parent, None)]
    lines = ["quantity                         parent run 1       parent run 2       head"]
    equal = True
    for k in sorted(cols[0]):
        v = [c.get(k, "missing") for c in cols]
        equal &= v[0] == v[1] == v[2]
        lines.append(f"{k:<32} {v[0]:<18} {v[1]:<18} {v[2]:<18}" + ("" if v[0] == v[1] == v[2] else "  <- DIFFERENT"))
    lines.append("all three columns equal" if equal else "COLUMNS DIFFER")
    open(os.path.join(out_dir, "chain16_bits.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    # parent (A), parent again (A'), head (B), interleaved: one fresh process each, `rounds` times
    med = {k: {"fwd": [], "bwd": []} for k in ("parent A", "parent A'", "head")}
    for _ in range(rounds):
        for k, lib in (("parent A", parent), ("head", None), ("parent A'", parent)):
            for l in child("time", lib).splitlines():
                w = l.split()
                if len(w) >= 3 and w[1] == "median_us":
                    med[k][w[0]].append(float(w[2]))
    lines = [f"median us per launch over {TIME_WINDOWS} windows of {TIME_LAUNCHES} launches, one fresh process per entry, builds interleaved"]
    for kern in ("fwd", "bwd"):
        for k in ("parent A", "parent A'", "head"):
            v = med[k][kern]
            lines.append(f"light16_{kern}_kernel  {k:<10} {[round(x, 2) for x in v]}  median {statistics.median(v):.2f}")
        both = med["parent A"][kern] + med["parent A'"][kern]
        h = statistics.median(med["head"][kern])
        lines.append(f"  parent's own runs span [{min(both):.2f}, {max(both):.2f}]; head's median {h:.2f} "
                     + ("inside" if min(both) <= h <= max(both) else "OUTSIDE"))
    open(os.path.join(out_dir, "chain16_time.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return equal


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "bits", "time"])
    ap.add_argument("--parent", help="libnpp_hip.so of the parent commit's build")
    ap.add_argument("--out", default="chain16_ab")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "bits":
        bits()
    elif a.mode == "time":
        time_launches()
    else:
        if not a.parent or not os.path.exists(a.parent):
            raise SystemExit("--parent: the parent build's libnpp_hip.so")
        sys.exit(0 if ab(os.path.abspath(a.parent), a.out, a.rounds) else 1)
