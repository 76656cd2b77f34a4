"""The segmentation task's INITIAL coarse segmentation (loaders/loaders.py:162-205): SLIC superpixels -> per-superpixel colour
features -> Gaussian mixture with `nb_classes` components -> Potts graph cut over the superpixel graph -> "the class that fills the
centre of the image is the periodic one".  The reference runs it through its vendored imsegm package (skimage.segmentation.slic,
sklearn.mixture.GaussianMixture, the gco library); none of the three is a dependency here (cvlite.py sets the precedent), and the
reference's own result differs from run to run (unseeded k-means starts).  This module states the same pipeline deterministically.

What runs where: everything per PIXEL -- colour conversion and blur, the ten assign / update rounds of SLIC, the per-superpixel
sums and histograms -- is HIP (csrc/npp_slic.hip through ops.slic_*).  Everything per SUPERPIXEL (a few hundred nodes) is NumPy /
SciPy on the host: the connectivity repair (a graph traversal done once per image), the mixture model and the graph cut.  The repair's
own per-pixel half -- labelling the 4-connected fragments, their sizes, colour sums and touching pairs -- runs on the host by default and
through npp_amd.regions (csrc/npp_regions.hip) with cc_device; its merge rounds over the fragments are host work either way.
"""
import numpy as np
import scipy.sparse as sparse
from scipy.sparse import csgraph

N_FEATURES = 9                      # mean x 3, median x 3, meanGrad x 3  (dict_features = {'color': ['mean', 'median', 'meanGrad']})
GC_REGUL = 2.0                      # loaders.py:178
MIN_UNARY_PROB, MIN_MAX_EDGE_WEIGHT = 0.01, 1e3          # graph_cuts.py:36,40


def as_u8(img):
    """(H,W,3) uint8 as is; a float image in [0,1] (what the loaders hand around) back to the 8-bit values it was read from."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        img = np.uint8(np.rint(np.clip(np.asarray(img, np.float64), 0.0, 1.0) * 255.0))
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected an (H, W, 3) image")
    return np.ascontiguousarray(img)


# ---- SLIC ---------------------------------------------------------------------------------------------------------------------
def slic_geometry(mask, sp_size):
    """n_segments = int(H W / sp_size^2) (superpixels.py:58), the step S = sqrt(mask pixels / n_segments), and the start positions:
    the grid points (S/2 + i S, S/2 + j S) whose pixel lies in the mask, row-major.  (This grid replaces the reference's random
    masked k-means start.)  -> n_segments, S, (K, 2) float64 (y, x)."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    n_segments = int(H * W / float(sp_size) ** 2)
    if n_segments < 1 or not mask.any():
        raise ValueError(f"no superpixels: image {H}x{W}, sp_size {sp_size}, {int(mask.sum())} mask pixels")
    S = float(np.sqrt(mask.sum() / n_segments))
    gy = np.arange(S / 2, H, S)
    gx = np.arange(S / 2, W, S)
    yy, xx = np.meshgrid(gy, gx, indexing="ij")
    pos = np.stack([yy.ravel(), xx.ravel()], 1)
    keep = mask[pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)]
    if not keep.any():
        raise ValueError("no grid point of the SLIC start falls on the mask")
    return n_segments, S, pos[keep]


def _fragments_cc(labels, colour, cc_device):
    """The per-pixel half of enforce_connectivity through npp_amd.regions on `cc_device` ("cpu": the library's host twins; a CUDA
    device: the kernels): -> frag (H,W) int32 tensor on that device (the 4-connected fragments numbered 1..C in raster order, 0
    outside), C, size (C+1,) and csum (C+1, nch) float64 (entry 0 unused: 0), the sorted unique int64 codes of the touching pairs."""
    import torch
    from . import ops, regions
    colour = np.asarray(colour)
    H, W = labels.shape
    if colour.dtype != np.uint8 or colour.shape[:2] != (H, W) or colour.ndim != 3 or not 1 <= colour.shape[2] <= ops.CC_MAX_CHANNELS:
        raise TypeError(f"enforce_connectivity(cc_device={cc_device!r}): colour must be an ({H}, {W}, 1..{ops.CC_MAX_CHANNELS}) uint8 "
                        f"image (what slic() passes), got {colour.dtype} {colour.shape}")
    dev = torch.device("cpu") if str(cc_device) == "cpu" else ops.select_device(cc_device)
    lab = torch.from_numpy(np.ascontiguousarray(np.where(labels > 0, labels, 0), np.int32))      # (the host path's `inside`)
    if dev.type == "cuda":
        frag, C = regions.label(lab.to(dev), dev)
        sz, cs, _, _ = regions.component_stats(frag, C, torch.from_numpy(np.ascontiguousarray(colour)).to(dev))
        sz, cs = sz.cpu().numpy(), cs.cpu().numpy()
    else:
        frag, C = regions.label(lab, "cpu")
        sz, cs, _, _ = regions.component_stats(frag.numpy(), C, colour)
    size = np.concatenate([[0.0], sz.astype(np.float64)])
    csum = np.concatenate([np.zeros((1, colour.shape[2])), cs.astype(np.float64)])
    f = frag.long()
    i, j = torch.cat([f[:, :-1].reshape(-1), f[:-1].reshape(-1)]), torch.cat([f[:, 1:].reshape(-1), f[1:].reshape(-1)])
    k = (i != j) & (i > 0) & (j > 0)
    i, j = i[k], j[k]
    pairs = torch.unique(torch.minimum(i, j) * (C + 1) + torch.maximum(i, j), sorted=True)
    return frag, C, size, csum, pairs.cpu().numpy()


def enforce_connectivity(labels, min_size, colour, max_size=None, cc_device=None):
    """Connectivity repair of a label image (0 = outside the mask): every 4-connected fragment becomes a segment of its own, then the
    segments smaller than `min_size` pixels are merged away in rounds -- each picks one adjacent segment, all picks of a round are
    carried out together -- until none is left that has a neighbour; labels are renumbered 1..N in raster order of first appearance.
    The pick: a neighbour that stays within `max_size` pixels (default 6 min_size = three mean segments, skimage's max_size_factor)
    before one that does not, then the one whose mean `colour` ((H,W,3) image) is nearest, then the lowest number.  The rule matters:
    at the reference's compactness ((20 * 0.1)^1.5 = 2.8 Lab units) the SLIC labels are close to a colour quantisation, on a textured
    image most of the area lies in fragments below `min_size`, and the merge decides what the superpixels are.  Merging by colour
    keeps a fragment of a flat region out of the textured segment next to it (and the other way round), which merging by border
    length or by size does not.  Host code on purpose: a graph traversal over a few thousand fragments, done once per image (whole
    rounds at a time in NumPy).  cc_device: None -- the fragments, their sizes, colour sums and touching pairs are found on the
    host too (SciPy); "cpu" or a CUDA device -- by npp_amd.regions there (`colour` must then be the uint8 image itself); the merge
    rounds are the same host code and the returned labels are identical."""
    labels = np.asarray(labels)
    H, W = labels.shape
    if cc_device is not None:
        import torch
        frag_t, C, size, csum, pairs = _fragments_cc(labels, colour, cc_device)
        max_size = 6 * min_size if max_size is None else max_size
        root = _merge_rounds(C, size, csum, pairs, min_size, max_size)
        # raster order of first appearance = ascending lowest fragment number: the fragments are numbered in that order themselves
        remap = np.zeros(C + 1, np.int32)
        kept = np.unique(root[1:])
        remap[kept] = np.arange(1, len(kept) + 1)
        lut = torch.from_numpy(remap[root]).to(frag_t.device)
        return lut[frag_t.long()].cpu().numpy()
    idx = np.arange(H * W).reshape(H, W)
    same_h = (labels[:, :-1] == labels[:, 1:]) & (labels[:, :-1] > 0)
    same_v = (labels[:-1] == labels[1:]) & (labels[:-1] > 0)
    a = np.concatenate([idx[:, :-1][same_h], idx[:-1][same_v]])
    b = np.concatenate([idx[:, 1:][same_h], idx[1:][same_v]])
    g = sparse.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(H * W, H * W)).tocsr()
    _, comp = csgraph.connected_components(g, directed=False)
    comp = comp.reshape(H, W)
    inside = labels > 0

    def raster_numbers(ids):
        """ids (H,W) -> the same partition of `inside` numbered 1..n in raster order of first appearance, 0 outside."""
        values, first = np.unique(ids[inside], return_index=True)
        remap = np.zeros(int(ids.max()) + 1, np.int64)
        remap[values[np.argsort(first, kind="stable")]] = np.arange(1, len(values) + 1)
        return np.where(inside, remap[ids], 0), len(values)
    frag, C = raster_numbers(comp)
    size = np.bincount(frag.ravel(), minlength=C + 1).astype(np.float64)
    size[0] = 0
    colour = np.asarray(colour, np.float64).reshape(H * W, -1)
    csum = np.stack([np.bincount(frag.ravel(), weights=colour[:, k], minlength=C + 1) for k in range(colour.shape[1])], 1)
    max_size = 6 * min_size if max_size is None else max_size
    pairs = _touching(np.concatenate([frag[:, :-1].ravel(), frag[:-1].ravel()]), np.concatenate([frag[:, 1:].ravel(), frag[1:].ravel()]), C)
    root = _merge_rounds(C, size, csum, pairs, min_size, max_size)
    return raster_numbers(root[frag])[0].astype(np.int32)


def _touching(i, j, C):
    """Unordered pairs of different segments as one sorted int64 code each."""
    k = (i != j) & (i > 0) & (j > 0)
    i, j = i[k], j[k]
    return np.unique(np.minimum(i, j) * (C + 1) + np.maximum(i, j))


def _merge_rounds(C, size, csum, pairs, min_size, max_size):
    """The merge rounds of enforce_connectivity over the fragments 1..C (size (C+1,), csum (C+1, nch) float64, pairs: the touching
    codes) -> root (C+1,): every fragment's segment, named by the lowest fragment number in it."""
    root = np.arange(C + 1)
    while True:
        i, j = pairs // (C + 1), pairs % (C + 1)
        c, t = np.concatenate([i, j]), np.concatenate([j, i])
        k = size[c] < min_size
        c, t = c[k], t[k]
        if len(c) == 0:
            break
        mean = csum / np.maximum(size, 1)[:, None]
        order = np.lexsort((t, ((mean[c] - mean[t]) ** 2).sum(1), size[c] + size[t] > max_size, c))
        c, t = c[order], t[order]
        k = np.concatenate([[True], c[1:] != c[:-1]])                    # the best neighbour of every small segment
        c, t = c[k], t[k]
        n, group = csgraph.connected_components(sparse.coo_matrix((np.ones(len(c), np.int8), (c, t)), shape=(C + 1, C + 1)), directed=False)
        lowest = np.full(n, C + 1)
        np.minimum.at(lowest, group, np.arange(C + 1))
        to = lowest[group]                                               # every segment of a group -> the group's lowest number
        root = to[root]
        size = np.bincount(to, weights=size, minlength=C + 1)
        csum = np.stack([np.bincount(to, weights=csum[:, k], minlength=C + 1) for k in range(csum.shape[1])], 1)
        pairs = _touching(to[i], to[j], C)
    return root


def slic_raw(img_u8, mask, sp_size, sp_regul, n_iter=10, device="cuda:0"):
    """The GPU half of slic(): prepare, then `n_iter` assign / update rounds from the grid start.  -> labels (H,W) int32 as the last
    assignment left them (0 outside the mask, k + 1 = centre k; not yet connected), and the step S."""
    import torch
    from . import ops
    if sp_regul <= 0:
        raise ValueError("slic. regularisation must be positive")                       # pipelines.py:263-264
    _, S, pos = slic_geometry(mask, sp_size)
    dev = ops.select_device(device)
    m = (sp_size * sp_regul) ** 1.5                                                     # superpixels.py:59
    lab = ops.slic_prepare(torch.from_numpy(img_u8).to(dev), float(img_u8.min()), float(img_u8.max()), m)
    t_mask = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    t_pos = torch.from_numpy(pos.astype(np.float32)).to(dev)
    centres = torch.cat([t_pos, lab[:, t_pos[:, 0].long(), t_pos[:, 1].long()].t()], 1).contiguous()
    labels = None
    for _ in range(n_iter):
        labels = ops.slic_assign(lab, t_mask, centres, S, labels)
        ops.slic_update(lab, labels, centres)
    return labels.cpu().numpy(), S


def slic(img_u8, mask, sp_size, sp_regul, n_iter=10, device="cuda:0", cc_device=None):
    """Masked SLIC superpixels of an (H,W,3) uint8 image (imsegm/superpixels.py:53-64 with the deterministic start of slic_geometry):
    (H,W) int32 labels, 0 outside the mask, 1..N inside, every superpixel 4-connected.  The pixel work runs on `device`; the
    connectivity repair (fragments below half the mean segment size S^2 are merged away) on the host, its per-pixel half on `cc_device`
    when one is given (enforce_connectivity)."""
    img_u8 = as_u8(img_u8)
    mask = np.asarray(mask).reshape(img_u8.shape[:2]) > 0
    labels, S = slic_raw(img_u8, mask, sp_size, sp_regul, n_iter, device)
    return enforce_connectivity(labels, 0.5 * S * S, img_u8, cc_device=cc_device)


def superpixel_features(img_u8, labels, device="cuda:0"):
    """-> count (N,), centroids (N,2) (y, x), features (N,9) float64: per-channel mean, median, meanGrad of the 0..255 values
    (pipelines.py:270-272; NaN -> 0) for the superpixels 1..N of `labels`."""
    import torch
    from . import ops
    img_u8 = as_u8(img_u8)
    labels = np.ascontiguousarray(labels, np.int32)
    N = int(labels.max())
    dev = ops.select_device(device)
    count, feat = ops.slic_features(torch.from_numpy(img_u8).to(dev), torch.from_numpy(labels).to(dev), N)
    feat = feat.cpu().numpy().astype(np.float64)
    feat[np.isnan(feat)] = 0
    return count.cpu().numpy(), feat[:, :2], feat[:, 2:]


# ---- the class model: standardised features -> full-covariance Gaussian mixture (graph_cuts.py:73-163) --------------------------------
def standardise(X):
    """sklearn.preprocessing.StandardScaler().fit_transform: zero mean, unit (population) deviation; a constant column stays 0."""
    X = np.asarray(X, np.float64)
    sd = X.std(0)
    return (X - X.mean(0)) / np.where(sd > 0, sd, 1.0)


def _kmeanspp(X, k, rs):
    n = len(X)
    c = X[rs.randint(n)]
    out = [c]
    d2 = ((X - c) ** 2).sum(1)
    for _ in range(1, k):
        tot = d2.sum()
        i = rs.randint(n) if tot <= 0 else min(int(np.searchsorted(np.cumsum(d2), rs.random_sample() * tot)), n - 1)
        out.append(X[i])
        d2 = np.minimum(d2, ((X - X[i]) ** 2).sum(1))
    return np.stack(out)


def _log_prob(X, weights, means, covs):
    """log(weight_k N(x | mean_k, cov_k)) (n, k)."""
    n, d = X.shape
    lp = np.empty((n, len(weights)))
    for k in range(len(weights)):
        L = np.linalg.cholesky(covs[k])
        y = np.linalg.solve(L, (X - means[k]).T)
        lp[:, k] = -0.5 * (d * np.log(2 * np.pi) + (y * y).sum(0)) - np.log(np.diag(L)).sum() + np.log(weights[k])
    return lp


def _e_step(X, model):
    lp = _log_prob(X, *model)
    mx = lp.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(lp - mx).sum(1))
    return float(lse.mean()), np.exp(lp - lse[:, None])


def _m_step(X, resp, reg):
    n, d = X.shape
    nk = resp.sum(0) + 10 * np.finfo(np.float64).eps
    means = resp.T @ X / nk[:, None]
    covs = np.empty((len(nk), d, d))
    for k in range(len(nk)):
        diff = X - means[k]
        covs[k] = (resp[:, k] * diff.T) @ diff / nk[k] + reg * np.eye(d)
    return nk / n, means, covs


def fit_mixture(X, nb_classes, seed=0, n_init=9, max_iter=99, tol=1e-3, reg_covar=1e-6):
    """mixture.GaussianMixture(n_components, 'full', n_init = int(sqrt(99)), max_iter = 99) (graph_cuts.py:113-115), deterministic:
    every restart starts from the hard assignment to k-means++ centres drawn from np.random.RandomState(seed); EM until the mean
    log-likelihood moves less than `tol`; the restart with the best lower bound is kept.  -> (weights, means, covariances)."""
    X = np.asarray(X, np.float64)
    if len(X) < nb_classes:
        raise ValueError(f"{len(X)} superpixels cannot carry {nb_classes} classes")
    rs = np.random.RandomState(seed)
    best, best_lb = None, -np.inf
    for _ in range(n_init):
        c = _kmeanspp(X, nb_classes, rs)
        resp = np.zeros((len(X), nb_classes))
        resp[np.arange(len(X)), ((X[:, None, :] - c[None]) ** 2).sum(2).argmin(1)] = 1.0
        try:
            model = _m_step(X, resp, reg_covar)
            lb = -np.inf
            for _ in range(max_iter):
                prev = lb
                lb, resp = _e_step(X, model)
                model = _m_step(X, resp, reg_covar)
                if abs(lb - prev) < tol:
                    break
            lb, _ = _e_step(X, model)
        except np.linalg.LinAlgError:                    # a collapsed component: this restart is void
            continue
        if lb > best_lb:
            best, best_lb = model, lb
    if best is None:
        raise RuntimeError("every mixture restart collapsed")
    return best


def predict_proba(model, X):
    return _e_step(np.asarray(X, np.float64), model)[1]


# ---- the graph cut (graph_cuts.py:523-555, 574-660, 663-751) --------------------------------------------------------------------
def superpixel_edges(labels):
    """The 4-connected pairs of different superpixels, (E,2) zero-based, i < j, sorted; label 0 takes no part (graph_cuts.py:612-617)."""
    labels = np.asarray(labels)
    e = np.concatenate([np.stack([labels[:, :-1].ravel(), labels[:, 1:].ravel()], 1),
                        np.stack([labels[:-1].ravel(), labels[1:].ravel()], 1)]).astype(np.int64)
    e = e[(e[:, 0] != e[:, 1]) & (e.min(1) > 0)]
    e.sort(axis=1)
    return np.unique(e, axis=0) - 1 if len(e) else np.zeros((0, 2), np.int64)


def edge_weights(edges, features_std, centroids):
    """gc_edge_type = 'features' (graph_cuts.py:637-659): exp(-d / (2 std(d)^2)) with d the Euclidean distance of the two ends'
    standardised features, over the centroid distance relative to its mean, clipped to [1e-3, 1e3]."""
    if len(edges) == 0:
        return np.zeros(0)
    d = np.linalg.norm(features_std[edges[:, 0]] - features_std[edges[:, 1]], axis=1)
    sd = d.std()
    w = np.exp(-d / (2 * sd ** 2)) if sd > 0 else np.ones(len(d))
    sp = np.linalg.norm(np.asarray(centroids, np.float64)[edges[:, 0]] - np.asarray(centroids, np.float64)[edges[:, 1]], axis=1)
    w = w / (sp / sp.mean())
    return np.clip(w, 1.0 / MIN_MAX_EDGE_WEIGHT, MIN_MAX_EDGE_WEIGHT)


def unary_cost(proba):
    return -np.log(np.clip(proba, MIN_UNARY_PROB, 1 - MIN_UNARY_PROB))                  # graph_cuts.py:523-540


def energy(labels, unary, edges, weights, gc_regul):
    """sum_i unary[i, l_i] + gc_regul * sum_(i,j) w_ij [l_i != l_j]."""
    labels = np.asarray(labels)
    e = float(unary[np.arange(len(labels)), labels].sum())
    if len(edges):
        e += float(gc_regul * (weights * (labels[edges[:, 0]] != labels[edges[:, 1]])).sum())
    return e


def _expansion_move(labels, alpha, unary, edges, weights, gc_regul):
    """The best labelling reachable by letting any set of nodes switch to `alpha`: one s-t minimum cut (Boykov, Veksler, Zabih 2001;
    the pair terms are decomposed as in Kolmogorov & Zabih 2004).  x_i = 0 (source side) keeps l_i, x_i = 1 takes alpha."""
    n = len(labels)
    c0 = unary[np.arange(n), labels].astype(np.float64)
    c1 = unary[:, alpha].astype(np.float64)
    i, j = (edges[:, 0], edges[:, 1]) if len(edges) else (np.zeros(0, np.int64),) * 2
    w = gc_regul * np.asarray(weights, np.float64)
    A = w * (labels[i] != labels[j])            # E(0,0)
    B = w * (labels[i] != alpha)                # E(0,1)
    Cc = w * (labels[j] != alpha)               # E(1,0);  E(1,1) = 0
    # E = A + (C - A) x_i - C x_j + (B + C - A) (1 - x_i) x_j, the last coefficient >= 0 for a metric
    np.add.at(c1, i, Cc - A)
    np.add.at(c1, j, -Cc)
    pair = B + Cc - A
    low = np.minimum(c0, c1)
    c0, c1 = c0 - low, c1 - low
    # integer capacities for scipy's maximum_flow, scaled so that the flow stays below 2^30
    bound = max(c0.sum(), c1.sum(), pair.max() if len(pair) else 0.0)
    if not bound > 0:                           # nothing to gain or lose (e.g. every node carries alpha already)
        return labels.copy()
    scale = (2.0 ** 30) / bound
    s, t = n, n + 1
    rows = np.concatenate([np.full(n, s), np.arange(n), i])
    cols = np.concatenate([np.arange(n), np.full(n, t), j])
    caps = np.rint(np.concatenate([c1, c0, pair]) * scale).astype(np.int64)
    keep = caps > 0
    cap = sparse.csr_matrix((caps[keep].astype(np.int32), (rows[keep], cols[keep])), shape=(n + 2, n + 2))
    flow = csgraph.maximum_flow(cap, s, t).flow
    residual = (cap - flow).tocsr()
    residual.data[residual.data < 0] = 0
    residual.eliminate_zeros()
    reach = csgraph.breadth_first_order(residual, s, directed=True, return_predecessors=False)
    x = np.ones(n + 2, bool)
    x[reach] = False
    out = labels.copy()
    out[x[:n]] = alpha
    return out


def graph_cut(unary, edges, weights, gc_regul=GC_REGUL):
    """Minimise energy() by alpha-expansion from the unary argmin until no move lowers it (gco's 'expansion', n_iter = -1;
    graph_cuts.py:733-748).  gc_regul <= 0: the unary argmin itself."""
    unary = np.asarray(unary, np.float64)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    labels = unary.argmin(1)
    if gc_regul <= 0 or len(edges) == 0:
        return labels
    best = energy(labels, unary, edges, weights, gc_regul)
    improved = True
    while improved:
        improved = False
        for alpha in range(unary.shape[1]):
            cand = _expansion_move(labels, alpha, unary, edges, weights, gc_regul)
            e = energy(cand, unary, edges, weights, gc_regul)
            if e < best - 1e-12 * max(1.0, abs(best)):
                labels, best, improved = cand, e, True
    return labels


# ---- from superpixels to the two masks ------------------------------------------------------------------------------------------
def segment_superpixels(labels, features, centroids, nb_classes=3, seed=0, gc_regul=GC_REGUL):
    """Superpixel features -> class per superpixel: model (estim_model_classes_group), probabilities, graph cut
    (segment_color2d_slic_features_model_graphcut, loaders.py:171-179).  -> (classes (N,), proba (N, nb_classes))."""
    Xs = standardise(features)
    model = fit_mixture(Xs, nb_classes, seed)
    proba = predict_proba(model, Xs)
    edges = superpixel_edges(labels)
    w = edge_weights(edges, Xs, centroids)
    return graph_cut(unary_cost(proba), edges, w, gc_regul), proba


def masks_from_classes(labels, classes, valid):
    """loaders.py:181-205: seg = (class + 1) * valid; the most frequent non-zero label of the central crop is the periodic one."""
    valid = np.asarray(valid).reshape(labels.shape) > 0.5
    cls_img = np.concatenate([[-1], np.asarray(classes, np.int64)])[labels]
    seg = np.uint8((cls_img + 1) * valid)
    h, w = seg.shape
    crop = seg[h // 4:h // 4 * 3, w // 4:w // 4 * 3].reshape(-1)
    counts = np.bincount(crop, minlength=2)[1:]
    period_label = int(counts.argmax()) + 1
    period = seg == period_label
    non_period = (seg > 0) & ~period
    return seg, period, non_period


def initial_segmentation(img, valid_mask, nb_classes=3, sp_size=20, sp_regul=0.1, seed=0, device="cuda:0", cc_device=None):
    """The initial periodic / non-periodic masks of an image (loaders.py:162-205).  img (H,W,3) uint8 (or float in [0,1]), valid_mask
    (H,W[,1]) with > 0.5 = valid.  -> dict(period_mask, non_period_mask (H,W) bool, seg (H,W) uint8: 0 invalid, class + 1 elsewhere,
    slic (H,W) int32 superpixels, proba (N, nb_classes) per superpixel)."""
    img_u8 = as_u8(img)
    valid = np.asarray(valid_mask).reshape(img_u8.shape[:2]) > 0.5
    sp = slic(img_u8, valid, sp_size, sp_regul, device=device, cc_device=cc_device)
    _, centroids, feats = superpixel_features(img_u8, sp, device=device)
    classes, proba = segment_superpixels(sp, feats, centroids, nb_classes, seed)
    seg, period, non_period = masks_from_classes(sp, classes, valid)
    return dict(period_mask=period, non_period_mask=non_period, seg=seg, slic=sp, proba=proba)
