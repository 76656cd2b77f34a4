"""The model file of a fitted NPP-Net: one .npz that np.load(..., allow_pickle=False) reads.  NumPy only (no torch, no library), so
that a file can be written, read and checked without a GPU.

What it holds (format_version 1):
  <state-dict name>          the network's tensors under the reference's names and shapes (models/networks.py:40-49 / :128-140:
                             weights (out, in), biases (out,)), so that
                                 net.load_state_dict({k: torch.from_numpy(v) for k, v in modelfile.state_dict(d).items()}, strict=False)
                             loads them into the reference's NPP_Net / NPP_Net_top1 (alpha_linear, unused there, stays missing)
  npp/latents                (6,) the adaptive pixel loss latents [alpha(3) | scale(3)] (models/helpers.py:8-9)
  npp/angles_deg, npp/periods  (K, 2) the embedder's selected_angles / selected_periods (models/embedder.py:93-148)
  npp/freqs                  (10,) the Fourier frequencies (embedder.py:26)
  npp/freq_offsets           (5,) freq_offsets
  npp/res                    (2,) int64 (H, W) of the fit: the frame its pixel coordinates live in
  npp/K, npp/width, npp/out_act, npp/format_version   int64 scalars (out_act: 1 sigmoid, 2 tanh; helpers.py:55-58)
  npp/meta/<key>             optional string metadata (task, image name, iterations, ...)
It is not a checkpoint to resume training from: no Adam moments, no random streams (fit.CompletionFit.state_dict has those)."""
import numpy as np

FORMAT_VERSION = 1
PREFIX = "npp/"
META = PREFIX + "meta/"
N_FREQ, N_OFF, E_PER_PROPOSAL = 10, 5, 462


def param_shapes(K, width):
    """{state-dict name: shape} of the tensors the forward uses, in the blob's order (include/npp_hip.h npp_param_layout): the eight
    snake layers (skip into layer 5), feature_linear1, for K > 1 scale_linears.0 and feature_linear2, pos_linears.0, rgb_linear."""
    E, W = E_PER_PROPOSAL, int(width)
    sh = {}
    for i in range(8):
        sh[f"periodic_linears.{i}.weight"] = (W, E if i == 0 else (W + E if i == 5 else W))
        sh[f"periodic_linears.{i}.bias"] = (W,)
    sh["feature_linear1.weight"], sh["feature_linear1.bias"] = (W, W), (W,)
    if K > 1:
        sh["scale_linears.0.weight"], sh["scale_linears.0.bias"] = (W, W + (K - 1) * E), (W,)
        sh["feature_linear2.weight"], sh["feature_linear2.bias"] = (W, W), (W,)
    sh["pos_linears.0.weight"], sh["pos_linears.0.bias"] = (W // 2, 2 * W if K > 1 else W), (W // 2,)
    sh["rgb_linear.weight"], sh["rgb_linear.bias"] = (3, W // 2), (3,)
    return sh


def write(path, params, latents, angles_deg, periods, freqs, res, width, out_act=1, freq_offsets=(0.0, -1.0, 1.0, 0.5, -0.5), **meta):
    """params: {state-dict name: array} (any extra names are ignored); meta: string-valued keyword arguments.  Writes `path`
    (np.savez_compressed appends .npz when the name lacks it).  Validates everything it writes."""
    a = np.asarray(angles_deg, np.float32).reshape(-1, 2)
    K = a.shape[0]
    arrays = {}
    for name, shp in param_shapes(K, width).items():
        if name not in params:
            raise ValueError(f"model file: tensor {name} missing from the parameters")
        v = np.asarray(params[name], np.float32)
        if v.size != int(np.prod(shp)):
            raise ValueError(f"model file: tensor {name} has {v.size} values, expected shape {shp}")
        arrays[name] = v.reshape(shp)
    arrays[PREFIX + "latents"] = np.asarray(latents, np.float32).reshape(6)
    arrays[PREFIX + "angles_deg"] = a
    arrays[PREFIX + "periods"] = np.asarray(periods, np.float32).reshape(K, 2)
    arrays[PREFIX + "freqs"] = np.asarray(freqs, np.float32).reshape(N_FREQ)
    arrays[PREFIX + "freq_offsets"] = np.asarray(freq_offsets, np.float32).reshape(N_OFF)
    arrays[PREFIX + "res"] = np.asarray([int(res[0]), int(res[1])], np.int64)
    for k, v in (("K", K), ("width", int(width)), ("out_act", int(out_act)), ("format_version", FORMAT_VERSION)):
        arrays[PREFIX + k] = np.asarray(v, np.int64)
    for k, v in meta.items():
        if v is not None:
            arrays[META + k] = np.asarray(str(v))
    _check(arrays, str(path))
    np.savez_compressed(path, **arrays)


def read(path):
    """-> dict: params {name: array} (reference names and shapes), latents, angles_deg, periods, freqs, freq_offsets, res (H, W),
    K, width, out_act, format_version, meta {key: str}.  ValueError naming the problem for a file that is not a model file of a
    known version, lacks a tensor or holds one of the wrong shape; FileNotFoundError for a missing file."""
    try:
        with np.load(path, allow_pickle=False) as f:
            arrays = {k: f[k] for k in f.files}
    except FileNotFoundError:
        raise
    except Exception as e:                                  # truncated / damaged archive: zipfile.BadZipFile, EOFError, zlib.error, ...
        raise ValueError(f"{path}: not a readable model file ({type(e).__name__}: {e})") from e
    return _check(arrays, str(path))


def state_dict(d):
    """The network tensors of a read() result (or of the raw archive's arrays), for load_state_dict(..., strict=False)."""
    p = d.get("params", d)
    return {k: v for k, v in p.items() if not k.startswith(PREFIX)}


def _need(arrays, key, where, shape=None):
    if key not in arrays:
        raise ValueError(f"{where}: {key} missing")
    v = arrays[key]
    if shape is not None and tuple(v.shape) != tuple(shape):
        raise ValueError(f"{where}: {key} has shape {tuple(v.shape)}, expected {tuple(shape)}")
    return v


def _scalar(arrays, key, where):
    v = _need(arrays, key, where)
    if v.shape != () or v.dtype.kind not in "iu":
        raise ValueError(f"{where}: {key} must be an integer scalar, got {v.dtype} {v.shape}")
    return int(v)


def _check(arrays, where):
    if PREFIX + "format_version" not in arrays:
        raise ValueError(f"{where}: not an NPP-Net model file ({PREFIX}format_version missing)")
    ver = _scalar(arrays, PREFIX + "format_version", where)
    if ver != FORMAT_VERSION:
        raise ValueError(f"{where}: format_version {ver} unknown (this build reads {FORMAT_VERSION})")
    K, width, out_act = (_scalar(arrays, PREFIX + k, where) for k in ("K", "width", "out_act"))
    if not 1 <= K <= 5:
        raise ValueError(f"{where}: K = {K} (1..5 proposals)")
    if width < 2 or width % 2:
        raise ValueError(f"{where}: width = {width}")
    if out_act not in (1, 2):
        raise ValueError(f"{where}: out_act = {out_act} (1 sigmoid or 2 tanh: the output nonlinearities a fit trains with)")
    out = {"K": K, "width": width, "out_act": out_act, "format_version": ver, "params": {}, "meta": {}}
    for name, shp in param_shapes(K, width).items():
        v = _need(arrays, name, where, shp)
        if v.dtype != np.float32:
            raise ValueError(f"{where}: {name} is {v.dtype}, expected float32")
        out["params"][name] = v
    for key, shp in (("latents", (6,)), ("angles_deg", (K, 2)), ("periods", (K, 2)), ("freqs", (N_FREQ,)), ("freq_offsets", (N_OFF,))):
        out[key] = np.asarray(_need(arrays, PREFIX + key, where, shp), np.float32)
    res = _need(arrays, PREFIX + "res", where, (2,))
    if res.dtype.kind not in "iu" or int(res.min()) < 1:
        raise ValueError(f"{where}: res {res.tolist()} must be two positive integers")
    out["res"] = (int(res[0]), int(res[1]))
    for k, v in arrays.items():
        if k.startswith(META):
            out["meta"][k[len(META):]] = str(v)
    return out
