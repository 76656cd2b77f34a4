"""4-connected components of label images and binary masks (include/npp_hip.h npp_cc_*, csrc/npp_regions.hip):
labelling in scipy.ndimage.label's numbering, per-component statistics, and the two mask operations the segmentation task's final
mask needs -- scipy.ndimage.binary_fill_holes and skimage.morphology.remove_small_objects(connectivity=1) -- built on them.

device=None or "cpu": the library's plain C++ twins on NumPy arrays, no GPU.  A CUDA device: the HIP kernels; tensors stay on the
device, a NumPy input is uploaded and the result comes back as a NumPy array (the type that went in).  A CUDA tensor passed with
device=None runs on its own device.  Both paths follow one definition and give identical integers."""
import numpy as np
import torch

from . import ops


def _resolve(x, device):
    """-> (torch.device or None for the host path, whether the result goes back to NumPy)."""
    is_t = isinstance(x, torch.Tensor)
    if device is None and is_t and x.is_cuda:
        return x.device, False
    if device is None or str(device) == "cpu":
        return None, not is_t
    dev = ops.select_device(device)
    if dev.type != "cuda":
        raise ValueError(f"device: None, 'cpu' or a CUDA device, got {device!r}")
    return dev, not is_t


def _as_labels_np(x):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.ndim != 2:
        raise ValueError(f"expected an (H, W) label image or mask, got shape {a.shape}")
    return np.ascontiguousarray(a != 0 if a.dtype == bool or a.dtype.kind == "f" else a, np.int32)


def _as_labels_t(x, dev):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() != 2:
        raise ValueError(f"expected an (H, W) label image or mask, got shape {tuple(t.shape)}")
    t = t.to(dev)
    if t.dtype == torch.bool or t.dtype.is_floating_point:
        t = t != 0
    return t.to(torch.int32).contiguous()


def _out(t, like_numpy):
    return t.cpu().numpy() if like_numpy else t


def label(x, device=None):
    """(H,W) label image (0 = outside, any other value a class; bool / float: a mask, non-zero = set) -> (numbered, C): the
    4-connected components of equal non-zero values numbered 1..C in raster order of first appearance, 0 outside, as (H,W) int32 --
    scipy.ndimage.label(mask)'s result for a mask."""
    dev, to_np = _resolve(x, device)
    if dev is None:
        numbered, C = ops.cc_number_host(ops.cc_label_host(_as_labels_np(x)))
        return (numbered if to_np else torch.from_numpy(numbered)), C
    numbered, count = ops.cc_number(ops.cc_label(_as_labels_t(x, dev)))
    return _out(numbered, to_np), int(count.item())


def component_stats(numbered, C, values_u8=None):
    """Per component 1..C of label()'s image (at index c - 1) -> (sizes (C,) int64, sums (C,nch) int64 of the (H,W,nch <= 4) uint8
    image `values_u8` (None: nch = 0), border (C,) uint8: 1 = touches the image border, boxes (C,4) int32: first row, first column,
    last row, last column).  NumPy in: the host twin, NumPy out; CUDA tensors in: the kernels, tensors out."""
    if isinstance(numbered, torch.Tensor) and numbered.is_cuda:
        if values_u8 is not None and not isinstance(values_u8, torch.Tensor):
            values_u8 = torch.from_numpy(np.ascontiguousarray(values_u8))
        if values_u8 is not None:
            values_u8 = values_u8.to(numbered.device).contiguous()
        return ops.cc_stats(numbered.contiguous(), C, values_u8)
    if isinstance(numbered, torch.Tensor):
        numbered = numbered.numpy()
    if isinstance(values_u8, torch.Tensor):
        values_u8 = values_u8.cpu().numpy()
    return ops.cc_stats_host(numbered, C, values_u8)


def _select(numbered, flags):
    """flags (C,) per component -> the (H,W) bool image of the pixels whose component is flagged."""
    if isinstance(numbered, torch.Tensor):
        lut = torch.cat([torch.zeros(1, dtype=torch.bool, device=numbered.device), flags.to(torch.bool)])
        return lut[numbered.long()]
    return np.concatenate([[False], np.asarray(flags, bool)])[numbered]


def _as_mask(x, dev):
    if dev is None:
        a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        return a != 0
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dev) != 0


def _mask_out(m, dev, to_np):
    if dev is None:
        return m if to_np else torch.from_numpy(m)
    return _out(m, to_np)


def fill_holes(mask, device=None):
    """scipy.ndimage.binary_fill_holes(mask) with its default structure: mask | (the 4-connected components of ~mask that do not touch
    the image border).  (H,W) -> (H,W) bool."""
    dev, to_np = _resolve(mask, device)
    m = _as_mask(mask, dev)
    numbered, C = label(~m, dev)
    if C == 0:
        return _mask_out(m, dev, to_np)
    _, _, border, _ = component_stats(numbered, C)
    return _mask_out(m | _select(numbered, border == 0), dev, to_np)


def remove_small_objects(mask, min_size, device=None):
    """skimage.morphology.remove_small_objects(mask, min_size, connectivity=1): the 4-connected components with fewer than `min_size`
    pixels are cleared.  (H,W) -> (H,W) bool."""
    dev, to_np = _resolve(mask, device)
    m = _as_mask(mask, dev)
    numbered, C = label(m, dev)
    if C == 0:
        return _mask_out(m, dev, to_np)
    sizes, _, _, _ = component_stats(numbered, C)
    return _mask_out(_select(numbered, sizes >= min_size), dev, to_np)
