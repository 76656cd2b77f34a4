"""The remapping task's blur detection on the GPU (NPP_remapping/blur_detection.py:13-60): a drop-in for io.get_blur_map.

What runs where: the gray conversion, the per-pixel singular-value share (float64 one-sided Jacobi on every 20 x 20 block) and the
erosion / dilation are HIP kernels (csrc/npp_blur.hip); the normalisation to [0, 1], the percentile and the `>` between them are a
few NumPy passes over H W numbers in float64 on the host (`finish`), which is also where the caller wants the map."""
import numpy as np
import torch

from . import ops

WIN_SIZE = 10          # the window the kernel is compiled for (blur_detection.py:13's default, the only one the loaders use)


def _to_dev_u8(a, dev, name):
    if isinstance(a, torch.Tensor):
        t = a.to(dev)
    else:
        a = np.asarray(a)
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8:
        raise TypeError(f"{name}: expected uint8 (or bool), got {t.dtype}")
    return t.contiguous()


def sv_share(gray_u8, sv_num=3, device="cuda:0"):
    """(H,W) uint8 gray -> device tensor (H,W) float64, the RAW share sum(s[:sv_num]) / (sum(s) + 1e-6) of blur_detection.py:32-46."""
    if not 1 <= int(sv_num) <= 2 * WIN_SIZE:
        raise ValueError(f"sv_num must be in 1..{2 * WIN_SIZE}, got {sv_num}")
    dev = ops.select_device(device)
    g = _to_dev_u8(gray_u8, dev, "gray_u8")
    if g.dim() != 2:
        raise ValueError("gray_u8: expected (H, W)")
    if g.shape[0] <= WIN_SIZE or g.shape[1] <= WIN_SIZE:
        raise ValueError("image smaller than the blur window")
    return ops.blur_sv_share(g, int(sv_num))


def _morph(mask, iterations, device, dilate):
    if int(iterations) < 1:
        raise ValueError("iterations must be >= 1 (scipy's 'repeat until nothing changes' form is not built)")
    dev = ops.select_device(device)
    return ops.binary_morph(_to_dev_u8(mask, dev, "mask"), int(iterations), dilate)


def binary_erosion(mask, iterations=1, device="cuda:0"):
    """scipy.ndimage.binary_erosion(mask, iterations=iterations) with its defaults (cross, border_value 0) -> device (H,W) uint8."""
    return _morph(mask, iterations, device, False)


def binary_dilation(mask, iterations=1, device="cuda:0"):
    """scipy.ndimage.binary_dilation(mask, iterations=iterations) with its defaults -> device (H,W) uint8 0 / 1."""
    return _morph(mask, iterations, device, True)


def finish(raw, thresh=50):
    """Host side of blur_detection.py:48-52 in float64: raw share (H,W) -> (blur_map normalised to [0, 1], the binary map
    blur_map > np.percentile(blur_map, thresh), NumPy's linear interpolation)."""
    blur = np.asarray(raw, np.float64)
    blur = (blur - blur.min()) / (blur.max() - blur.min())
    return blur, blur > np.percentile(blur, thresh)


def get_blur_map(img_u8, win_size=10, sv_num=3, thresh=50, device="cuda:0"):
    """io.get_blur_map's contract, computed on `device`: (blur_map float64 (H,W) in [0, 1], clear mask float64 (H,W) in {0, 255})."""
    if win_size != WIN_SIZE:
        raise ValueError(f"the GPU blur detection is built for win_size = {WIN_SIZE} only (got {win_size}); "
                         "io.get_blur_map handles other window sizes on the host")
    dev = ops.select_device(device)
    img = _to_dev_u8(img_u8, dev, "img_u8")
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("img_u8: expected (H, W, 3)")
    if img.shape[0] <= WIN_SIZE or img.shape[1] <= WIN_SIZE:
        raise ValueError("image smaller than the blur window")
    raw = sv_share(ops.rgb_to_gray_u8(img), sv_num, dev)
    blur, binary = finish(raw.cpu().numpy(), thresh)
    binary = binary_erosion(binary, 20, dev)                     # blur_detection.py:54
    binary = binary_dilation(binary, 40, dev)                    # :56
    return blur, (1 - binary.cpu().numpy()).astype(np.float64) * 255
