"""Drawing a label map over its image: mmseg's ``show_result`` blend as one HIP kernel
(``gs_seg_overlay``, csrc/tta.hip) plus the Pillow file I/O around it."""
import numpy as np
import torch

from ..hip import lib as _lib
from ..hip.runtime import current_stream_ptr


def read_bgr(path):
    """A decoded image file as uint8 [H, W, 3] in BGR (what cv2.imread gives)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.array(im.convert("RGB"), dtype=np.uint8)[:, :, ::-1])


def write_bgr(path, img):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]), "RGB").save(path)


def overlay(seg, img, palette, opacity=0.5, device="cuda"):
    """uint8(img * (1 - opacity) + palette[seg] * opacity): ``seg`` [H, W] integer labels (array or
    tensor), ``img`` uint8 BGR [H, W, 3], ``palette`` [C, 3] RGB.  A label outside [0, C) is drawn
    black.  Returns the blended BGR image as a numpy array."""
    if not 0 < opacity <= 1.0:
        raise ValueError("opacity must be in (0, 1], got %r" % (opacity,))
    img_t = torch.as_tensor(np.ascontiguousarray(img))
    if img_t.dtype != torch.uint8 or img_t.dim() != 3 or img_t.shape[2] != 3:
        raise TypeError("expected a uint8 image [H, W, 3]")
    seg_t = torch.as_tensor(seg).to(device).to(torch.int64).contiguous()
    h, w = int(img_t.shape[0]), int(img_t.shape[1])
    if tuple(seg_t.shape) != (h, w):
        raise ValueError("label map %s and image %s differ in size" % (tuple(seg_t.shape), (h, w)))
    pal = torch.as_tensor(np.asarray(palette)).to(torch.uint8).to(device).contiguous()
    if pal.dim() != 2 or pal.shape[1] != 3:
        raise ValueError("palette must be [num_classes, 3]")
    img_t = img_t.to(device).contiguous()
    out = torch.empty_like(img_t)
    _lib.check(_lib.load().gs_seg_overlay(seg_t.data_ptr(), img_t.data_ptr(), pal.data_ptr(),
                                          int(pal.shape[0]), h, w, float(opacity), out.data_ptr(),
                                          current_stream_ptr()), "gs_seg_overlay")
    return out.cpu().numpy()
