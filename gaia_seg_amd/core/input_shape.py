"""Applying ``data.input_shape`` to a batch (elastic input resolution).

The value forms and the target size are ``core.model_space.resolve_input_shape``'s; the resampling is
one ``gs_batch_rescale`` launch (hip/ops.py batch_rescale).  Training rescales image and labels,
evaluation the image only: its labels stay at ``ori_shape``, where the test epilogue brings the
predictions back to.
"""
from .model_space import resolve_input_shape

INPUT_SHAPE_KEY = "data.input_shape"


def _scaled_meta(m, h, w, H, W):
    """A copy of one img_metas entry for the rescaled image: img_shape / pad_shape / scale_factor
    follow the new size (scale_factor keeps this project's form, a float on the height), ori_shape
    and everything else stay."""
    m = dict(m)
    c = tuple(m.get("pad_shape", (h, w, 3)))[2:]
    ih, iw = tuple(m.get("img_shape", (h, w, 3)))[:2]
    if (ih, iw) == (h, w):
        m["img_shape"] = (H, W) + c
    else:   # (a crop smaller than its padded canvas keeps its share of it)
        m["img_shape"] = ((2 * ih * H + h) // (2 * h), (2 * iw * W + w) // (2 * w)) + c
    m["pad_shape"] = (H, W) + c
    m["scale_factor"] = m.get("scale_factor", 1.0) * (H / h)
    return m


def rescale_batch(batch, value, with_labels=True):
    """``batch`` (dict(img, img_metas[, gt_semantic_seg])) under ``data.input_shape = value``:
    returns (batch, (H, W)).  The input dict, its tensors and its metas are never modified (loaders
    hand the same batch objects out again); a target equal to the batch size returns ``batch`` itself
    without a launch.  ``with_labels=False`` leaves gt_semantic_seg as it is (evaluation)."""
    from ..hip import ops
    img = batch["img"]
    h, w = int(img.shape[-2]), int(img.shape[-1])
    H, W = resolve_input_shape(value, h, w)
    if (H, W) == (h, w):
        return batch, (h, w)
    gt = batch.get("gt_semantic_seg") if with_labels else None
    out = dict(batch)
    out["img"], new_gt = ops.batch_rescale(img, gt, (H, W))
    if gt is not None:
        out["gt_semantic_seg"] = new_gt
    out["img_metas"] = [_scaled_meta(m, h, w, H, W) for m in batch["img_metas"]]
    return out, (H, W)
