"""Batch unpackers used by the epochers (ref: contrastyou/epocher/_utils.py:25-33), the contrastive label generators (ref :52-86) and
``unfold_position`` (ref :36-49)."""
from typing import List, Sequence


def _to(x, device, non_blocking):
    if isinstance(x, (list, tuple)):
        return [_to(v, device, non_blocking) for v in x]
    return x.to(device, non_blocking=non_blocking)


def preprocess_input_with_twice_transformation(data, device, non_blocking=True):
    [(image, target), (image_tf, target_tf)] = _to(data[0], device, non_blocking)
    return (image, target), (image_tf, target_tf), data[1], data[2], data[3]


def preprocess_input_with_single_transformation(data, device, non_blocking=True):
    return data[0][0].to(device, non_blocking=non_blocking), data[0][1].to(device, non_blocking=non_blocking), data[1], data[2], data[3]


class GlobalLabelGenerator:
    """Contrastive class ids of a batch (ref contrastyou/epocher/_utils.py:52-69): per sample, the enabled attributes -- patient
    first, then partition -- joined as ``"_" + patient`` / ``"_" + partition``; the id is the rank of the sample's string among the
    batch's sorted unique strings.  Returns a list of ints (they fit int32: at most the batch size)."""

    def __init__(self, contrastive_on_patient: bool = False, contrastive_on_partition: bool = True) -> None:
        self._contrastive_on_patient = contrastive_on_patient
        self._contrastive_on_partition = contrastive_on_partition

    def __call__(self, partition_list: Sequence[str], patient_list: Sequence[str]) -> List[int]:
        assert len(partition_list) == len(patient_list), (len(partition_list), len(patient_list))
        keys = [""] * len(partition_list)
        if self._contrastive_on_patient:
            keys = [k + "_" + str(p) for k, p in zip(keys, patient_list)]
        if self._contrastive_on_partition:
            keys = [k + "_" + str(p) for k, p in zip(keys, partition_list)]
        rank = {k: i for i, k in enumerate(sorted(set(keys)))}
        return [rank[k] for k in keys]


def unfold_position(features, partition_num=(4, 4)):
    """ref contrastyou/epocher/_utils.py:36-49: cut [b, c, h, w] into its ``partition_num`` grid of (h // ph) x (w // pw) blocks,
    concatenated along the batch in row-major block order -> ([ph * pw * b, c, h // ph, w // pw], the (row, column) pixel offset of
    each row's block).  The pool kernel writes this layout directly
    (``LocalProjectionHead.embeddings``); the function is the reference's export and the composition's."""
    import torch
    b, _c, h, w = features.shape
    block_h, block_w = h // partition_num[0], w // partition_num[1]
    blocks, flags = [], []
    for top in range(0, h - block_h + 1, block_h):
        for left in range(0, w - block_w + 1, block_w):
            blocks.append(features[:, :, top:top + block_h, left:left + block_w])
            flags.extend([(top, left)] * b)
    return torch.cat(blocks, dim=0), flags


class LocalLabelGenerator(GlobalLabelGenerator):
    """Contrastive class ids of the unfolded blocks (ref contrastyou/epocher/_utils.py:72-86): ``location_list`` holds one entry per
    unfolded row (``unfold_position``'s second result), the batch's partitions and patients repeat under it; two rows share an id
    when patient, partition and block position all agree.  The id is the rank of ``"_" + location + "_" + patient + "_" + partition``
    among the sorted unique strings."""

    def __init__(self) -> None:
        super().__init__(True, True)

    def __call__(self, partition_list: Sequence[str], patient_list: Sequence[str], location_list: Sequence) -> List[int]:
        partition_list, patient_list = [str(x) for x in partition_list], [str(x) for x in patient_list]
        location_list = [str(x) for x in location_list]
        repeat = len(location_list) // len(patient_list)
        partition_list, patient_list = partition_list * repeat, patient_list * repeat
        assert len(location_list) == len(partition_list), (len(location_list), len(partition_list))
        return super().__call__([a + "_" + b for a, b in zip(patient_list, partition_list)], location_list)


# ---- prediction dumps of the InferenceEpocher (ref: contrastyou/epocher/_utils.py:88-118; skimage.io.imsave -> PIL)
def _write_single_png(mask, save_dir: str, filename: str):
    import os

    import numpy as np
    from PIL import Image
    assert len(mask.shape) == 2, mask.shape
    os.makedirs(save_dir, exist_ok=True)
    Image.fromarray(mask.detach().cpu().numpy().astype(np.uint8)).save(os.path.join(save_dir, filename + ".png"))


def write_predict(predict_logit, save_dir: str, filenames):
    import os
    assert len(predict_logit.shape) == 4, predict_logit.shape
    filenames = [filenames] if isinstance(filenames, str) else filenames
    assert len(filenames) == len(predict_logit)
    for m, f in zip(predict_logit.max(1)[1], filenames):
        _write_single_png(m, os.path.join(save_dir, "pred"), f)


def write_prediction_map(pred, save_dir: str, filenames, folder: str):
    """Class-coded maps [N, H, W] (a prediction after post-processing) as PNGs under ``save_dir/folder``, named like ``pred/``'s."""
    import os
    assert len(pred.shape) == 3, pred.shape
    filenames = [filenames] if isinstance(filenames, str) else filenames
    assert len(filenames) == len(pred)
    for m, f in zip(pred.detach().cpu(), filenames):
        _write_single_png(m, os.path.join(save_dir, folder), f)


def write_img_target(image, target, save_dir: str, filenames):
    import os
    filenames = [filenames] if isinstance(filenames, str) else filenames
    image, target = image.squeeze(1), target.squeeze(1)
    assert image.shape == target.shape
    for img, f in zip(image, filenames):
        _write_single_png(img * 255, os.path.join(save_dir, "img"), f)
    for targ, f in zip(target, filenames):
        _write_single_png(targ, os.path.join(save_dir, "gt"), f)
