"""Batch unpackers used by the epochers (ref: contrastyou/epocher/_utils.py:25-33) and the contrastive label generator (ref :52-69)."""
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


def write_img_target(image, target, save_dir: str, filenames):
    import os
    filenames = [filenames] if isinstance(filenames, str) else filenames
    image, target = image.squeeze(1), target.squeeze(1)
    assert image.shape == target.shape
    for img, f in zip(image, filenames):
        _write_single_png(img * 255, os.path.join(save_dir, "img"), f)
    for targ, f in zip(target, filenames):
        _write_single_png(targ, os.path.join(save_dir, "gt"), f)
