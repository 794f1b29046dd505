"""CPU oracle of the synthetic paired loader -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_synth_data.py).

A PIL + torch-CPU restatement of MyDatasetSynthetic.transform (scripts/utils.py:483-553) with the random draws
(flip, i, j) as inputs, built on the helpers of oracle/data_oracle.py.  The image chain is that module's transform_image;
the mask / label chain is written out literally: resize(..., NEAREST) to the resized image_b's size, crop, to_tensor * 255,
mapping, the maximum rule and the two threshold assignments.

As in oracle/data_oracle.py, torchvision is not installed: Resize / crop / ToTensor are restated from their documented
behaviour and the pixel arithmetic is Pillow's own, which the HIP kernels are checked against bit for bit.  `mapping` is
restated from its table; tests/golden/golden_synth_data.json holds what the reference's own function returns for all 256
grey values, and tests/test_cpu_synth_data.py pins this restatement on it."""
import numpy as np

from oracle.data_oracle import _FLIP, _NEAREST, resized_hw, to_tensor, transform_image

_LABELS = ((255, 8), (200, 7), (178, 6), (149, 5), (133, 4), (76, 3), (55, 2), (29, 1), (0, 0))


def mapping(im):
    """utils.py:1356-1366: in place, equality on the float values."""
    for grey, cls in _LABELS:
        im[im == grey] = cls
    return im


def transform_plane(plane, flip, size_wh, crop):
    """The part of the chain the mask and the label maps share: flip, NEAREST resize to the resized image's (w, h), crop."""
    i, j, h, w = crop
    if flip:
        plane = plane.transpose(_FLIP)
    plane = plane.resize(size_wh, _NEAREST)
    return plane.crop((j, i, j + w, i + h))


def transform_mask(mask, flip, size_wh, crop):
    mask = transform_plane(mask, flip, size_wh, crop)
    if np.max(mask) == 1:
        mask = to_tensor(mask) * 255
    else:
        mask = to_tensor(mask)
    mask[mask > 0.5] = 1
    mask[mask < 0.5] = 0
    return mask


def transform_label(sem, flip, size_wh, crop):
    sem = transform_plane(sem, flip, size_wh, crop)
    return mapping(to_tensor(sem) * 255)


def transform_synthetic(image_a, image_b, mask, semantic_a, semantic_b, flip, new_size, crop):
    """PIL inputs (RGB, RGB, L, L, L); crop = (i, j, h, w) inside the resized image_b.  Returns the five tensors of
    MyDatasetSynthetic.transform: (3,h,w), (3,h,w), (1,h,w), (1,h,w), (1,h,w) float32."""
    rs_h, rs_w = resized_hw(image_b.size[0], image_b.size[1], new_size)
    return (transform_image(image_a, flip, new_size, crop), transform_image(image_b, flip, new_size, crop),
            transform_mask(mask, flip, (rs_w, rs_h), crop), transform_label(semantic_a, flip, (rs_w, rs_h), crop),
            transform_label(semantic_b, flip, (rs_w, rs_h), crop))
