"""
Yardstick of the lesion segmentation, numpy + scipy on the host: label is scipy.ndimage.label with
the structure of the connectivity, segment adds the size filter and the raster renumbering, detection counts lesions
found, missed and invented by explicit loops over the regions.  Nothing here is shared with the code under test.
"""

import numpy as np
from scipy import ndimage

RANK = {6: 1, 18: 2, 26: 3}


def foreground(volume, threshold, keep=None):
    """vol > threshold in fp32 (NaN compares false), and keep != 0"""
    with np.errstate(invalid="ignore"):
        mask = np.asarray(volume, dtype=np.float32) > np.float32(threshold)
    return mask if keep is None else mask & (np.asarray(keep) != 0)


def label(mask, connectivity):
    """(labels int32, n): scipy numbers the components in raster order of their first voxel"""
    structure = ndimage.generate_binary_structure(3, RANK[connectivity])
    labels, n = ndimage.label(np.asarray(mask, dtype=bool), structure=structure)
    return labels.astype(np.int32), int(n)


def roots(labels):
    """the kernel's raw answer from a labelling: the flat index of each component's first voxel, -1 for background"""
    flat = labels.reshape(-1)
    first = np.full(int(flat.max()) + 1, flat.size, dtype=np.int64)
    at = np.nonzero(flat)[0]
    np.minimum.at(first, flat[at], at)
    first[0] = -1
    return first[flat].astype(np.int32).reshape(labels.shape)


def segment(volume, threshold, connectivity=26, min_voxels=1, keep=None):
    """(labels int32, n): components of fewer than min_voxels voxels are 0, the others 1..n in raster order"""
    labels, n = label(foreground(volume, threshold, keep), connectivity)
    sizes = np.bincount(labels.reshape(-1), minlength=n + 1)
    new = np.zeros(n + 1, dtype=np.int32)
    kept = 0
    for old in range(1, n + 1):                                    # ascending old numbers are raster order
        if sizes[old] >= min_voxels:
            kept += 1
            new[old] = kept
    return new[labels], kept


def detection(target_labels, estimate_labels):
    t, e = np.asarray(target_labels), np.asarray(estimate_labels)
    n_target, n_estimate = int(t.max()), int(e.max())
    found, overlap = [], []
    for r in range(1, n_target + 1):
        hits = int(np.count_nonzero(e[t == r]))
        overlap.append(hits)
        found.append(hits > 0)
    false_positives = 0
    for c in range(1, n_estimate + 1):
        if not np.any(t[e == c]):
            false_positives += 1
    n_found = sum(found)
    return {"n_target": n_target, "n_estimate": n_estimate, "found": found, "overlap": overlap, "n_found": n_found,
            "n_missed": n_target - n_found, "false_positives": false_positives,
            "sensitivity": n_found / n_target if n_target else None}


def random_mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def serpentine(shape):
    """One voxel-wide chain through the whole volume: in every even plane the full lines of the even rows, joined at
    alternating ends by one voxel on the odd row between them; consecutive even planes joined by one voxel on the odd
    plane between them, alternately at the path's end and at its start, so that the planes are walked back and forth.
    One component at every connectivity."""
    D, H, W = shape
    plane = np.zeros((H, W), dtype=bool)
    rows = list(range(0, H, 2))
    for i, y in enumerate(rows):
        plane[y, :] = True
        if i + 1 < len(rows):
            plane[y + 1, 0 if i % 2 else W - 1] = True
    start = (0, 0)
    end = (rows[-1], (W - 1 if len(rows) % 2 else 0) if W > 1 else 0)
    m = np.zeros(shape, dtype=bool)
    for k, z in enumerate(range(0, D, 2)):
        m[z] = plane
        if z + 2 < D:
            y, x = start if k % 2 else end
            m[z + 1, y, x] = True
    return m


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return (z + y + x) % 2 == 0


def blobs_pair(shape=(20, 24, 40)):
    """(target, estimate) float32: 5 hot blobs in the target; in the estimate the first is absent, the second shifted
    but overlapping, the third split in two, the other two as they are, and two extra blobs"""
    t = np.zeros(shape, dtype=np.float32)
    e = np.zeros(shape, dtype=np.float32)
    t[2:5, 2:5, 2:5] = 3.0                                         # 1: absent
    t[2:6, 10:14, 2:6] = 3.0                                       # 2: shifted by 2 along every axis
    e[4:8, 12:16, 4:8] = 3.0
    t[2:5, 18:22, 10:20] = 3.0                                     # 3: split in two along W
    e[2:5, 18:22, 10:14] = 3.0
    e[2:5, 18:22, 16:20] = 3.0
    t[10:14, 2:6, 20:26] = 3.0                                     # 4, 5: kept
    e[10:14, 2:6, 20:26] = 3.0
    t[12:17, 12:18, 30:36] = 3.0
    e[12:17, 12:18, 30:36] = 3.0
    e[16:19, 2:5, 2:6] = 3.0                                       # two hot spots the target has not
    e[17:19, 20:23, 12:15] = 3.0
    return t, e
