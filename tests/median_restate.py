"""Two independent statements of cv2.medianBlur on uint8 images, in numpy: the oracle of tests/test_gpu_median.py.

  median_restate(img, k)     the definition: per channel, the middle element (index k*k // 2 of the sorted window) of the k x k window over
                             the edge-padded image.  OpenCV's sorting networks (k = 3, 5), its O(1) histogram code and its 'Om' code
                             all compute exactly this over BORDER_REPLICATE; nothing is rounded and no tie rule exists.
  majority_restate(mask, k)  for 0/255 images: 255 where more than k*k // 2 window pixels are set, from a summed-area table."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def median_restate(img, k):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and k >= 1 and k % 2 == 1
    if img.ndim == 3:
        return np.stack([median_restate(np.ascontiguousarray(img[:, :, c]), k) for c in range(img.shape[2])], axis=2)
    r = k // 2
    win = sliding_window_view(np.pad(img, r, mode="edge"), (k, k)).reshape(img.shape[0], img.shape[1], k * k)
    return np.ascontiguousarray(np.partition(win, k * k // 2, axis=2)[:, :, k * k // 2])


def majority_restate(mask, k):
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2 and k >= 1 and k % 2 == 1
    r = k // 2
    sat = np.zeros((mask.shape[0] + k, mask.shape[1] + k), np.int64)
    sat[1:, 1:] = np.pad((mask != 0).astype(np.int64), r, mode="edge").cumsum(0).cumsum(1)
    cnt = sat[k:, k:] - sat[:-k, k:] - sat[k:, :-k] + sat[:-k, :-k]
    return np.where(cnt > k * k // 2, 255, 0).astype(np.uint8)
