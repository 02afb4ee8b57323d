"""The speckle filter, restated: the contract of vp_filter_speckles_* (DESIGN.md section 4.35).  A plain serial flood fill, no cleverness.

  * Pixels equal to new_val belong to no region and stay as they are.
  * Two other pixels are linked if they are 4-neighbours and |d[p] - d[q]| <= max_diff, the difference taken in int32.
  * A region is a connected component of that graph: links chain (each flood step compares with the pixel just popped, not with the
    seed), so a ramp 0, 1, 2, 3, ... with max_diff = 1 is one region.  The components of a graph do not depend on the visiting order.
  * Every region with at most max_speckle_size pixels is overwritten with new_val; everything else is copied unchanged.

This is the rule of cv2.filterSpeckles for int16 images.  It has not met a real OpenCV (tests/test_live_cv2_speckle.py does that where
one is installed)."""
import numpy as np


def regions(d, new_val, max_diff):
    """int32 (h, w): 0 for pixels of no region, else the region's number 1, 2, ... in raster order of first pixels; and the sizes"""
    d = np.asarray(d)
    assert d.dtype == np.int16 and d.ndim == 2
    h, w = d.shape
    v = d.astype(np.int32)
    lab = np.zeros((h, w), np.int32)
    sizes = [0]
    for sy in range(h):
        for sx in range(w):
            if lab[sy, sx] or v[sy, sx] == new_val:
                continue
            n = len(sizes)
            lab[sy, sx] = n
            stack, count = [(sy, sx)], 0
            while stack:
                y, x = stack.pop()
                count += 1
                for qy, qx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= qy < h and 0 <= qx < w and not lab[qy, qx] and v[qy, qx] != new_val and abs(int(v[qy, qx]) - int(v[y, x])) <= max_diff:
                        lab[qy, qx] = n
                        stack.append((qy, qx))
            sizes.append(count)
    return lab, np.array(sizes, np.int64)


def filter_speckles(d, new_val, max_speckle_size, max_diff):
    """a new int16 image"""
    lab, sizes = regions(d, new_val, max_diff)
    out = np.array(d, np.int16, copy=True)
    small = sizes <= max_speckle_size
    small[0] = False
    out[small[lab]] = new_val
    return out
