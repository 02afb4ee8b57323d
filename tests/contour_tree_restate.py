"""Two independent statements of cv2.findContours' RETR_CCOMP / RETR_TREE structure (OpenCV 4.x, offset 0), in numpy / scipy.

Both return the borders in the order cv2 returns them, as `(starts, holes, hierarchy)`: starts (N, 2) int (y, x) start pixels,
holes (N,) uint8 hole flags, hierarchy (N, 4) int32 rows [next, prev, first_child, parent] (-1 for none).  The points of each
border are the RETR_LIST border with the same start (oracle.find_contours); `expected` maps one onto the other.

(a) `raster_scan`: Suzuki-Abe's raster scan literally - the marks NBD / -NBD left by the tracer, LNBD, the parent table, a front
    insertion into the parent's child list (cvInsertNodeIntoTree in icvEndProcessContour), the tree flattened in pre-order
    (cvTreeToNodeSeq).
(b) `topological`: 8-connected foreground components and 4-connected background regions of the zero-padded mask
    (scipy.ndimage.label); an outer border per component, starting at its first pixel; a hole border per region that does not
    reach the frame, starting at the pixel left of its first pixel.  Parent of an outer border: the hole border of the region
    left of its first pixel (none if that region is the frame's); parent of a hole border: the outer border of the component
    left of the region's first pixel.  Order: pre-order, top level first, siblings by decreasing start (newest first).
"""
import numpy as np

RETR_CCOMP, RETR_TREE = 2, 3

# directions counter-clockwise as displayed (y down): E, NE, N, NW, W, SW, S, SE
_DY = (0, -1, -1, -1, 0, 1, 1, 1)
_DX = (1, 1, 0, -1, -1, -1, 0, 1)


def _dir(dy, dx):
    for d in range(8):
        if _DY[d] == dy and _DX[d] == dx:
            return d
    raise ValueError((dy, dx))


def _flatten(n, children):
    """pre-order of the forest (children[-1] = the top level; lists already newest first) -> (order, hierarchy in that order)"""
    order = []
    stack = list(reversed(children[-1]))
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(reversed(children[v]))
    pos = {v: i for i, v in enumerate(order)}
    hier = np.full((n, 4), -1, np.int32)
    for p, ch in children.items():
        for k, v in enumerate(ch):
            row = hier[pos[v]]
            row[0] = pos[ch[k + 1]] if k + 1 < len(ch) else -1
            row[1] = pos[ch[k - 1]] if k > 0 else -1
            row[3] = pos[p] if p >= 0 else -1
        if p >= 0 and ch:
            hier[pos[p], 2] = pos[ch[0]]
    return order, hier


def raster_scan(mask, mode):
    """(a) Suzuki-Abe's raster scan with the LNBD parent rule."""
    if mode not in (RETR_CCOMP, RETR_TREE):
        raise ValueError("mode")
    h, w = mask.shape
    f = np.zeros((h + 2, w + 2), np.int64)
    f[1:-1, 1:-1] = mask != 0
    f = f.tolist()
    # border 1 = the frame, a hole border; borders 2.. in discovery order
    is_hole = {1: True}
    parent = {1: None}
    start = {}
    nbd = 1
    for i in range(1, h + 1):
        lnbd = 1
        row = f[i]
        for j in range(1, w + 1):
            v = row[j]
            if v == 0:
                continue
            if v == 1 and row[j - 1] == 0:
                hole, d2 = False, 4                       # outer border, (i2, j2) = (i, j - 1)
            elif v >= 1 and row[j + 1] == 0:
                hole, d2 = True, 0                        # hole border, (i2, j2) = (i, j + 1)
                if v > 1:
                    lnbd = v
            else:
                if v != 1:
                    lnbd = abs(v)
                continue
            nbd += 1
            b = lnbd
            if hole:
                parent[nbd] = b if not is_hole[b] else parent[b]
            else:
                parent[nbd] = b if is_hole[b] else parent[b]
            is_hole[nbd] = hole
            start[nbd] = (i - 1, j - 1)
            # (3.1) clockwise from (i2, j2) for a nonzero pixel
            d1 = None
            for k in range(8):
                d = (d2 - k) % 8
                if f[i + _DY[d]][j + _DX[d]] != 0:
                    d1 = d
                    break
            if d1 is None:
                row[j] = -nbd
            else:
                i1, j1 = i + _DY[d1], j + _DX[d1]
                i2, j2 = i1, j1
                i3, j3 = i, j
                while True:
                    # (3.3) counter-clockwise from the element after (i2, j2)
                    d = _dir(i2 - i3, j2 - j3)
                    east_zero = False
                    for _ in range(8):
                        d = (d + 1) % 8
                        if f[i3 + _DY[d]][j3 + _DX[d]] != 0:
                            break
                        if d == 0:
                            east_zero = True
                    i4, j4 = i3 + _DY[d], j3 + _DX[d]
                    # (3.4)
                    if east_zero:
                        f[i3][j3] = -nbd
                    elif f[i3][j3] == 1:
                        f[i3][j3] = nbd
                    # (3.5)
                    if (i4, j4) == (i, j) and (i3, j3) == (i1, j1):
                        break
                    i2, j2, i3, j3 = i3, j3, i4, j4
            # (4)
            if row[j] != 1:
                lnbd = abs(row[j])
    n = nbd - 1
    children = {k: [] for k in range(-1, n)}
    for b in range(2, nbd + 1):                           # discovery order; each new border goes to the front of its parent's list
        p = parent[b]
        if mode == RETR_CCOMP and not is_hole[b]:
            p = 1
        children[-1 if p == 1 else p - 2].insert(0, b - 2)
    order, hier = _flatten(n, children)
    starts = np.array([start[v + 2] for v in order], np.int64).reshape(-1, 2)
    holes = np.array([1 if is_hole[v + 2] else 0 for v in order], np.uint8)
    return starts, holes, hier


def topological(mask, mode):
    """(b) the tree from the components and regions of the padded mask (scipy.ndimage.label)."""
    from scipy import ndimage
    if mode not in (RETR_CCOMP, RETR_TREE):
        raise ValueError("mode")
    h, w = mask.shape
    fg = np.zeros((h + 2, w + 2), bool)
    fg[1:-1, 1:-1] = mask != 0
    comp, _ = ndimage.label(fg, structure=np.ones((3, 3), int))
    reg, _ = ndimage.label(~fg, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    frame_region = int(reg[0, 0])
    flat_c, flat_r = comp.ravel(), reg.ravel()

    def firsts(flat):                                     # label -> first pixel in raster order (of the padded image)
        idx = np.flatnonzero(flat)
        labs, at = np.unique(flat[idx], return_index=True)
        return dict(zip(labs.tolist(), idx[at].tolist()))
    borders = [(a, False, lab) for lab, a in firsts(flat_c).items()]
    borders += [(a - 1, True, lab) for lab, a in firsts(flat_r).items() if lab != frame_region]
    borders.sort()                                        # scan order of the start pixels
    outer_of = {lab: k for k, (a, hole, lab) in enumerate(borders) if not hole}
    hole_of = {lab: k for k, (a, hole, lab) in enumerate(borders) if hole}
    n = len(borders)
    parent = []
    for a, hole, lab in borders:
        if hole:
            parent.append(outer_of[int(flat_c[a])])        # the component left of the region's first pixel
        elif mode == RETR_CCOMP:
            parent.append(-1)
        else:
            r = int(flat_r[a - 1])                         # the region left of the component's first pixel
            parent.append(-1 if r == frame_region else hole_of[r])
    children = {k: [] for k in range(-1, n)}
    for k in range(n - 1, -1, -1):                        # newest (latest start) first
        children[parent[k]].append(k)
    order, hier = _flatten(n, children)
    W = w + 2
    starts = np.array([divmod(borders[k][0], W) for k in order], np.int64).reshape(-1, 2) - 1
    holes = np.array([1 if borders[k][1] else 0 for k in order], np.uint8)
    return starts, holes, hier


def expected(mask, mode, list_contours, statement=raster_scan):
    """(contours, holes, hierarchy) that cv2.findContours(mask, mode, method) returns, given the RETR_LIST contours of the same method
    (newest first = by decreasing start pixel)."""
    starts, holes, hier = statement(mask, mode)
    by_start = sorted(((int(y), int(x)) for y, x in starts), reverse=True)
    at = {s: k for k, s in enumerate(by_start)}
    assert len(at) == len(list_contours)
    return [list_contours[at[(int(y), int(x))]] for y, x in starts], holes, hier
