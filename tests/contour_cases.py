"""Masks whose number of border segments ("heads", csrc/vp_contours.inl) is chosen, for the tests that put the contour pass on the two
sides of every head count at which it changes form (tests/test_contour_cases.py on the CPU, tests/test_gpu_contour_capacity.py).

`head_count` restates the count from the definition in the header comment of vp_contours.inl, pixel by pixel:
  * a crack is an edge between a foreground pixel and a 4-adjacent background pixel (outside the image is background);
  * the state that sweeps a crack is (pixel, s), s = the first foreground neighbour clockwise from the crack's direction;
  * eligible cracks: N / S cracks in columns x % 4 == 0 (x % 8 in the sparse cut), W / E cracks in rows y % 2 == 0 (y % 4), every W
    crack of a pixel with nothing in the three pixels above it, every E crack whose background pixel has foreground above it;
  * a head is a state that sweeps at least one eligible crack (it counts once however many it sweeps), and a pixel without neighbours
    is one head.
Nothing here looks at the bit formulas of k_ct_headmaps.

Two families of masks with exactly H heads in the dense cut:
  snake(H)  one serpentine wall, one pixel wide, whose single outer border carries all but a few of the heads (one long cycle for the
            pointer jumping), and lone pixels for the rest;
  nests(H)  a frame-wide ring with cells of three concentric rings side by side in its hole (RETR_EXTERNAL: every component in the hole
            has the answer of the one to its left - chains as long as a row of cells; the hierarchy is seven levels deep), more cells
            below the ring at the top level, and lone pixels for the rest.
A lone pixel adds exactly one head as long as it has no 8-neighbour: every term of the count looks at a pixel's 3x3 neighbourhood only.
"""
import functools

import numpy as np

# directions counter-clockwise as displayed (y down): E, NE, N, NW, W, SW, S, SE
_DY = (0, -1, -1, -1, 0, 1, 1, 1)
_DX = (1, 1, 0, -1, -1, -1, 0, 1)
E, NE, N, NW, W, SW, S, SE = range(8)

BOUNDARIES = (1024, 2048, 3072, 4096, 6144, 8192)       # the last head count of ctj_body_lds<1|2|3|4|6|8> (k_ct_jump)
ITEMS = (1, 2, 3, 4, 6, 8)
LDS_HEADS = 8192                                        # CTJ_LDS_HEADS
SHAPE, SHAPE_ODD = (128, 256), (128, 250)               # 250: the last word of a row is partial
FAMILIES = ("snake", "nests")


def heads(mask, sparse=False):
    """The heads of the mask as a set of (y, x, s); s = -1 for a pixel without neighbours."""
    h, w = mask.shape
    f = np.zeros((h + 2, w + 2), bool)
    f[1:-1, 1:-1] = mask != 0
    f = f.tolist()
    rows, cols = (4, 8) if sparse else (2, 4)
    out = set()
    ys, xs = np.nonzero(mask)
    for y, x in zip(ys.tolist(), xs.tolist()):
        nb = [f[y + 1 + _DY[d]][x + 1 + _DX[d]] for d in range(8)]
        if not any(nb):
            out.add((y, x, -1))
            continue
        for d in (W, E, N, S):
            if nb[d]:
                continue                                  # no crack on this side
            if d == W:
                eligible = y % rows == 0 or not (nb[NW] or nb[N] or nb[NE])
            elif d == E:
                eligible = y % rows == 0 or nb[NE]        # (y - 1, x + 1) lies above the crack's background pixel (y, x + 1)
            else:
                eligible = x % cols == 0
            if not eligible:
                continue
            s = d
            while not nb[s]:                              # clockwise = towards smaller direction numbers
                s = (s - 1) % 8
            out.add((y, x, s))                            # (a set: a state that sweeps several eligible cracks is one head)
    return out


def head_count(mask, sparse=False):
    return len(heads(mask, sparse))


def word_heads(mask, sparse=False):
    """(h, ceil(w / 64)) heads per 64-pixel word of a row - what k_ct_headmaps keeps in one byte"""
    h, w = mask.shape
    out = np.zeros((h, (w + 63) // 64), np.int64)
    for y, x, _ in heads(mask, sparse):
        out[y, x // 64] += 1
    return out


def densest_word(w=192):
    """Five rows of a checkerboard; word 1 of row 2 (an even row, away from the frame) is believed - and here shown - to hold the most
    heads a word can.
    A head owns an eligible crack of its own, so a word holds at most as many heads as eligible cracks.  Its W and E cracks number two
    per run of foreground pixels in the row: at most 64 with 32 runs of one pixel.  Its N and S cracks are eligible in 16 columns only:
    at most 32.  96 in all - and the checkerboard reaches it: every pixel of the even row has four background 4-neighbours and four
    foreground diagonal ones, so each crack has a state of its own; the 16 pixels at x % 4 == 0 are four heads each, the 16 at
    x % 4 == 2 two (W and E)."""
    yy, xx = np.mgrid[0:5, 0:w]
    return np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)      # (rows 0, 2 and 4 hold the pixels at even x)


DENSEST_WORD_HEADS = 96


def _free(mask, y, x):
    h, w = mask.shape
    return not mask[max(y - 1, 0):min(y + 2, h), max(x - 1, 0):min(x + 2, w)].any()


def _top_up(mask, H, slots, what):
    """lone pixels at the first free slots until the mask has H heads; the slots are two apart in both directions"""
    c = head_count(mask)
    need = H - c
    if need < 0:
        raise ValueError(f"{what}: the structure alone has {c} heads, {H} wanted")
    for y, x in slots:
        if need == 0:
            break
        if _free(mask, y, x):
            mask[y, x] = 255
            need -= 1
    if need:
        raise ValueError(f"{what}: no room for {need} more lone pixels")
    got = head_count(mask)
    assert got == H, (what, got, H)
    mask.setflags(write=False)
    return mask


def snake_path(shape):
    """the wall as an ordered pixel list: down column 0, one step right along the last row, up column 2, right along row 0, ..."""
    h, w = shape
    path = []
    for i, x in enumerate(range(0, w, 2)):
        rows = range(h) if i % 2 == 0 else range(h - 1, -1, -1)
        path += [(y, x) for y in rows]
        if x + 2 < w:
            path.append((h - 1 if i % 2 == 0 else 0, x + 1))
    return path


@functools.lru_cache(maxsize=None)
def snake(H, shape=SHAPE):
    h, w = shape
    path = snake_path(shape)
    keep = 16                                             # lone pixels wanted at least: both kinds of head in every mask
    n = max(1, min(len(path), H - keep))

    def wall(n):
        m = np.zeros(shape, np.uint8)
        ys, xs = zip(*path[:n])
        m[list(ys), list(xs)] = 255
        return m
    for _ in range(8):                                    # about one head per wall pixel: a few corrections settle the length
        m = wall(n)
        c = head_count(m)
        if c <= H - keep or n == 1:
            break
        n = max(1, n - (c - (H - keep)))
    x_end = max(x for _, x in path[:n])
    slots = [(y, x) for x in range(x_end + 3, w, 2) for y in range(1, h, 2)]
    return _top_up(m, H, slots, f"snake({H}, {shape})")


CELL = 11                                                 # three concentric one-pixel rings: sides 11, 7 and 3
PITCH = CELL + 1


def _cell():
    c = np.zeros((CELL, CELL), np.uint8)
    for k in (0, 2, 4):
        c[k:CELL - k, k:CELL - k] = 255
        c[k + 1:CELL - k - 1, k + 1:CELL - k - 1] = 0
    return c


CELL_CONTOURS = 6                                         # an outer and a hole border per ring


def nest_slots(shape):
    """(ring height R, cell origins): cells in the hole of the ring (rows 0 .. R - 1, the whole width) and below it, two in the hole
    for every one below"""
    h, w = shape
    R = h - 3 * PITCH - 4 if h >= 100 else h - PITCH - 2
    xs = list(range(2, w - 2 - CELL, PITCH))
    inside = [(y, x) for y in range(2, R - 2 - CELL, PITCH) for x in xs]
    below = [(y, x) for y in range(R + 1, h - CELL + 1, PITCH) for x in xs]
    order = []
    while inside or below:
        order += inside[:2] + below[:1]
        inside, below = inside[2:], below[1:]
    return R, order


def _nest_base(shape):
    R, order = nest_slots(shape)
    m = np.zeros(shape, np.uint8)
    m[0:R, :] = 255
    m[1:R - 1, 1:shape[1] - 1] = 0
    return m, order


def _lone_slots(order, used):
    return [(y + 1 + 2 * a, x + 1 + 2 * b) for y, x in reversed(order[used:]) for a in range(5) for b in range(5)]


@functools.lru_cache(maxsize=None)
def nests(H, shape=SHAPE):
    m, order = _nest_base(shape)
    cell = _cell()
    keep = 4
    total = head_count(m)
    used = 0
    for y, x in order:                                    # (components that do not touch add their heads up)
        one = np.zeros(shape, np.uint8)
        one[y:y + CELL, x:x + CELL] = cell
        c = head_count(one)
        if total + c > H - keep:
            break
        m[y:y + CELL, x:x + CELL] = cell
        total += c
        used += 1
    return _top_up(m, H, _lone_slots(order, used), f"nests({H}, {shape})")


@functools.lru_cache(maxsize=None)
def nests_contours(N, shape=(64, 250)):
    """the same layout with exactly N borders (RETR_LIST / RETR_CCOMP / RETR_TREE): 2 for the ring, 6 per cell, lone pixels for the rest"""
    m, order = _nest_base(shape)
    cell = _cell()
    used = min((N - 2 - 3) // CELL_CONTOURS, len(order) - 1)
    if used < 3:
        raise ValueError(f"nests_contours({N}): too few borders for a nest")
    for y, x in order[:used]:
        m[y:y + CELL, x:x + CELL] = cell
    need = N - 2 - CELL_CONTOURS * used
    for y, x in _lone_slots(order, used)[:need]:
        assert _free(m, y, x)
        m[y, x] = 255
    m.setflags(write=False)
    return m


def shape_for(b):
    return SHAPE_ODD if b in (3072, 8192) else SHAPE


def boundary_cases():
    """(name, family, H, mask builder arguments) on the two sides of every boundary, both families"""
    out = []
    for b in BOUNDARIES:
        for H in (b, b + 1):
            for fam in FAMILIES:
                out.append((f"{fam}-{H}", fam, H, shape_for(b)))
    return out


def build(fam, H, shape):
    return {"snake": snake, "nests": nests}[fam](H, shape)


def tiled_4x4(rng, h=96, w=200):
    """random 4x4 patterns edge to edge"""
    t = rng.integers(0, 1 << 16, size=((h + 3) // 4, (w + 3) // 4), dtype=np.uint32)
    m = np.zeros((t.shape[0] * 4, t.shape[1] * 4), np.uint8)
    for b in range(16):
        m[b // 4::4, b % 4::4] = ((t >> b) & 1).astype(np.uint8) * 255
    return np.ascontiguousarray(m[:h, :w])
