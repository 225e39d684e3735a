"""The numpy reference of Cropper(subject="largest", fill_holes=N), every face on its own,
H and W the crop's size:

    m0(y,x) = 1 where labels(y,x) < 19 and bit labels(y,x) of class_bits is set, else 0
    subject="largest": the 8-connected components of {m0 = 1}; a component's key is (its pixel count, then the SMALLER
        raster index y*W + x of its first pixel in raster order); m1 = the component with the largest count, among equal
        counts the one whose first pixel comes first; no foreground pixel: m1 = m0.  Otherwise m1 = m0.
    fill_holes=N: the 4-connected components of {m1 = 0}; a hole is one that has no pixel in row 0, row H-1, column 0 or
        column W-1; m2 = m1, plus every hole of at most N pixels.  Otherwise m2 = m1.
    out(y,x) = m2(y,x), one byte, 0 or 1

``components_slow`` is a plain union-find over pixels in Python ints; ``components`` is the form the GPU tests use: the
runs of every row from numpy, a union-find over the runs of adjacent rows.  Both give every pixel of the set the smallest
raster index of its component (-1 outside), which is all the definition needs.  No scipy here."""
import numpy as np

NUM_CLASSES = 19
DEFAULT_BITS = sum(1 << c for c in range(1, NUM_CLASSES))
ONE_17 = (1 << 1) | (1 << 17)
SUBJECT_BITS = 1 << 1
TILE_W, TILE_H = 64, 32                     # kTileW, kTileH of csrc/fcp_subject.hip


def mask0(labels, bits):
    """labels (..., H, W) uint8 -> m0 as bool."""
    lut = np.array([c < NUM_CLASSES and bool(bits >> c & 1) for c in range(256)], bool)
    return lut[np.asarray(labels, np.uint8)]


def _find(parent, x):
    while parent[x] != x:
        x = parent[x]
    return x


def _union(parent, a, b):
    a, b = _find(parent, a), _find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)


def components_slow(s, conn):
    """s (H,W) bool -> (H,W) int64: the smallest raster index of the pixel's ``conn``-connected component, -1 outside s.
    A union-find over the pixels, in Python ints."""
    h, w = s.shape
    parent = list(range(h * w))
    near = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if conn == 8 else [])
    for y in range(h):
        for x in range(w):
            if s[y, x]:
                for dy, dx in near:
                    v, u = y + dy, x + dx
                    if 0 <= v and 0 <= u < w and s[v, u]:
                        _union(parent, y * w + x, v * w + u)
    out = np.full((h, w), -1, np.int64)
    for y in range(h):
        for x in range(w):
            if s[y, x]:
                out[y, x] = _find(parent, y * w + x)
    return out


def components(s, conn):
    """The same from the runs of the rows: run k of row y covers columns start[k] .. end[k] - 1; runs of adjacent rows
    touch where their column ranges overlap (4) or come within one column (8)."""
    h, w = s.shape
    d = np.diff(np.concatenate([np.zeros((h, 1), np.int8), s.astype(np.int8), np.zeros((h, 1), np.int8)], axis=1), axis=1)
    ys, starts = np.nonzero(d == 1)                                   # in raster order: a run's id grows with its first pixel
    ends = np.nonzero(d == -1)[1]
    first = np.searchsorted(ys, np.arange(h + 1))                     # the runs of row y are first[y] .. first[y + 1] - 1
    parent = list(range(len(ys)))
    e = 1 if conn == 8 else 0
    st, en = starts.tolist(), ends.tolist()
    for y in range(1, h):
        a, a_end, b, b_end = first[y - 1], first[y], first[y], first[y + 1]
        while a < a_end and b < b_end:
            if st[a] < en[b] + e and st[b] < en[a] + e:
                _union(parent, a, b)
            if en[a] < en[b]:
                a += 1
            else:
                b += 1
    root = np.array([_find(parent, k) for k in range(len(ys))], np.int64)
    out = np.full(h * w, -1, np.int64)
    if len(ys):
        index = (ys * w + starts)[root]
        length = ends - starts
        at = np.repeat(ys * w + starts - np.concatenate([[0], np.cumsum(length)[:-1]]), length) + np.arange(length.sum())
        out[at] = np.repeat(index, length)
    return out.reshape(h, w)


def largest(m, comp=components):
    """m (H,W) bool -> its largest 8-connected component (first pixel first among equals); m itself where it is empty."""
    if not m.any():
        return m.copy()
    c = comp(m, 8)
    area = np.bincount(c[c >= 0], minlength=m.size)
    return c == int(np.argmax(area))                                  # the first maximum: the smaller raster index


def filled(m, n, comp=components):
    """m (H,W) bool -> m plus every 4-connected region of its complement of at most n pixels that has no border pixel."""
    c = comp(~m, 4)
    area = np.bincount(c[c >= 0], minlength=m.size)
    edge = np.concatenate([c[0], c[-1], c[:, 0], c[:, -1]])
    open_ = np.zeros(m.size + 1, bool)
    open_[edge[edge >= 0]] = True
    fill = (c >= 0) & ~open_[c] & (area[c] <= n)                       # c == -1 indexes the spare last entry
    return m | fill


def subject_mask(labels, bits, keep_largest, max_hole, comp=components):
    """labels (F,H,W) uint8 -> out (F,H,W) uint8 of 0 / 1."""
    labels = np.asarray(labels, np.uint8)
    out = np.zeros(labels.shape, np.uint8)
    for k, m in enumerate(mask0(labels, bits)):
        if keep_largest:
            m = largest(m, comp)
        if max_hole:
            m = filled(m, int(max_hole), comp)
        out[k] = m
    return out


def connected(m, conn=8, comp=components):
    """Whether the set pixels of m are one component (or none)."""
    c = comp(m, conn)
    return len(np.unique(c[c >= 0])) <= 1


# ---- patterns: (rng, h, w) -> (h, w) uint8 labels, class 1 on class 0 unless said otherwise
def _random(density):
    def make(rng, h, w):
        return (rng.random((h, w)) < density).astype(np.uint8)
    return make


def _checker(rng, h, w):
    return ((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0).astype(np.uint8)


def _serpentine(rng, h, w):
    """Full even rows joined at alternating ends: one component whose only path is about h w / 2 long."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for y in range(1, h, 2):
        m[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def _serpentine_t(rng, h, w):
    return np.ascontiguousarray(_serpentine(rng, w, h).T)


def _spiral(rng, h, w):
    """Rectangles at insets 0, 2, 4, ..., each cut open below its top left corner and bridged to the next one."""
    m = np.zeros((h, w), np.uint8)
    for k in range(0, (min(h, w) + 1) // 2, 2):
        m[k, k:w - k] = m[h - 1 - k, k:w - k] = 1
        m[k:h - k, k] = m[k:h - k, w - 1 - k] = 1
        if k + 2 < h - 1 - k and k + 2 < w - 1 - k:
            m[k + 1, k] = 0
            m[k + 1, k + 2] = 1
    return m


def _full(rng, h, w):
    return np.ones((h, w), np.uint8)


def _empty(rng, h, w):
    return np.zeros((h, w), np.uint8)


def _corners(rng, h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    return m


def _put(m, pixels):
    for y, x in pixels:
        if 0 <= y < m.shape[0] and 0 <= x < m.shape[1]:
            m[y, x] = 1
    return m


def _tie(rng, h, w):
    """Two components of equal count: A starts at (0, w - 1), B at (1, 0), whose bounding box comes first row-major by
    its column; A's first pixel comes first in raster order and survives."""
    return _put(np.zeros((h, w), np.uint8), [(0, w - 1), (1, w - 1), (1, 0), (2, 0)])


def _diag(main):
    def make(rng, h, w):
        """A component of 4 pixels joined only by a diagonal through the corner of four tiles, and a rival of 3."""
        m = np.zeros((h, w), np.uint8)
        if main:
            _put(m, [(TILE_H - 2, TILE_W - 1), (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W)])
        else:
            _put(m, [(TILE_H - 2, TILE_W), (TILE_H - 1, TILE_W), (TILE_H, TILE_W - 1), (TILE_H + 1, TILE_W - 1)])
        return _put(m, [(0, 0), (0, 1), (0, 2)])
    return make


def _rings(step):
    def make(rng, h, w):
        """Rectangles one pixel thick at insets 1, 1 + step, ...: holes, and islands inside holes."""
        m = np.zeros((h, w), np.uint8)
        for k in range(1, (min(h, w) + 1) // 2, step):
            m[k, k:w - k] = m[h - 1 - k, k:w - k] = 1
            m[k:h - k, k] = m[k:h - k, w - 1 - k] = 1
        return m
    return make


def _classes(rng, h, w):
    return rng.integers(0, NUM_CLASSES, (h, w)).astype(np.uint8)


PATTERNS = {
    "random41": _random(0.41), "random50": _random(0.5), "checker": _checker, "serpentine": _serpentine,
    "serpentine_t": _serpentine_t, "spiral": _spiral, "full": _full, "empty": _empty, "corners": _corners, "tie": _tie,
    "diag_main": _diag(True), "diag_anti": _diag(False), "ring": _rings(1 << 20), "nested": _rings(2), "classes": _classes,
}
# three faces a call, a different pattern in each
GROUPS = [("random41", "checker", "serpentine"), ("random50", "serpentine_t", "spiral"), ("full", "empty", "corners"),
          ("tie", "diag_main", "diag_anti"), ("ring", "nested", "classes")]


def labels_of(group, rng, h, w):
    return np.stack([PATTERNS[p](rng, h, w) for p in group])
