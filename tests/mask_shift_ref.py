"""The numpy reference of Cropper(edge_shift=N), every face on its own, r = |shift|:

    m0(y,x) = (class_bits >> labels(y,x)) & 1
    only positions inside the crop exist: a pixel outside the crop is neither subject nor background, never a source
    shift > 0 (grow):   out(y,x) = 1 iff some (y',x') inside the crop has m0 = 1 and (y-y')^2 + (x-x')^2 <= r^2
    shift < 0 (shrink): out(y,x) = 1 iff m0(y,x) = 1 and no (y',x') inside the crop has m0 = 0 and (y-y')^2 + (x-x')^2 <= r^2
    shift = 0: out = m0;  out is one byte, 0 or 1

Written from the definition: ``reached`` is an OR over the offsets of the disc, one shifted view of the zero-padded
source plane per offset (the padding is the "never a source" of positions outside the crop); a grow is ``reached`` of the
subject, a shrink the NOR of ``reached`` of the background.  Nothing here knows of rows of the disc, of distances or of
tiles.  No scipy here.  Also the pattern builders of the tests."""
import numpy as np

NUM_CLASSES = 19
DEFAULT_BITS = sum(1 << c for c in range(1, NUM_CLASSES))
ONE_17 = (1 << 1) | (1 << 17)
SUBJECT_BITS = 1 << 1
TILE_W, TILE_H = 64, 64                     # kTile of csrc/fcp_mask_shift.hip
MAX_SHIFT = 64                              # kMaxShift


def mask0(labels, bits):
    """labels (..., H, W) uint8 -> m0 as bool."""
    lut = np.array([c < NUM_CLASSES and bool(bits >> c & 1) for c in range(256)], bool)
    return lut[np.asarray(labels, np.uint8)]


def disc(r):
    """The offsets (dy, dx) with dy^2 + dx^2 <= r^2."""
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def reached(source, r):
    """source (..., H, W) bool -> whether some source pixel inside the plane lies in the disc of radius r around (y, x).
    An unsigned integer plane is as many bool planes as it has bits, each on its own: the OR is bitwise."""
    h, w = source.shape[-2:]
    padded = np.zeros(source.shape[:-2] + (h + 2 * r, w + 2 * r), source.dtype)
    padded[..., r:r + h, r:r + w] = source
    out = np.zeros(source.shape, source.dtype)
    for dy, dx in disc(r):
        if abs(dy) < h and abs(dx) < w:                               # farther than the plane is wide: all padding
            out |= padded[..., r + dy:r + dy + h, r + dx:r + dx + w]
    return out


def grow(m, r):
    return reached(m, r)


def shrink(m, r):
    return ~reached(~m, r)


def shift_planes(m, shift):
    """m (K,H,W) bool -> out (K,H,W) uint8 of 0 / 1, every plane on its own.  The planes travel as the bits of one integer
    plane, up to 64 at a time, so that the OR over the disc runs once for all of them."""
    m = np.asarray(m, bool)
    out = np.zeros(m.shape, np.uint8)
    for k0 in range(0, len(m), 64):
        part = m[k0:k0 + 64]
        dtype = next(t for t in (np.uint8, np.uint16, np.uint32, np.uint64) if len(part) <= 8 * np.dtype(t).itemsize)
        packed = np.zeros(m.shape[1:], dtype)
        for k, plane in enumerate(part):
            packed |= plane.astype(dtype) << dtype(k)
        moved = grow(packed, shift) if shift >= 0 else shrink(packed, -shift)
        for k in range(len(part)):
            out[k0 + k] = (moved >> dtype(k)) & dtype(1)
    return out


def shift_mask(labels, bits, shift):
    """labels (F,H,W) uint8 -> out (F,H,W) uint8 of 0 / 1."""
    return shift_planes(mask0(labels, bits), shift)


# ---- patterns: (rng, h, w) -> (h, w) uint8 labels, class 1 on class 0 unless said otherwise
def _random(density):
    def make(rng, h, w):
        return (rng.random((h, w)) < density).astype(np.uint8)
    return make


def _empty(rng, h, w):
    return np.zeros((h, w), np.uint8)


def _full(rng, h, w):
    return np.ones((h, w), np.uint8)


def _five(h, w):
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]


def _pixels(rng, h, w):
    """One pixel at each corner and at the centre."""
    m = np.zeros((h, w), np.uint8)
    for y, x in _five(h, w):
        m[y, x] = 1
    return m


def _holes(rng, h, w):
    """One hole at each corner and at the centre."""
    return 1 - _pixels(rng, h, w)


def _disc(rng, h, w):
    y, x = np.mgrid[:h, :w]
    return ((2 * y - (h - 1)) ** 2 + (2 * x - (w - 1)) ** 2 <= (2 * min(h, w) // 3) ** 2).astype(np.uint8)


def _checker(rng, h, w):
    return ((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0).astype(np.uint8)


def _seams(rng, h, w):
    """One-pixel lines on both sides of every tile seam, rows and columns."""
    m = np.zeros((h, w), np.uint8)
    for y in range(TILE_H, h, TILE_H):
        m[y - 1] = 1
    for x in range(TILE_W, w, TILE_W):
        m[:, x] = 1
    if not m.any():                                                   # a plane of one tile: its middle row and column
        m[h // 2] = 1
        m[:, w // 2] = 1
    return m


def _shoulders(rng, h, w):
    """A subject that touches only the bottom border: a half ellipse standing on the last row."""
    y, x = np.mgrid[:h, :w]
    a, b = max(w / 3.0, 0.6), max(2.0 * h / 3.0, 0.6)
    m = (((x - (w - 1) / 2.0) / a) ** 2 + ((y - (h - 1)) / b) ** 2 <= 1.0).astype(np.uint8)
    if h > 1:
        m[0] = 0
    if w > 2:
        m[:, 0] = m[:, -1] = 0
    return m


def _classes(rng, h, w):
    return rng.integers(0, NUM_CLASSES, (h, w)).astype(np.uint8)


PATTERNS = {
    "empty": _empty, "full": _full, "pixels": _pixels, "holes": _holes, "random02": _random(0.02), "random50": _random(0.5),
    "random98": _random(0.98), "disc": _disc, "checker": _checker, "seams": _seams, "shoulders": _shoulders, "classes": _classes,
}
# three faces a call, a different pattern in each; the second is the face-separation case: full, empty, full
GROUPS = [("random02", "random50", "random98"), ("full", "empty", "full"), ("pixels", "holes", "disc"),
          ("checker", "seams", "shoulders"), ("classes", "classes", "classes")]
SEPARATION = GROUPS[1]
CLASS_BITS = (DEFAULT_BITS, 1, ONE_17)      # of the "classes" group


def labels_of(group, rng, h, w):
    return np.stack([PATTERNS[p](rng, h, w) for p in group])


# ---- the synthetic scene of the demonstration number
DEMO_FILL = (0, 177, 64)
DEMO_FEATHER = 5
DEMO_OVERSHOOT = 2


def demo(matte):
    """A 96 x 80 scene whose mask overshoots the true subject by 2 px, composited over a new fill through the feather of
    5 (``matte``: tests/matte_ref.py's ``matte``).  The true subject is a head on shoulders that stand on the bottom
    border (two ellipses, with a concave corner at the neck on either side), in its own colours on an old background of
    others; the mask is the true subject grown by 2, as a parser's resampled label map sits outside it.  The ring is
    the mask's pixels outside the true subject; the error of a composite is its
    mean absolute difference, over the ring and the three channels, from the composite through the true subject.
    -> (the error with the mask as it is, the error with the mask shrunk by 2, the pixels of the ring)."""
    h, w = 96, 80
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    head = (xx - 39.5) ** 2 / 16.0 ** 2 + (yy - 34.0) ** 2 / 22.0 ** 2 <= 1.0
    shoulders = (xx - 39.5) ** 2 / 34.0 ** 2 + (yy - 95.0) ** 2 / 42.0 ** 2 <= 1.0
    true = head | shoulders
    f = np.stack([200 + 20 * np.sin(xx / 5), 60 + 20 * np.cos(yy / 7), np.full((h, w), 50.0)], -1)
    b = np.stack([np.full((h, w), 20.0), 200 + 30 * np.sin(yy / 9), 30 + 20 * np.cos(xx / 4)], -1)
    rng = np.random.default_rng(1)
    f = f + rng.integers(-6, 7, f.shape)
    b = b + rng.integers(-6, 7, b.shape)
    crop = np.where(true[..., None], f, b).round().clip(0, 255).astype(np.uint8)[None]
    mask = shift_planes(true[None], DEMO_OVERSHOOT)
    ring = (mask[0] == 1) & ~true
    ideal = matte(crop, true[None].astype(np.uint8), SUBJECT_BITS, DEMO_FEATHER, DEMO_FILL)[0][0].astype(np.float64)

    def error(labels):
        out = matte(crop, labels, SUBJECT_BITS, DEMO_FEATHER, DEMO_FILL)[0][0].astype(np.float64)
        return float(np.abs(out - ideal)[ring].mean())
    return error(mask), error(shift_mask(mask, SUBJECT_BITS, -DEMO_OVERSHOOT)), int(ring.sum())
