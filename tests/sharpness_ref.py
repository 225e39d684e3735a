"""Numpy restatement of the sharpness measure, the reference of the sharpness tests:

1. gray       g = (9798 R + 19235 G + 3735 B + 16384) >> 15             (OpenCV 4.x 8-bit COLOR_RGB2GRAY)
2. Laplacian  L(y,x) = g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4 g(y,x), BORDER_REFLECT_101 (-1 -> 1, n -> n-2; a
              dimension of size 1 maps every neighbour to index 0)      (cv2.Laplacian(gray, CV_64F), ksize = 1)
3. sums       S1 = sum L, S2 = sum L*L over the N = H*W pixels, exact integers
4. score      (N*S2 - S1*S1) / (N*N): numerator in Python integers, one correctly rounded division
"""
import numpy as np


def gray(img):
    """(H,W,3) uint8 RGB -> (H,W) uint8."""
    v = np.asarray(img).astype(np.int64)
    return ((9798 * v[..., 0] + 19235 * v[..., 1] + 3735 * v[..., 2] + 16384) >> 15).astype(np.uint8)


def _reflect101(n):
    """Indices of the neighbours -1 .. n of a dimension of size n."""
    idx = np.arange(-1, n + 1)
    if n == 1:
        return np.zeros_like(idx)
    idx[0], idx[-1] = 1, n - 2
    return idx


def laplacian(g):
    """(H,W) gray -> (H,W) int64."""
    g = np.asarray(g).astype(np.int64)
    h, w = g.shape
    p = g[_reflect101(h)][:, _reflect101(w)]
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * g


def sums(img):
    """(H,W,3) uint8 -> (S1, S2) Python integers."""
    lap = laplacian(gray(img))
    return int(lap.sum()), int((lap * lap).sum())


def score(img):
    """(H,W,3) uint8 -> float: the population variance of the Laplacian."""
    s1, s2 = sums(img)
    n = int(img.shape[0]) * int(img.shape[1])
    return (n * s2 - s1 * s1) / (n * n)
