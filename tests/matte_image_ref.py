"""Numpy restatement of the composite over pictures, the reference of the background_image
tests.  It states one thing of its own, which picture lies behind a face; the alpha, the composite and the subject's
colour are those of tests/matte_ref.py and tests/cutout_ref.py, loaded by path and not restated.  For crops c (F,h,w,3)
u8, an alpha plane a (F,h,w) u8, a bank (K,h,w,3) u8 and picks (F,) in 0..K-1:

    P(i)   = bank[picks[i]]                                           the picture of face i, pixel for pixel
    out_ch = (c_ch a + P_ch (255 - a) + 127) // 255                   matte_ref.composite with a per-pixel fill
    out_ch = (F_ch a + P_ch (255 - a) + 127) // 255                   with taps: F = cutout_ref.foreground(c, a, taps)

a == 0 gives the picture's bytes and a == 255 the crop's; a bank of one colour gives matte_ref.matte / cutout_ref.fill
with that colour.
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name + "_for_matte_image",
                                                   os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CR = _load("cutout_ref")
MR = CR.MR

SHAPES = [(1, 1), (1, 7), (5, 3), (33, 47), (64, 64), (70, 130)]       # the 64 x 32 tile of csrc/fcp_matte.hip: see the GPU tests
F, K, PICKS = 3, 2, (1, 0, 1)


def behind(bank, picks):
    """(F,h,w,3) u8: the picture of every face."""
    return np.asarray(bank)[np.asarray(picks, np.int64).reshape(-1)]


def composite(crops, alpha, bank, picks, taps=None):
    """-> (F,h,w,3) u8: the crops, or with taps their estimated subject colours, over their pictures through alpha."""
    colour = np.asarray(crops) if taps is None else CR.foreground(crops, alpha, taps)
    return MR.composite(colour, alpha, behind(bank, picks))


def matte_image(crops, labels, bits, feather, bank, picks, taps=None):
    """-> (out (F,h,w,3) u8, alpha (F,h,w) u8) with the feathered mask of the labels as the alpha."""
    alpha = CR.feathered(labels, bits, feather)
    return composite(crops, alpha, bank, picks, taps), alpha


def random_bank(rng, k, h, w):
    return rng.integers(0, 256, (k, h, w, 3), dtype=np.uint8)


def constant_bank(colour, h, w, k=1):
    return np.broadcast_to(np.array(colour, np.uint8), (k, h, w, 3)).copy()
