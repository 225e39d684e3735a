"""The conv kernels return the bits they returned before their shared code was stated once (fcp_conv_common.h): the fused
epilogue's arithmetic (conv_value) and the generic kernels' im2col walk (xcd_tile_order, conv_row, TapWalk / set_tap, dma_slice).

``torch.equal`` treats -0.0 and 0.0 as equal and no other test compares a commit with its parent, so every case of
tests/conv_epilogue_cases.py asserts

1. that every tile choice offered for the shape gives the same BYTES (compared as int32), and
2. that their sha256 is the one in tests/golden/conv_epilogue_bits.json, recorded on an MI355X at the parent commit by
   tests/golden/make_golden_conv_epilogue.py.  A case without a recorded hash fails.

The epilogue cases: each generic epilogue behind each generic kernel under five epilogue settings, the halo-tile kernels, the
bottleneck-chain forms, the fused stem + pool + conv1 (hashes from the parent of the commit that gathered the epilogue).  The
walk cases, under one epilogue setting: stride 2, 25 taps, one / two / three K slices, a ragged M tile across an image boundary,
the nearest-x2 fetch, the 3-channel NHWC4 mode, row bands, a second source and flat addressing, each on every generic kernel
that takes it (hashes from the parent of the commit that gathered the walk, which reproduced the older ones).  The halo walk
cases, under the same setting, each next to the generic tile of its shape: the nearest-x2 fetch on the four halo forms, 3 / 4
slices (narrow) and three 18-tap units (wide), row bands, and 2 x 1040 x 33 images whose 520 patches make every workgroup walk
two or three tiles (hashes from the parent of the commit that gathered the halo kernels' shared pieces, likewise).

A ReLU case must hold at least one -0.0 (a negative pre-activation times slope 0: part of the epilogue's contract) and one
positive value, a resized-residual case a residual map smaller than the output: no case passes trivially.

A later change that legitimately changes bits — a different K order, say — regenerates the hashes with the generator script.
"""
import json
import os

import pytest
import torch

import conv_epilogue_cases as CE

pytestmark = pytest.mark.gpu

CASES = CE.cases()
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_epilogue_bits.json")) as _f:
    GOLDEN = json.load(_f)["hashes"]


def _signs(raw, fmt, view):
    """(holds a -0.0, holds a positive value) of an output buffer given as int32 [n, h, w, ld]."""
    if fmt == 1:                       # split32: per 32 channels 32 binary16 hi parts, then 32 lo parts; -0.0 = hi 0x8000, lo +0
        g = raw.view(torch.int16).reshape(-1, 2, 32).to(torch.int32) & 0xFFFF
        hi, lo = g[:, 0], g[:, 1]
        return bool(((hi == 0x8000) & ((lo & 0x7FFF) == 0)).any()), bool(((hi > 0) & (hi < 0x7C00)).any())
    c0, c = view if view is not None else (0, raw.shape[-1])
    v = raw[..., c0:c0 + c]
    return bool((v == -(1 << 31)).any()), bool((v.view(torch.float32) > 0).any())


@pytest.mark.parametrize("case_id,kind,spec", CASES, ids=[c[0] for c in CASES])
def test_epilogue_bits(case_id, kind, spec, device):
    outs, info = CE.run_case(case_id, kind, spec, device)
    labels = list(outs)
    first = outs[labels[0]]
    for label in labels[1:]:
        for a, b in zip(first, outs[label]):
            assert a.shape == b.shape and bool((a == b).all()), f"tile {label} and tile {labels[0]} give different bytes"
    if info["res1_smaller"] is not None:
        assert info["res1_smaller"], "the resized residual must be smaller than the output"
    if CE.slope0(kind, spec):
        neg0, pos = _signs(first[0], info["fmt"], info["view"])
        assert neg0 and pos, f"a ReLU case must hold -0.0 ({neg0}) and positive values ({pos})"
    assert case_id in GOLDEN, "no recorded hash for this case (tests/golden/make_golden_conv_epilogue.py)"
    assert CE.digest(first) == GOLDEN[case_id], "bytes differ from the ones recorded at the parent commit"


def test_every_recorded_hash_has_a_case():
    assert set(GOLDEN) == {c[0] for c in CASES}
