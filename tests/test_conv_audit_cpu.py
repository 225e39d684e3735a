"""The float64 reference of the launch auditor (tests/conv_audit.py) against torch.nn.functional in float64, on the CPU:
every epilogue option, the nearest-resize residual, in_up2, the two-source conv, row bands, the chain forms, both stems,
the max-pool, the split32 decoder, and the pixel classes the sampler must return.  What the GPU audit trusts is checked
here first."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _load():
    spec = importlib.util.spec_from_file_location("_conv_audit", os.path.join(os.path.dirname(__file__), "conv_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


A = _load()
TOL = 1e-11


def _act(v: torch.Tensor, fmt: int, c0: int = 0, ld: int | None = None):
    """NCHW float64 values -> an engine Act view (channels [c0, c0 + c) of an ld-channel NHWC buffer) holding them in format
    ``fmt``; returns (act, the values the buffer really holds, NCHW float64)."""
    from face_crop_plus_amd import engine as E
    n, c, h, w = v.shape
    ld = ld or c0 + c
    nhwc = v.permute(0, 2, 3, 1).contiguous()
    buf = torch.randn(n, h, w, ld, dtype=torch.float32)                    # junk outside the view
    if fmt == 1:
        buf[..., c0:c0 + c] = A.encode(nhwc)
        held = A.decode(buf[..., c0:c0 + c], 1)
    else:
        buf[..., c0:c0 + c] = nhwc.float()
        held = buf[..., c0:c0 + c].double()
    return E.Act(buf, c0, c, fmt), held.permute(0, 3, 1, 2).contiguous()


def _at(ref_nchw: torch.Tensor, mi: torch.Tensor):
    n, c, h, w = ref_nchw.shape
    return ref_nchw.permute(0, 2, 3, 1).reshape(-1, c)[mi]


def _all(n, h, w):
    return torch.arange(n * h * w)


def test_split32_decoder_reads_hi_then_lo_planes():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(3, 64, generator=g, dtype=torch.float64) * 100
    hi = v.numpy().astype(np.float16)
    lo = (v.numpy() - hi.astype(np.float64)).astype(np.float16)
    raw = np.empty((3, 2, 2, 32), np.float16)                              # per 32 channels: 32 hi, then 32 lo
    raw[:, :, 0] = hi.reshape(3, 2, 32)
    raw[:, :, 1] = lo.reshape(3, 2, 32)
    got = A.decode(torch.from_numpy(raw.reshape(3, 128).view(np.float32).copy()), 1)
    want = torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64))
    assert torch.equal(got, want)
    assert (got - v).abs().max() <= 2.0 ** -21 * v.abs().max()
    assert torch.equal(A.decode(A.encode(v), 1), got)
    assert torch.equal(A.decode(v.float(), 0), v.float().double())


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (1, 1, 0), (3, 2, 1), (1, 2, 0), (7, 2, 3)])
def test_ref_conv_plain(k, stride, pad, fmt):
    g = torch.Generator().manual_seed(k * 10 + stride)
    x = torch.randn(2, 64, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(48, 64, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(48, generator=g, dtype=torch.float64)
    xa, xv = _act(x, fmt, c0=32, ld=128)
    ref = F.conv2d(xv, w, b, stride, pad)
    oh, ow = ref.shape[2:]
    got = A.ref_conv(w, b, stride, pad, xa, _all(2, oh, ow), oh, ow, chunk=37)
    assert (got - _at(ref, _all(2, oh, ow))).abs().max() <= TOL * ref.abs().max()


@pytest.mark.parametrize("res1_pre", [True, False])
@pytest.mark.parametrize("res_size", [(8, 10), (4, 5), (3, 7)])     # same size, exact 2x, odd nearest resize
def test_ref_conv_epilogue(res1_pre, res_size):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 32, 8, 10, generator=g, dtype=torch.float64)
    w = torch.randn(64, 32, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(64, generator=g, dtype=torch.float64)
    r1 = torch.randn(2, 64, *res_size, generator=g, dtype=torch.float64)
    r2 = torch.randn(2, 64, 8, 10, generator=g, dtype=torch.float64)
    slope, alpha, alpha2 = 0.2, 0.7, 0.3
    xa, xv = _act(x, 1)
    r1a, r1v = _act(r1, 1, c0=64, ld=128)
    r2a, r2v = _act(r2, 0, c0=0, ld=96)
    v = F.conv2d(xv, w, b, 1, 1)
    up = F.interpolate(r1v, size=(8, 10), mode="nearest")
    if res1_pre:
        v = v + up
    v = F.leaky_relu(v, slope) * alpha
    if not res1_pre:
        v = v + up
    v = v * alpha2 + r2v
    mi = _all(2, 8, 10)
    got = A.ref_conv(w, b, 1, 1, xa, mi, 8, 10, act_slope=slope, alpha=alpha, res1=r1a, res1_pre=res1_pre, res2=r2a, alpha2=alpha2)
    assert (got - _at(v, mi)).abs().max() <= TOL * v.abs().max()
    relu = A.ref_conv(w, None, 1, 1, xa, mi, 8, 10, act_slope=0.0)
    assert (relu - _at(torch.relu(F.conv2d(xv, w, None, 1, 1)), mi)).abs().max() <= TOL * relu.abs().max()


def test_nearest_rule_is_pytorchs():
    for src, dst in [(25, 50), (13, 26), (7, 20), (20, 7), (160, 320), (3, 3)]:
        d = torch.arange(dst)
        want = F.interpolate(torch.arange(src, dtype=torch.float64)[None, None, :, None], size=(dst, 1), mode="nearest").flatten().long()
        assert torch.equal(A.nearest_src(d, src, dst), want), (src, dst)


def test_ref_conv_in_up2():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(32, 64, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(32, generator=g, dtype=torch.float64)
    xa, xv = _act(x, 1)
    ref = F.leaky_relu(F.conv2d(F.interpolate(xv, scale_factor=2, mode="nearest"), w, b, 1, 1), 0.2)
    mi = _all(1, 10, 14)
    got = A.ref_conv(w, b, 1, 1, xa, mi, 10, 14, act_slope=0.2, in_up2=True)
    assert (got - _at(ref, mi)).abs().max() <= TOL * ref.abs().max()


@pytest.mark.parametrize("s", [1, 2])
def test_ref_conv_two_source(s):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 6, 5, generator=g, dtype=torch.float64)
    x2 = torch.randn(2, 96, 6 * s, 5 * s, generator=g, dtype=torch.float64)
    w = torch.randn(128, 160, 1, 1, generator=g, dtype=torch.float64)
    b = torch.randn(128, generator=g, dtype=torch.float64)
    xa, xv = _act(x, 1, c0=0, ld=96)
    x2a, x2v = _act(x2, 1, c0=32, ld=128)
    ref = torch.relu(F.conv2d(torch.cat([xv, x2v[:, :, ::s, ::s]], 1), w, b))
    mi = _all(2, 6, 5)
    got = A.ref_conv(w, b, 1, 0, xa, mi, 6, 5, act_slope=0.0, x2=x2a, x2_stride=s)
    assert (got - _at(ref, mi)).abs().max() <= TOL * ref.abs().max()


@pytest.mark.parametrize("a,b_", [(0, 4), (3, 7), (5, 12), (0, 12)])
def test_ref_conv_band_is_rows_of_the_whole_image(a, b_):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 32, 12, 9, generator=g, dtype=torch.float64)
    w = torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64)
    full = F.conv2d(x, w, None, 1, 1)
    bt, bb = (1 if a > 0 else 0), (1 if b_ < 12 else 0)
    xa, _ = _act(x[:, :, a - bt:b_ + bb].contiguous(), 0)
    mi = _all(1, b_ - a, 9)
    got = A.ref_conv(w.float().double(), None, 1, 1, xa, mi, b_ - a, 9, band=(bt, bb))
    ref = _at(F.conv2d(x.float().double(), w.float().double(), None, 1, 1)[:, :, a:b_].contiguous(), mi)
    assert (got - ref).abs().max() <= TOL * full.abs().max()


def test_ref_chain_forms():
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n, h, w = 2, 7, 9
    mi = _all(n, h, w)
    # conv2 form: t2 = relu(conv2_3x3(t1)), out = relu(conv3(t2) + res), t1n = relu(conv1'(out))
    t1, res = rn(n, 64, h, w), rn(n, 256, h, w)
    W = {"w2": rn(64, 64, 3, 3) / 8, "b2": rn(64), "w3": rn(256, 64, 1, 1) / 8, "b3": rn(256)}
    w1, b1 = rn(128, 256, 1, 1) / 16, rn(128)
    t1a, t1v = _act(t1, 1)
    ra, rv = _act(res, 1)
    t2 = torch.relu(F.conv2d(t1v, W["w2"], W["b2"], 1, 1))
    out = torch.relu(F.conv2d(t2, W["w3"], W["b3"]) + rv)
    got = A.ref_chain(W, t1a, ra, mi, chunk=50)
    assert (got - _at(out, mi)).abs().max() <= TOL * out.abs().max()
    t1n = torch.relu(F.conv2d(out, w1, b1))
    assert (A.ref_1x1_relu(w1, b1, got) - _at(t1n, mi)).abs().max() <= TOL * t1n.abs().max()
    # pair form without residual, over a [conv2 out | stem] concat view
    cat = rn(n, 128, h, w)
    Wp = {"w3": rn(256, 128, 1, 1) / 8, "b3": rn(256)}
    ca, cv = _act(cat, 1)
    out = torch.relu(F.conv2d(cv, Wp["w3"], Wp["b3"]))
    assert (A.ref_chain(Wp, ca, None, mi) - _at(out, mi)).abs().max() <= TOL * out.abs().max()
    # two-source pair form: [t1 (128) | t1b(::2, ::2) (256)]
    t1b = rn(n, 256, 2 * h, 2 * w)
    Wt = {"w3": rn(512, 384, 1, 1) / 16, "b3": rn(512)}
    t1a, t1v = _act(rn(n, 128, h, w), 1)
    tba, tbv = _act(t1b, 1)
    out = torch.relu(F.conv2d(torch.cat([t1v, tbv[:, :, ::2, ::2]], 1), Wt["w3"], Wt["b3"]))
    got = A.ref_chain(Wt, t1a, None, mi, t1b=tba, t1b_stride=2)
    assert (got - _at(out, mi)).abs().max() <= TOL * out.abs().max()


def test_ref_stems_and_maxpool():
    g = torch.Generator().manual_seed(13)
    n, h, w = 2, 37, 30
    img = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    wt = torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64) / 20
    b = torch.randn(64, generator=g, dtype=torch.float64)
    mean = (123, 117, 104)
    x = img.permute(0, 3, 1, 2).double() - torch.tensor(mean, dtype=torch.float64)[:, None, None]
    pooled = F.max_pool2d(torch.relu(F.conv2d(x, wt, b, 2, 3)), 3, 2, 1)
    hp, wp = pooled.shape[2:]
    assert (hp, wp) == ((((h - 1) // 2) // 2) + 1, (((w - 1) // 2) // 2) + 1)
    pi = _all(n, hp, wp)
    got = A.ref_stem(wt, b, img, pi, hp, wp, mean=mean, chunk=29)
    assert (got - _at(pooled, pi)).abs().max() <= TOL * pooled.abs().max()
    # fp32 NHWC4 stem (channel 3 is ignored)
    x4 = torch.randn(n, h, w, 4, generator=g, dtype=torch.float32)
    pooled = F.max_pool2d(torch.relu(F.conv2d(x4[..., :3].permute(0, 3, 1, 2).double(), wt, b, 2, 3)), 3, 2, 1)
    got = A.ref_stem(wt, b, x4, pi, hp, wp)
    assert (got - _at(pooled, pi)).abs().max() <= TOL * pooled.abs().max()
    # max-pool of a split32 view
    y = torch.randn(n, 64, 11, 8, generator=g, dtype=torch.float64)
    ya, yv = _act(y, 1)
    mp = F.max_pool2d(yv, 3, 2, 1)
    pi = _all(n, *mp.shape[2:])
    assert torch.equal(A.ref_maxpool(ya, pi, *mp.shape[2:]), _at(mp, pi))


def test_sampler_returns_every_required_pixel_class():
    g = torch.Generator().manual_seed(0)
    n, oh, ow = 9, 40, 33
    m = n * oh * ow
    s = A.sample_rows(n, oh, ow, g, nrand=4096, bounds=(4,))
    assert torch.equal(s, torch.unique(s)) and int(s.min()) >= 0 and int(s.max()) < m
    have = set(s.tolist())
    assert set(range(A.EDGE_ROWS)) <= have and set(range(m - A.EDGE_ROWS, m)) <= have          # both ends of M
    ni, ho, wo = A.split_m(torch.arange(m), oh, ow)
    edge = ((ho == 0) | (ho == oh - 1) | (wo == 0) | (wo == ow - 1)).nonzero().flatten().tolist()
    assert set(edge) <= have                                                                      # every image's border
    r = 4 * oh * ow
    assert set(range(r - A.EDGE_ROWS, r + A.EDGE_ROWS)) <= have                                  # both sides of a boundary
    inner = s[(s >= A.EDGE_ROWS) & (s < m - A.EDGE_ROWS)]
    ni, ho, wo = A.split_m(inner, oh, ow)
    interior = inner[(ho > 0) & (ho < oh - 1) & (wo > 0) & (wo < ow - 1)]
    assert len(interior) > 1500                                                                   # random pixels ...
    assert len(set(A.split_m(interior, oh, ow)[0].tolist())) == n                                # ... in every image
    big = A.sample_rows(64, 256, 256, g)
    assert len(big) >= 4096 + 2 * A.EDGE_ROWS


def test_family_names():
    assert A.conv_family("conv 3x3 s1 64->64 @8x8 tile 256x256 bal +res", 1, 1) == "conv 256 bal"
    assert A.conv_family("conv 3x3 s1 64->64 @8x8 tile 256x128", 1, 1) == "conv 256"
    assert A.conv_family("conv 3x3 s1 64->64 @8x8 tile 1x32", 1, 1) == "conv halo"
    assert A.conv_family("conv 3x3 s1 64->64 @8x8 tile 1x128", 1, 1) == "conv halo-wide"
    assert A.conv_family("conv 3x3 s1 64->64 @8x8 tile 128x64", 1, 1) == "conv 128 dma"
    assert A.conv_family("conv 3x3 s1 64->64 @8x8 tile 128x64", 0, 0) == "conv f32"
    assert A.chain_family("chain 3x3 64->256->64 @8x8 +res out@even") == "chain 3x3 out@even"
    assert A.chain_family("chain 384->512->128 @8x8 two-source") == "chain two-source"
    assert A.chain_family("expand 256->1024 @8x8 +res") == "chain expand"
