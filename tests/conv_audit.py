"""Launch auditor of the conv engine (test helper, not a test module).

While a model ``load()``s, ``Auditor.record()`` keeps the host-folded fp32 weights of every packed filter (``fold_bn``'s
output after ``cin_perm``) — not weights unpacked from the device image, so a packing or hi / lo split bug shows up as an
error.  While a model runs, ``Auditor.audit()`` wraps the engine entry points the networks call (``conv``,
``bottleneck_chain``, ``stem_relu_pool_u8``, ``stem_relu_pool_f32``, ``maxpool3x3s2``): every launch is synchronised
and checked at once against a float64 reference of the op ``include/fcp_hip.h`` documents, on a sample of output pixels
(all output channels), before the next launch can overwrite anything.

The reference functions below are plain torch on whatever device the tensors live on; they never call the engine (split32
tensors are decoded from their binary16 hi / lo bytes here, not by ``split32_to_f32``).  tests/test_conv_audit_cpu.py checks
them against ``torch.nn.functional`` in float64.
"""
from __future__ import annotations

import contextlib
import inspect
import re

import numpy as np
import torch

TOL_REL, TOL_ABS = 2e-5, 1e-6      # the suite's conv rule (tests/test_conv_gpu.py::_tol), here against float64
F32_FACTOR = 3                     # the exact-fp32 path gets 3x (test_conv_randomized_shapes)
EDGE_ROWS = 512                    # first / last rows of M always sampled
N_RANDOM = 4096                    # uniformly random pixels over all images


# ----------------------------------------------------------------------------------------------------- split32 format
def decode(raw: torch.Tensor, fmt: int) -> torch.Tensor:
    """(..., c) float32 storage of a channel view -> float64 values.  fmt 1 (split32): per 32 channels, 32 binary16 hi parts
    then 32 binary16 lo parts in the same 128 bytes; value = hi + lo."""
    if fmt == 0:
        return raw.double()
    c = raw.shape[-1]
    assert c % 32 == 0
    h = raw.contiguous().view(torch.float16).reshape(*raw.shape[:-1], c // 32, 2, 32).double()
    return (h[..., 0, :] + h[..., 1, :]).reshape(*raw.shape[:-1], c)


def encode(v: torch.Tensor) -> torch.Tensor:
    """float values (..., c) -> split32 storage (float32 tensor of the same shape): hi = fp16(v), lo = fp16(v - hi)."""
    c = v.shape[-1]
    v = v.double()
    hi = v.half()
    lo = (v - hi.double()).half()
    out = torch.stack([hi.reshape(*v.shape[:-1], c // 32, 32), lo.reshape(*v.shape[:-1], c // 32, 32)], -2)
    return out.reshape(*v.shape[:-1], 2 * c).contiguous().view(torch.float32)


# -------------------------------------------------------------------------------------------------------------- sampler
def sample_rows(n: int, oh: int, ow: int, gen: torch.Generator, nrand: int = N_RANDOM, bounds=(), device="cpu") -> torch.Tensor:
    """Sorted unique flat output pixels (rows of M = n * oh * ow): the first and last ``EDGE_ROWS`` rows of M, the first and
    last output row and column of every image, ``EDGE_ROWS`` rows on both sides of every image index in ``bounds``
    (sub-batch boundaries inside one launch), and ``nrand`` uniformly random pixels."""
    m = n * oh * ow
    parts = [torch.arange(min(m, EDGE_ROWS)), torch.arange(max(0, m - EDGE_ROWS), m)]
    hw = oh * ow
    img = torch.arange(n)[:, None] * hw
    cols = torch.arange(ow)
    rows = torch.arange(oh) * ow
    parts += [(img + cols).flatten(), (img + (oh - 1) * ow + cols).flatten(),
              (img + rows).flatten(), (img + rows + ow - 1).flatten()]
    for b in bounds:
        r = b * hw
        parts.append(torch.arange(max(0, r - EDGE_ROWS), min(m, r + EDGE_ROWS)))
    parts.append(torch.randint(0, m, (nrand,), generator=gen))
    return torch.unique(torch.cat(parts)).to(device)


def split_m(m_idx: torch.Tensor, oh: int, ow: int):
    hw = oh * ow
    ni = torch.div(m_idx, hw, rounding_mode="floor")
    rem = m_idx - ni * hw
    ho = torch.div(rem, ow, rounding_mode="floor")
    return ni, ho, rem - ho * ow


def _gather(t, ni, y, x, c0, c, fmt) -> torch.Tensor:
    """Values of channels [c0, c0 + c) of the NHWC buffer ``t`` (n, h, w, ld) at integer pixels (any shape), float64; pixels
    outside the image read 0."""
    n, h, w, ld = t.shape
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    flat = (ni * h + y.clamp(0, h - 1)) * w + x.clamp(0, w - 1)
    raw = t.view(-1, ld)[:, c0:c0 + c][flat.flatten()]
    v = decode(raw, fmt).reshape(*flat.shape, c)
    return v * ok[..., None]


def gather_act(a, ni, y, x) -> torch.Tensor:
    return _gather(a.buf, ni, y, x, a.c0, a.c, a.fmt)


def nearest_src(dst: torch.Tensor, src_size: int, dst_size: int) -> torch.Tensor:
    """PyTorch's nearest rule as fcp_hip.h states it: min(floor(dst * (float)src / dst_size), src - 1), in float32."""
    scale = np.float32(src_size) / np.float32(dst_size)
    return torch.clamp(torch.floor(dst.float() * float(scale)).long(), max=src_size - 1)


# --------------------------------------------------------------------------------------------------------------- conv
def ref_conv(w: torch.Tensor, b, stride: int, pad: int, x, m_idx: torch.Tensor, oh: int, ow: int, *, act_slope=1.0,
             alpha=1.0, res1=None, res1_pre=True, res2=None, alpha2=1.0, in_up2=False, x2=None, x2_stride=1,
             band=(0, 0), chunk: int = 4096) -> torch.Tensor:
    """float64 (S, cout) of ``fcp_conv2d_nhwc_f32`` at the flat output pixels ``m_idx``.  ``w`` (cout, cin, kh, kw) float64 on
    the device of the tensors (the trailing ``x2.c`` input channels read ``x2``), ``b`` (cout,) or None."""
    cout, cin, kh, kw = w.shape
    c1 = cin - (x2.c if x2 is not None else 0)
    if c1 < x.c:                       # cin4 mode: an NHWC4 input, the filter's missing channels weigh 0
        assert x2 is None and x.c == 4
        w, c1 = torch.cat([w, w.new_zeros(cout, 4 - c1, kh, kw)], 1), 4
    assert c1 == x.c
    w1 = w[:, :c1].permute(0, 2, 3, 1).reshape(cout, -1)               # K order (ky, kx, c)
    in_h, in_w = (x.h * 2, x.w * 2) if in_up2 else (x.h, x.w)
    ky, kx = torch.meshgrid(torch.arange(kh, device=m_idx.device), torch.arange(kw, device=m_idx.device), indexing="ij")
    ky, kx = ky.flatten(), kx.flatten()
    outs = []
    for s in range(0, len(m_idx), chunk):
        mi = m_idx[s:s + chunk]
        ni, ho, wo = split_m(mi, oh, ow)
        y = ho[:, None] * stride - pad + band[0] + ky[None, :]
        xx = wo[:, None] * stride - pad + kx[None, :]
        ok = (y >= 0) & (y < in_h) & (xx >= 0) & (xx < in_w)
        if in_up2:
            y, xx = torch.div(y, 2, rounding_mode="floor"), torch.div(xx, 2, rounding_mode="floor")
        win = gather_act(x, ni[:, None].expand_as(y), y, xx) * ok[..., None]      # (S, T, c1)
        v = win.reshape(len(mi), -1) @ w1.T
        if x2 is not None:
            assert (kh, kw, pad) == (1, 1, 0)
            v = v + gather_act(x2, ni, ho * x2_stride, wo * x2_stride) @ w[:, c1:, 0, 0].T
        if b is not None:
            v = v + b
        r1 = None
        if res1 is not None:
            r1 = gather_act(res1, ni, nearest_src(ho, res1.h, oh), nearest_src(wo, res1.w, ow))
            if res1_pre:
                v = v + r1
        v = torch.where(v >= 0, v, v * act_slope) * alpha
        if res1 is not None and not res1_pre:
            v = v + r1
        if res2 is not None:
            v = v * alpha2 + gather_act(res2, ni, ho, wo)
        outs.append(v)
    return torch.cat(outs)


# -------------------------------------------------------------------------------------------------------------- chain
def ref_chain(W, t1, res, m_idx, *, t1b=None, t1b_stride=1, chunk: int = 4096):
    """float64 ``out`` (S, nout) of ``fcp_bottleneck_chain_f16x3`` at ``m_idx`` of the (n, h, w) grid of ``t1``.  ``W``: dict with
    ("w3", "b3") and optionally ("w2", "b2") (the conv2 forms: t2 = relu(conv2_3x3(t1) + b2) on the 3x3 neighbourhood)."""
    h, w = t1.h, t1.w
    outs = []
    for s in range(0, len(m_idx), chunk):
        mi = m_idx[s:s + chunk]
        if W.get("w2") is not None:
            t2 = torch.relu(ref_conv(W["w2"], W["b2"], 1, 1, t1, mi, h, w))
        else:
            ni, ho, wo = split_m(mi, h, w)
            t2 = gather_act(t1, ni, ho, wo)
            if t1b is not None:
                t2 = torch.cat([t2, gather_act(t1b, ni, ho * t1b_stride, wo * t1b_stride)], 1)
        v = t2 @ W["w3"][:, :, 0, 0].T + W["b3"]
        if res is not None:
            ni, ho, wo = split_m(mi, h, w)
            v = v + gather_act(res, ni, ho, wo)
        outs.append(torch.relu(v))
    return torch.cat(outs)


def ref_1x1_relu(w, b, vals):
    """relu(conv1x1(vals) + b) on (S, cin) float64 values: conv1' of a chain, conv1 of the fused stem."""
    return torch.relu(vals @ w[:, :, 0, 0].T + b)


# --------------------------------------------------------------------------------------------------------------- stem
def ref_stem(w, b, src, p_idx, hp, wp, *, mean=None, chunk: int = 2048):
    """float64 pooled stem (S, 64) at flat pooled pixels ``p_idx``: 7x7 / 2 / pad 3 conv (``w`` (64, 3, 7, 7), BN folded) + bias
    -> ReLU -> 3x3 / 2 / pad 1 max-pool.  ``src``: (n, h, w, 3) uint8 RGB with ``mean`` (3 ints) subtracted, or an fp32
    NHWC4 tensor (n, h, w, 4) whose channels 0..2 are used (``mean`` None)."""
    n, h, wd = src.shape[:3]
    hs, ws = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    dev = p_idx.device
    wk = w.permute(0, 2, 3, 1).reshape(64, -1)                            # K order (ky, kx, c)
    d = torch.arange(-1, 2, device=dev)
    k7 = torch.arange(7, device=dev)
    outs = []
    for s in range(0, len(p_idx), chunk):
        ni, py, px = split_m(p_idx[s:s + chunk], hp, wp)
        sy = (2 * py[:, None, None] + d[None, :, None]).expand(-1, 3, 3)  # (S, 3, 3) stem pixels of the pool window
        sx = (2 * px[:, None, None] + d[None, None, :]).expand(-1, 3, 3)
        valid = (sy >= 0) & (sy < hs) & (sx >= 0) & (sx < ws)
        y = sy[..., None, None] * 2 - 3 + k7[:, None]                      # (S, 3, 3, 7, 1)
        x = sx[..., None, None] * 2 - 3 + k7[None, :]                      # (S, 3, 3, 1, 7)
        y, x = torch.broadcast_tensors(y, x)
        nn = ni[:, None, None, None, None].expand_as(y)
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < wd)
        flat = (nn * h + y.clamp(0, h - 1)) * wd + x.clamp(0, wd - 1)
        if mean is not None:
            pix = src.reshape(-1, 3)[flat.flatten()].double() - torch.tensor([float(m) for m in mean], dtype=torch.float64, device=dev)
        else:
            pix = src.reshape(-1, src.shape[3])[flat.flatten(), :3].double()
        pix = pix.reshape(*flat.shape, 3) * ok[..., None]
        conv = torch.relu(pix.reshape(*valid.shape, -1) @ wk.T + b)        # (S, 3, 3, 64)
        conv = torch.where(valid[..., None], conv, torch.full_like(conv, -float("inf")))
        outs.append(conv.flatten(1, 2).amax(1))
    return torch.cat(outs)


def ref_maxpool(x, p_idx, oh, ow) -> torch.Tensor:
    """float64 MaxPool2d(3, 2, 1) of the dense NHWC view ``x`` at flat output pixels ``p_idx``."""
    ni, py, px = split_m(p_idx, oh, ow)
    d = torch.arange(-1, 2, device=p_idx.device)
    y = (2 * py[:, None, None] + d[None, :, None]).expand(-1, 3, 3)
    xx = (2 * px[:, None, None] + d[None, None, :]).expand(-1, 3, 3)
    ok = (y >= 0) & (y < x.h) & (xx >= 0) & (xx < x.w)
    v = gather_act(x, ni[:, None, None].expand_as(y), y, xx)
    v = torch.where(ok[..., None], v, torch.full_like(v, -float("inf")))
    return v.flatten(1, 2).amax(1)


# ------------------------------------------------------------------------------------------------------------ auditor
def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else (None if v is None else np.asarray(v))


def _clone_view(a):
    """A private copy of an operand view (channels only, same format)."""
    return type(a)(a.buf[..., a.c0:a.c0 + a.c].contiguous(), fmt=a.fmt)


def _overlaps(t, out) -> bool:
    """The overlap test of ``engine._alias_safe_out`` (tuner trials, relaunches): same storage and intersecting channel ranges."""
    return (t is not None and t.buf.untyped_storage().data_ptr() == out.buf.untyped_storage().data_ptr()
            and t.c0 < out.c0 + out.c and out.c0 < t.c0 + t.c)


def conv_family(label: str, precision: int, in_fmt: int) -> str:
    m = re.search(r"tile (\d+)x(\d+)( bal)?", label)
    tm, tn, bal = int(m.group(1)), int(m.group(2)), bool(m.group(3))
    if precision == 0:
        return "conv f32"
    if tm == 1:
        return "conv halo" if tn == 32 else "conv halo-wide"
    if tm == 256:
        return "conv 256 bal" if bal else "conv 256"
    return "conv 128 dma" if in_fmt == 1 else "conv 128 f16x3"


def chain_family(label: str) -> str:
    if label.startswith("expand"):
        return "chain expand"
    fam = "chain 3x3" if "3x3" in label else ("chain two-source" if "two-source" in label else "chain pair")
    if "out@even" in label:
        fam += " out@even"
    return fam


class AuditError(AssertionError):
    pass


class Auditor:
    def __init__(self, engine, seed: int = 0, nrand: int = N_RANDOM, verbose: bool = True, bounds=()):
        self.E = engine
        self.W = {}          # id(packed object) -> dict(obj=<kept alive>, w=float64 host, b=..., stride, pad, precision)
        self.dev_w = {}
        self.rows = []       # (label, family, samples, err / tol)
        self.gen = torch.Generator().manual_seed(seed)
        self.nrand, self.verbose, self.bounds = nrand, verbose, bounds

    # ------------------------------------------------------------------ weights
    @contextlib.contextmanager
    def record(self):
        E = self.E
        orig_pc, orig_ps = E.pack_conv, E.pack_stem_fused

        def pack_conv(weight, bias=None, bn=None, stride=1, pad=0, device="cuda", cin_perm=None, precision=None):
            pc = orig_pc(weight, bias, bn, stride, pad, device, cin_perm, precision)
            bnn = None if bn is None else {k: _np(v) for k, v in bn.items()}
            w, b = E.fold_bn(_np(weight), bnn, _np(bias))
            if cin_perm is not None:
                w = w[:, cin_perm]
            self.W[id(pc)] = dict(obj=pc, w=np.asarray(w, np.float64), b=None if b is None else np.asarray(b, np.float64),
                                  stride=stride, pad=pad, precision=pc.precision)
            return pc

        def pack_stem_fused(weight, bn, device, cin_perm=None):
            ps = orig_ps(weight, bn, device, cin_perm)
            w, b = E.fold_bn(_np(weight), {k: _np(v) for k, v in bn.items()}, None)
            if cin_perm is not None:
                w = w[:, cin_perm]
            self.W[id(ps)] = dict(obj=ps, w=np.asarray(w, np.float64), b=np.asarray(b, np.float64), stride=2, pad=3, precision=1)
            return ps

        E.pack_conv, E.pack_stem_fused = pack_conv, pack_stem_fused
        try:
            yield self
        finally:
            E.pack_conv, E.pack_stem_fused = orig_pc, orig_ps

    def _w(self, obj, dev):
        key = (id(obj), str(dev))
        if key not in self.dev_w:
            assert id(obj) in self.W and self.W[id(obj)]["obj"] is obj, "launch of a filter packed outside Auditor.record()"
            r = self.W[id(obj)]
            self.dev_w[key] = (torch.from_numpy(r["w"]).to(dev), None if r["b"] is None else torch.from_numpy(r["b"]).to(dev))
        return self.dev_w[key]

    def forget_weights(self):
        self.W.clear()
        self.dev_w.clear()

    # ------------------------------------------------------------------ checks
    def _sample(self, n, oh, ow, dev):
        return sample_rows(n, oh, ow, self.gen, self.nrand, self.bounds, dev)

    def _check(self, label, family, got, ref, factor=1, exact=False):
        err = float((got - ref).abs().max())
        tol = 0.0 if exact else factor * (TOL_REL * float(ref.abs().max()) + TOL_ABS)
        ratio = (0.0 if err == 0 else float("inf")) if exact else err / tol
        self.rows.append((label, family, int(got.shape[0]), ratio))
        if self.verbose:
            print(f"audit {label} | {family} | samples {got.shape[0]} | err/tol {ratio:.3g}", flush=True)
        if not ratio <= 1.0:
            raise AuditError(f"{label} ({family}): max |kernel - float64 reference| = {err:.4g} > tol {tol:.4g} over {got.shape[0]} "
                             f"sampled pixels")

    def _label(self):
        """The label the engine captured for the launch just audited (``ConvStats.replay`` was emptied before it)."""
        rep = self.E.ConvStats.replay
        assert len(rep) == 1, f"the engine captured {len(rep)} launches for one call"
        self.E.ConvStats.replay = []
        return rep[0][0]

    def families(self):
        return {fam for _, fam, _, _ in self.rows}

    def worst(self):
        return max((r[3] for r in self.rows), default=0.0)

    # ------------------------------------------------------------------ wrapped entry points
    @contextlib.contextmanager
    def audit(self):
        E = self.E
        orig = dict(conv=E.conv, bottleneck_chain=E.bottleneck_chain, stem_relu_pool_u8=E.stem_relu_pool_u8,
                    stem_relu_pool_f32=E.stem_relu_pool_f32, maxpool3x3s2=E.maxpool3x3s2)
        sig = {k: inspect.signature(f) for k, f in orig.items()}
        prev_replay = E.ConvStats.replay

        def bound(name, args, kw):
            ba = sig[name].bind(*args, **kw)
            ba.apply_defaults()
            return ba.arguments

        def conv(*args, **kw):
            a = bound("conv", args, kw)
            pc, x, out = a["pc"], a["x"], a["out"]
            ops = {k: a[k] for k in ("x", "x2", "res1", "res2")}
            if out is not None:
                ops = {k: (_clone_view(t) if _overlaps(t, out) else t) for k, t in ops.items()}
            E.ConvStats.replay = []
            out = orig["conv"](*args, **kw)
            torch.cuda.synchronize()
            lab = self._label()
            w, b = self._w(pc, out.buf.device)
            oh, ow = out.h, out.w
            mi = self._sample(out.n, oh, ow, out.buf.device)
            ref = ref_conv(w, b, pc.stride, pc.pad, ops["x"], mi, oh, ow, act_slope=a["act_slope"], alpha=a["alpha"],
                           res1=ops["res1"], res1_pre=a["res1_pre"], res2=ops["res2"], alpha2=a["alpha2"], in_up2=a["in_up2"],
                           x2=ops["x2"], x2_stride=a["x2_stride"], band=tuple(a["band"]))
            got = gather_act(out, *split_m(mi, oh, ow))
            self._check(lab, conv_family(lab, pc.precision, x.fmt), got, ref, F32_FACTOR if pc.precision == 0 else 1)
            return out

        def bottleneck_chain(*args, **kw):
            a = bound("bottleneck_chain", args, kw)
            pc2, pc3, pc1n, t1, res, t1b = a["pc2"], a["pc3"], a["pc1n"], a["t1"], a["res"], a["t1b"]
            E.ConvStats.replay = []
            out, t1n = orig["bottleneck_chain"](*args, **kw)
            torch.cuda.synchronize()
            lab = self._label()
            fam = chain_family(lab)
            dev = out.buf.device
            W = {}
            W["w3"], W["b3"] = self._w(pc3, dev)
            if pc2 is not None:
                W["w2"], W["b2"] = self._w(pc2, dev)
            mi = self._sample(out.n, out.h, out.w, dev)
            ni, ho, wo = split_m(mi, out.h, out.w)
            even = ((ho % 2) == 0) & ((wo % 2) == 0)
            ref = ref_chain(W, t1, res, mi, t1b=t1b, t1b_stride=a["t1b_stride"])
            got = gather_act(out, ni, ho, wo)
            if "out@even" in lab:        # FCP_CHAIN_OUT_EVEN_ONLY: the other pixels of `out` are not written
                self._check(lab + " [out]", fam, got[even], ref[even])
            else:
                self._check(lab + " [out]", fam, got, ref)
            if t1n is not None:
                w1, b1 = self._w(pc1n, dev)
                src = torch.where(even[:, None], got, ref) if "out@even" in lab else got     # conv1' of the kernel's own out
                self._check(lab + " [t1n]", fam, gather_act(t1n, ni, ho, wo), ref_1x1_relu(w1, b1, src))
            return out, t1n

        def stem_relu_pool_u8(*args, **kw):
            a = bound("stem_relu_pool_u8", args, kw)
            ps, images, conv1 = a["ps"], a["images_u8"], a["conv1"]
            E.ConvStats.replay = []
            res = orig["stem_relu_pool_u8"](*args, **kw)
            torch.cuda.synchronize()
            lab = self._label()
            out, t1 = (res, None) if conv1 is None else res
            dev = out.buf.device
            w, b = self._w(ps, dev)
            pi = self._sample(out.n, out.h, out.w, dev)
            ni, py, px = split_m(pi, out.h, out.w)
            fam = "stem + conv1" if conv1 is not None else "stem"
            got = gather_act(out, ni, py, px)
            self._check(lab + " [pooled]", fam, got, ref_stem(w, b, images, pi, out.h, out.w, mean=a["mean_rgb"]))
            if conv1 is not None:
                w1, b1 = self._w(conv1, dev)
                self._check(lab + " [t1]", fam, gather_act(t1, ni, py, px), ref_1x1_relu(w1, b1, got))
            return res

        def stem_relu_pool_f32(*args, **kw):
            a = bound("stem_relu_pool_f32", args, kw)
            ps, x4 = a["ps"], a["x4"]
            E.ConvStats.replay = []
            out = orig["stem_relu_pool_f32"](*args, **kw)
            torch.cuda.synchronize()
            lab = self._label()
            w, b = self._w(ps, out.buf.device)
            pi = self._sample(out.n, out.h, out.w, out.buf.device)
            got = gather_act(out, *split_m(pi, out.h, out.w))
            self._check(lab, "stem f32", got, ref_stem(w, b, x4.buf, pi, out.h, out.w))
            return out

        def maxpool3x3s2(*args, **kw):
            a = bound("maxpool3x3s2", args, kw)
            x = a["x"]
            xs = _clone_view(x) if a["out"] is not None and _overlaps(x, a["out"]) else x
            out = orig["maxpool3x3s2"](*args, **kw)
            torch.cuda.synchronize()
            pi = self._sample(out.n, out.h, out.w, out.buf.device)
            got = gather_act(out, *split_m(pi, out.h, out.w))
            self._check(f"maxpool 3x3 s2 @{out.h}x{out.w}", "maxpool", got, ref_maxpool(xs, pi, out.h, out.w), exact=True)
            return out

        E.conv, E.bottleneck_chain, E.stem_relu_pool_u8 = conv, bottleneck_chain, stem_relu_pool_u8
        E.stem_relu_pool_f32, E.maxpool3x3s2 = stem_relu_pool_f32, maxpool3x3s2
        E.ConvStats.replay = []
        try:
            yield self
        finally:
            for k, f in orig.items():
                setattr(E, k, f)
            E.ConvStats.replay = prev_replay
