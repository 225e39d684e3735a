"""The float32 warpAffine family's plumbing, without a GPU: the C export, the registered op, and the family selector."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_float_warp():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    decl = re.search(r"int fcp_warp_affine_u8_float\(([^)]*)\)", hdr)
    fixed = re.search(r"int fcp_warp_affine_u8\(([^)]*)\)", hdr)
    assert decl and fixed
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(decl.group(1)) == norm(fixed.group(1))                  # exactly the fixed family's parameter list
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "fcp_warp_affine_u8_float")
    assert N.SIGNATURES["fcp_warp_affine_u8_float"] == N.SIGNATURES["fcp_warp_affine_u8"]


def test_float_warp_op_is_registered_and_refuses_cpu_tensors():
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "warp_affine_u8_float" in T.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::warp_affine_u8_float", "CUDA")
    schema = str(torch.ops.fcp.warp_affine_u8_float.default._schema)
    assert schema.split("(", 1)[1] == str(torch.ops.fcp.warp_affine_u8.default._schema).split("(", 1)[1]
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.warp_affine_u8_float(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                                 torch.zeros(1, 2, 3, dtype=torch.float64), None, None, 4, 4, 0)


def test_resolve_precedence(monkeypatch):
    from face_crop_plus_amd import align
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    assert align.resolve_warp_family(None, "constant") == "fixed"
    monkeypatch.setenv("FCP_WARP_FAMILY", "float32")
    assert align.resolve_warp_family(None, "constant") == "float32"
    assert align.resolve_warp_family("fixed", "constant") == "fixed"          # the keyword wins over the environment
    monkeypatch.setenv("FCP_WARP_FAMILY", "fixed")
    assert align.resolve_warp_family("float32", 0) == "float32"
    monkeypatch.setenv("FCP_WARP_FAMILY", "")
    assert align.resolve_warp_family(None, 0) == "fixed"


@pytest.mark.parametrize("bad", ["float", "FIXED", "float64", 1])
def test_resolve_rejects_unknown_families(bad, monkeypatch):
    from face_crop_plus_amd import align
    with pytest.raises(ValueError, match="fixed.*float32.*auto"):
        align.resolve_warp_family(bad, 0)
    monkeypatch.setenv("FCP_WARP_FAMILY", str(bad))
    with pytest.raises(ValueError, match="fixed.*float32"):
        align.resolve_warp_family(None, 0)


def test_warp_and_crop_reject_unknown_families():
    from face_crop_plus_amd import align
    with pytest.raises(ValueError, match="fixed.*float32"):
        align.warp_affine(None, None, None, None, None, (4, 4), 0, family="auto")
    with pytest.raises(ValueError, match="fixed.*float32"):
        align.crop_align(None, None, None, None, (4, 4), family="float")


@pytest.mark.parametrize("how", ["keyword", "environment"])
def test_auto_without_cv2_is_fixed_and_never_touches_the_gpu(how, monkeypatch):
    from face_crop_plus_amd import align
    monkeypatch.setitem(sys.modules, "cv2", None)                   # `import cv2` raises ImportError

    def no_gpu(*a, **k):
        raise AssertionError("the auto probe ran without cv2")
    monkeypatch.setattr(align, "warp_affine", no_gpu)
    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    if how == "environment":
        monkeypatch.setenv("FCP_WARP_FAMILY", "auto")
        assert align.resolve_warp_family(None, "reflect") == "fixed"
    else:
        monkeypatch.setenv("FCP_WARP_FAMILY", "float32")
        assert align.resolve_warp_family("auto", "reflect") == "fixed"
