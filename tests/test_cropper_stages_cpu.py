"""The Cropper's host side without a GPU: option defaults stated on the class, the stages ``_process_images`` drives, the
constructor's shared checks."""
import contextlib
import os

import numpy as np
import pytest
import torch

OFF = {None: ("background", "background_blur", "background_image", "background_fit", "blur_taps", "decontaminate",
              "decontaminate_taps", "refine", "refine_eps", "subject", "fill_holes", "edge_shift", "denoise", "clahe",
              "clahe_grid", "sharpen", "sharpen_sigma", "sharpen_threshold", "min_sharpness", "jpeg", "io_ring_mb", "_io",
              "_io_procs", "_io_procs_active", "_rows_cache", "_pictures_dev"),
       "host": ("png_encoder", "encoder"),
       0: ("foreground_bits",)}


def test_a_bare_cropper_reads_every_option_as_off():
    from face_crop_plus_amd import Cropper
    c = Cropper.__new__(Cropper)
    assert vars(c) == {}
    for value, names in OFF.items():
        for name in names:
            got = getattr(c, name)
            assert got is value if value is None else got == value and type(got) is type(value), name
    assert c._has_background() is False and c._encodes_on_device() is False and c._jpeg_kw() == {}


@pytest.fixture
def chain(monkeypatch):
    """A bare Cropper whose finishing steps are recorders: (calls, cropper).  A call is (step, open ranges, arguments)."""
    from face_crop_plus_amd import cropper as CR
    calls, open_ranges = [], []

    @contextlib.contextmanager
    def span(name):
        open_ranges.append(name)
        try:
            yield
        finally:
            open_ranges.pop()

    def recorder(step, result):
        return lambda *a, **k: calls.append((step, tuple(open_ranges), a, k)) or result
    monkeypatch.setattr(CR.trace, "range", span)
    monkeypatch.setattr(CR.denoising, "denoise", recorder("denoise", "denoised"))
    monkeypatch.setattr(CR.equalizing, "clahe", recorder("clahe", "equalised"))
    monkeypatch.setattr(CR.sharpening, "sharpen", recorder("sharpen", "sharpened"))
    monkeypatch.setattr(CR.Cropper, "_matte_device", lambda self, *a, **k: recorder("matte", ("matted", None))(*a, **k))
    monkeypatch.setattr(CR.matting, "pick_pictures", recorder("pick", "picks"))
    c = CR.Cropper.__new__(CR.Cropper)
    c.strategy, c.output_format = "largest", "png"
    return calls, c


NAMES = np.array(["x.jpg", "y.jpg"])


def test_the_finishing_chain_runs_every_step_in_order_on_the_previous_output(chain):
    calls, c = chain
    c.denoise, c.clahe, c.clahe_grid, c.sharpen, c.sharpen_sigma, c.sharpen_threshold = 8.0, 2.0, 8, 1.0, 1.5, 0
    c.background = (1, 2, 3)
    assert c._finish_crops("crops", "labels", NAMES, "out") == "matted"
    assert calls == [("denoise", ("fcp:denoise",), ("crops", 8.0), {}),
                     ("clahe", ("fcp:clahe",), ("denoised", 2.0, 8), {}),
                     ("sharpen", ("fcp:sharpen",), ("equalised", 1.0, 1.5, 0), {}),
                     ("matte", ("fcp:matte",), ("sharpened", "labels"), {})]


def test_the_picks_come_from_the_target_paths_exactly_with_background_image(chain):
    calls, c = chain
    c.background_image = np.zeros((2, 4, 4, 3), np.uint8)
    assert c._finish_crops("crops", "labels", NAMES, "out") == "matted"
    paths = c._target_paths(NAMES, "out")
    assert paths == [os.path.join("out", "x.png"), os.path.join("out", "y.png")]
    assert calls == [("pick", ("fcp:matte",), (paths, 2), {}),
                     ("matte", ("fcp:matte",), ("crops", "labels"), {"picks": "picks"})]
    del calls[:]
    c.background_image, c.background_blur = None, 3.0
    c._finish_crops("crops", "labels", NAMES, "out")
    assert calls == [("matte", ("fcp:matte",), ("crops", "labels"), {})]


@pytest.mark.parametrize("on", ["denoise", "clahe", "sharpen", "labels", None])
def test_a_step_of_the_chain_runs_only_when_its_option_is_set(chain, on):
    calls, c = chain
    if on not in ("labels", None):
        setattr(c, on, 2.0)
    crops = object()
    got = c._finish_crops(crops, "labels" if on == "labels" else None, NAMES, "out")
    assert [call[0] for call in calls] == ([] if on is None else ["matte" if on == "labels" else on])
    assert all(call[2][0] is crops for call in calls)
    if on is None:
        assert got is crops                       # nothing set, no labels: the input itself, nothing launched


def test_keep_filters_faces_device_faces_and_indices_together():
    from face_crop_plus_amd import Cropper
    keep = np.array([True, False, True])
    faces = np.arange(3 * 2 * 2 * 3, dtype=np.uint8).reshape(3, 2, 2, 3)
    faces_dev = torch.from_numpy(faces.copy())
    got, got_dev, indices = Cropper.__new__(Cropper)._keep(keep, faces, faces_dev, [4, 4, 7])
    assert np.array_equal(got, faces[[0, 2]]) and torch.equal(got_dev, faces_dev[[0, 2]]) and indices == [4, 7]
    got, got_dev, indices = Cropper.__new__(Cropper)._keep(keep, None, faces_dev, [9, 2, 1])
    assert got is None and torch.equal(got_dev, faces_dev[[0, 2]]) and indices == [9, 1] and type(indices) is list


# the texts the constructor raised when each option carried its own copy of the check, recorded from it
NEEDS_ALIGNED = {
    "min_sharpness": (5.0, "min_sharpness needs aligned crops: it cannot be combined with det_threshold=None and "
                           "landmarks=None (no alignment), where the faces are the images themselves"),
    "background": (0, "background / background_blur need aligned crops: they cannot be combined with det_threshold=None and "
                      "landmarks=None (no alignment), where the faces are the images themselves"),
    "background_blur": (3.0, "background / background_blur need aligned crops: they cannot be combined with "
                             "det_threshold=None and landmarks=None (no alignment), where the faces are the images themselves"),
    "background_image": (np.zeros((8, 8, 3), np.uint8),
                         "background_image needs aligned crops: it cannot be combined with det_threshold=None and "
                         "landmarks=None (no alignment), where the faces are the images themselves"),
    "clahe": (2.0, "clahe needs aligned crops: it cannot be combined with det_threshold=None and landmarks=None (no "
                   "alignment), where the faces are the images themselves"),
    "denoise": (8, "denoise needs aligned crops: it cannot be combined with det_threshold=None and landmarks=None (no "
                   "alignment), where the faces are the images themselves"),
    "sharpen": (1.0, "sharpen needs aligned crops: it cannot be combined with det_threshold=None and landmarks=None (no "
                     "alignment), where the faces are the images themselves"),
}


@pytest.mark.parametrize("option", sorted(NEEDS_ALIGNED))
def test_the_aligned_crops_messages_are_the_old_ones(monkeypatch, option):
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    value, text = NEEDS_ALIGNED[option]
    with pytest.raises(ValueError) as err:
        CR.Cropper(det_threshold=None, landmarks=None, **{option: value})
    assert str(err.value) == text


def test_pair():
    from face_crop_plus_amd.cropper import _pair
    assert [_pair(v) for v in (7, np.int64(7), [7], (7, 9), [7, 9])] == [(7, 7), (7, 7), (7, 7), (7, 9), (7, 9)]
    assert all(type(_pair(v)) is tuple for v in (7, np.int64(7), [7], (7, 9), [7, 9]))


def test_a_numpy_integer_size_makes_a_cropper(monkeypatch):
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = CR.Cropper(output_size=np.int64(64), resize_size=np.int64(160))
    assert c.output_size == (64, 64) and c.resize_size == (160, 160)
    assert CR.Cropper(output_size=[64, 48]).output_size == (64, 48)


def test_no_option_is_read_through_an_absent_attribute_guard():
    from face_crop_plus_amd import cropper as CR
    with open(CR.__file__, encoding="utf-8") as fh:
        assert "getattr(self" not in fh.read()
