"""Records tests/golden/jpeg_streams.npz: for every case of tests/jpeg_ref.py's list the input pixels (a checksum of them for the 256 x 256 cases) and the file
Pillow writes for them with the project's JPEG settings (``_io_codec._ENCODER_KW``: quality 95, 4:2:0), plus the versions
of the libraries that wrote them.  Run from the repository root: ``python tests/golden/make_golden_jpeg.py``."""
import io
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import PIL
    from PIL import Image, features
    import jpeg_ref as R
    from face_crop_plus_amd._io_codec import _ENCODER_KW
    kw = _ENCODER_KW[".jpg"]
    assert features.check_feature("libjpeg_turbo"), "record the fixture with a Pillow built on libjpeg-turbo"
    out = {"versions": np.array([f"Pillow {PIL.__version__}", f"libjpeg-turbo {features.version('jpg')}",
                                 f"numpy {np.__version__}", f"settings {sorted(kw.items())}"])}
    for kind, h, w, ch in R.cases():
        img = R.content(kind, h, w, ch)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, **kw)
        key = f"{kind}_{h}x{w}x{ch}"
        if h * w < 256 * 256:
            out["in_" + key] = img
        else:                                   # the one large input is generated again (seeded); its checksum pins it
            out["crc_" + key] = np.array(zlib.crc32(img.tobytes()), np.int64)
        out["jpg_" + key] = np.frombuffer(buf.getvalue(), np.uint8)
    path = os.path.join(HERE, "jpeg_streams.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(R.cases()), "cases")


if __name__ == "__main__":
    main()
