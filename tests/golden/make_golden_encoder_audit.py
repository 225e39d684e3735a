"""Records tests/golden/encoder_audit.npz: for every face of tests/encoder_audit_cases.py's JPEG groups (the default
output size and above, 1024 x 1024, the extreme aspect ratios; every mode, standard and optimised tables, quality 90) the
length and the CRC-32 of the file Pillow writes, a checksum of the input (the inputs are generated again, seeded), and the
versions of the libraries that wrote them.  Run from the repository root:
``python tests/golden/make_golden_encoder_audit.py``."""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import PIL
    from PIL import features
    import encoder_audit_cases as C
    assert features.check_feature("libjpeg_turbo"), "record the fixture with a Pillow built on libjpeg-turbo"
    out = {"versions": np.array([f"Pillow {PIL.__version__}", f"libjpeg-turbo {features.version('jpg')}",
                                 f"numpy {np.__version__}"])}
    for name, h, w, ch, ss, opt, _ in C.jpeg_groups():
        kinds, imgs = C.jpeg_faces(h, w, ch)
        for kind, img in zip(kinds, imgs):
            out[f"crc_{kind}_{h}x{w}x{ch}"] = np.array(zlib.crc32(img.tobytes()), np.int64)
            data = C.O.pillow(img, C.QUALITY, ss, opt)
            out[C.fixture_key(name, kind)] = np.array([len(data), zlib.crc32(data)], np.int64)
    path = os.path.join(HERE, "encoder_audit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(C.jpeg_groups()), "groups")


if __name__ == "__main__":
    main()
