"""Records tests/golden/jpeg_options.npz: for every case of tests/jpeg_options_ref.py's list (sizes x contents x RGB at the
three chroma subsamplings and gray x standard and optimised Huffman tables x qualities) the file Pillow writes, plus the two
Fibonacci length-limit images' files, the inputs (a checksum of them from 96 x 80 on: they are generated again, seeded)
and the versions of the libraries that wrote them.  The files of the noise content from 96 x 80 on (incompressible, 12 to
36 KB each) are recorded as their length and checksum, which keeps the fixture under 512 KB.  Run from the repository root:
``python tests/golden/make_golden_jpeg_options.py``."""
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
    import jpeg_options_ref as O
    assert features.check_feature("libjpeg_turbo"), "record the fixture with a Pillow built on libjpeg-turbo"
    out = {"versions": np.array([f"Pillow {PIL.__version__}", f"libjpeg-turbo {features.version('jpg')}",
                                 f"numpy {np.__version__}"])}
    for case in O.cases():
        kind, h, w, ch, ss, opt, q = case
        img = O.R.content(kind, h, w, ch)
        key = f"{kind}_{h}x{w}x{ch}"
        if h * w < 96 * 80:
            out["in_" + key] = img
        else:
            out["crc_" + key] = np.array(zlib.crc32(img.tobytes()), np.int64)
        data = O.pillow(img, q, ss, opt)
        if kind == "noise" and h * w >= 96 * 80:
            out["sum_" + O.case_key(case)] = np.array([len(data), zlib.crc32(data)], np.int64)
        else:
            out["jpg_" + O.case_key(case)] = np.frombuffer(data, np.uint8)
    for shift, nsym in ((0, 19), (1, 18)):
        img, _ = O.fibonacci_image(shift, nsym)
        out[f"crc_fibonacci_{shift}_{nsym}"] = np.array(zlib.crc32(img.tobytes()), np.int64)
        out[f"jpg_fibonacci_{shift}_{nsym}"] = np.frombuffer(O.pillow(img, 50, "4:2:0", True), np.uint8)
    path = os.path.join(HERE, "jpeg_options.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(O.cases()), "cases")


if __name__ == "__main__":
    main()
