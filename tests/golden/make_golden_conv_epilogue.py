"""Record tests/golden/conv_epilogue_bits.json: the sha256 of every case of tests/conv_epilogue_cases.py.

    python tests/golden/make_golden_conv_epilogue.py [output.json]

Run on an MI355X with the library built from the commit whose bits are the reference (the fixture in the repository was
recorded at the parent of the commit that introduced the shared epilogue helpers, and again, with the walk cases added and the
older hashes reproduced, at the parent of the commit that introduced the shared im2col walk, and once more, with the halo walk
cases added, at the parent of the commit that gathered the halo kernels' shared pieces).  A case whose tile choices disagree is an
error here too: the hash would depend on the tile.  A later change of the K order (or of the epilogue's arithmetic) that is
meant to change bits regenerates the file with this script.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import conv_epilogue_cases as CE  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_epilogue_bits.json")
    device = torch.device("cuda:0")
    hashes = {}
    for case_id, kind, spec in CE.cases():
        outs, _ = CE.run_case(case_id, kind, spec, device)
        first = next(iter(outs.values()))
        for label, bufs in outs.items():
            assert all(torch.equal(a, b) for a, b in zip(first, bufs)), f"{case_id}: tile {label} differs"
        hashes[case_id] = CE.digest(first)
        print(case_id, hashes[case_id][:16], flush=True)
    with open(dst, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "hashes": hashes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(hashes)} cases -> {dst}")


if __name__ == "__main__":
    main()
