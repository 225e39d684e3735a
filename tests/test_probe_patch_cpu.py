"""Retired experiments stay retired: no experiment switch in the product kernels, no retired A/B variable read by the
product modules.  The experiments themselves are recorded in profiles/*.md."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "face-crop-plus_amd")

# A/B switches whose losing paths were deleted; the shipped behaviour is what their defaults selected
RETIRED_VARIABLES = ("FCP_BIG_TILES", "FCP_BALANCE_TAIL", "FCP_HALO_WIDE", "FCP_CHAIN_TILE_M", "FCP_CHAIN_PATCH",
                     "FCP_CHAIN_SPARSE_OUT", "FCP_CHAIN_TWO_SOURCE", "FCP_L3_FORM", "FCP_FUSED_STEM", "FCP_FUSED_STEM_CONV1",
                     "FCP_FUSED_CHAIN", "FCP_SPLIT_CU_BUDGET", "FCP_BISE_FUSED_STEM", "FCP_RRDB_BAND", "FCP_BUILD_DEFINES",
                     "FCP_BUILD_FLAGS")


def test_product_kernels_carry_no_experiment_switches():
    bad = []
    csrc = os.path.join(PKG, "csrc")
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            for i, line in enumerate(open(os.path.join(csrc, name)), 1):
                if re.search(r"FCP_\w*(ABLATE|PROBE|_ROT\b|REG_EPI|STAGES3|BURST\)|SPREAD\)|PROFILING|STEM_PW|WIDE2_BT)", line) \
                        and line.lstrip().startswith("#"):
                    bad.append(f"{name}:{i}: {line.strip()}")
    # ... and none spelt as a constant either: `constexpr bool ROT = false;` kept a whole retired loop behind `if constexpr`
    for folder, _, names in os.walk(csrc):
        for name in names:
            if name.endswith((".hip", ".h", ".cpp")):
                for i, line in enumerate(open(os.path.join(folder, name)), 1):
                    if re.search(r"constexpr bool \w+ = (false|true);", line):
                        bad.append(f"{name}:{i}: {line.strip()}")
    assert not bad, bad


def test_product_modules_read_no_retired_variable():
    pattern = re.compile(r"\b(" + "|".join(RETIRED_VARIABLES) + r")\b")
    bad = []
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            for i, line in enumerate(open(os.path.join(PKG, name)), 1):
                if pattern.search(line):
                    bad.append(f"{name}:{i}: {line.strip()}")
    assert not bad, bad
