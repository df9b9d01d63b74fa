#!/usr/bin/env python3
"""Extract the reference's ORB sampling pattern, bit_pattern_31_2 (include/opencv/CvORB.h of its tree), into a data fixture.

    python tools/make_orb_fixtures.py REFERENCE_TREE

REFERENCE_TREE is the root of the reference's checkout (the directory that holds src/slam). Output:
tests/golden/orb_pattern.npz with `pattern` (512 x 2 int32: the points (x, y), pairs of consecutive points compared) and
tests/golden/orb_pattern.sha256 (sha256 of that array's bytes). The table is data; it is kept under tests/golden/ only, and the
library takes the pattern as an argument.
"""
import hashlib
import pathlib
import re
import sys

import numpy as np

OUT = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden"


def extract(header_text):
    m = re.search(r"bit_pattern_31_2\s*\[[^\]]*\]\s*=\s*\{(.*?)\};", header_text, re.S)
    if not m:
        raise SystemExit("bit_pattern_31_2 not found")
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    vals = [int(t) for t in re.findall(r"-?\d+", body)]
    if len(vals) != 1024:
        raise SystemExit(f"expected 1024 values, found {len(vals)}")
    return np.array(vals, dtype=np.int32).reshape(512, 2)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    hdr = pathlib.Path(sys.argv[1]) / "src" / "slam" / "include" / "opencv" / "CvORB.h"
    pat = extract(hdr.read_text())
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "orb_pattern.npz", pattern=pat)
    (OUT / "orb_pattern.sha256").write_text(hashlib.sha256(pat.tobytes()).hexdigest() + "  pattern\n")
    print("wrote", OUT / "orb_pattern.npz", "range", int(pat.min()), int(pat.max()))


if __name__ == "__main__":
    main()
