#!/usr/bin/env python3
"""Writes the scenes of tests/_buildcases.py, and the non-finite scenes the library must
refuse, into one file for csrc/host_build_check (make -C ba_pathtracing_fur_amd/csrc
asan-check): the host builder under AddressSanitizer and UBSan, outside Python.

Per case: name (uint32 length + bytes), expected status (0 KHP_OK, 1 KHP_EINVAL),
n_tris, n_cones (uint32), then tri_v, tri_n (float32), tri_mat (uint32),
cone_base_r0, cone_apex_r1 (float32), cone_mat (uint32)."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
os.environ.setdefault("KHP_NO_BUILD", "1")

import _buildcases as C  # noqa: E402
from test_build_truth import NONFINITE  # noqa: E402


def write(f, name, sd, status):
    nm = name.encode()
    f.write(struct.pack("<I", len(nm)) + nm)
    f.write(struct.pack("<III", status, len(sd.tri_v), len(sd.cone_base_r0)))
    for a, t in ((sd.tri_v, np.float32), (sd.tri_n, np.float32), (sd.tri_mat, np.uint32),
                 (sd.cone_base_r0, np.float32), (sd.cone_apex_r1, np.float32), (sd.cone_mat, np.uint32)):
        f.write(np.ascontiguousarray(a, t).tobytes())


def main(path):
    n = 0
    with open(path, "wb") as f:
        for name, case in list(C.CASES.items()) + [("depth_64", C.DEPTH_64)]:
            write(f, name, case.scene(), 0)
            n += 1
        for name, make, _ in NONFINITE:
            write(f, "nonfinite-" + name, make(), 1)
            n += 1
    print(f"{n} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
