#!/usr/bin/env python3
"""The two lookup tables and nine coefficients of the 8-bit BGR -> Lab conversion (dcmt_bgr_convert*), as the
header the library compiles: depth_completion_mt_amd/csrc/dcmt_lab_tables.h.

    python tools/make_lab_tables.py            prints the two sha256 (tables as little-endian uint16)
    python tools/make_lab_tables.py --write    rewrites the header as well

numpy only.  Everything is computed in f64; no entry lies closer than 4.7e-6 of a unit to a rounding tie and no coefficient closer
than 0.029, so any f64 pow gives the same integers."""
import hashlib
import os
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "depth_completion_mt_amd", "csrc", "dcmt_lab_tables.h")

GAMMA_ONE = 2040                 # gamma[255]: linear light 1.0
CBRT_N = 3072                    # cbrt's entries; index GAMMA_ONE is t = 1.0
CBRT_ONE = 32768                 # cbrt[GAMMA_ONE]: f(1.0)
COEF_SHIFT = 12
M = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))     # sRGB -> XYZ, D65
W = (0.950456, 1.0, 1.088754)                                                                             # the white point


def gamma_table() -> np.ndarray:
    v = np.arange(256, dtype=np.float64) / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    return np.floor(GAMMA_ONE * lin + 0.5).astype(np.uint16)


def cbrt_table() -> np.ndarray:
    t = np.arange(CBRT_N, dtype=np.float64) / GAMMA_ONE
    f = np.where(t < 0.008856, 7.787 * t + 16.0 / 116.0, t ** (1.0 / 3.0))
    return np.floor(CBRT_ONE * f + 0.5).astype(np.uint16)


def coefficients() -> np.ndarray:
    m, w = np.array(M, dtype=np.float64), np.array(W, dtype=np.float64)
    return np.rint((1 << COEF_SHIFT) * m / w[:, None]).astype(np.int32)         # [row of XYZ][R, G, B]


def sha256_le16(table: np.ndarray) -> str:
    return hashlib.sha256(table.astype("<u2").tobytes()).hexdigest()


def _initialiser(name: str, table: np.ndarray, per_line: int) -> str:
    rows = [", ".join(str(int(x)) for x in table[i:i + per_line]) for i in range(0, len(table), per_line)]
    return f"#define {name} \\\n    " + ", \\\n    ".join(rows) + "\n"


def render() -> str:
    g, c, k = gamma_table(), cbrt_table(), coefficients().reshape(-1)
    return (
        "// dcmt_lab_tables.h -- the constants of the 8-bit BGR -> Lab conversion (dcmt_kernels_bgr.h; DESIGN section 15).  Written by\n"
        "// tools/make_lab_tables.py: change that, not this.  No HIP, nothing but initialiser lists.\n"
        "//   DCMT_LAB_GAMMA  [256]   uint16  floor(2040 * lin(i / 255) + 0.5), the sRGB curve\n"
        "//   DCMT_LAB_CBRT   [3072]  uint16  floor(32768 * f(i / 2040) + 0.5), f = the CIE cube root with its linear toe\n"
        "//   DCMT_LAB_COEF   [9]     int32   rint(4096 * M[r][c] / W[r]), rows X, Y, Z over columns R, G, B; every row sums to 4096\n"
        f"// sha256 (little-endian uint16): gamma {sha256_le16(g)}\n"
        f"//                                cbrt  {sha256_le16(c)}\n"
        "#pragma once\n\n"
        + _initialiser("DCMT_LAB_GAMMA", g, 16) + "\n" + _initialiser("DCMT_LAB_CBRT", c, 16) + "\n" + _initialiser("DCMT_LAB_COEF", k, 9))


def main(argv) -> int:
    print("gamma", sha256_le16(gamma_table()))
    print("cbrt ", sha256_le16(cbrt_table()))
    if "--write" in argv:
        with open(HEADER, "w") as f:
            f.write(render())
        print("wrote", os.path.normpath(HEADER))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
