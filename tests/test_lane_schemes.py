"""Index arithmetic of the kernels' lane schemes, restated in numpy and checked against the definition on the CPU (the
kernels themselves are checked bit for bit against the oracle by the GPU tests).

k_fp_q (csrc/dcmt_kernels_fp_q16.h): the 31-wide horizontal maximum with two columns per lane -- exclusive prefix / suffix
scans inside 16-lane DPP rows, the halo columns wrapped onto lanes 0..7 / 56..63 of a second register, two ds_bpermute
addresses -- and the sort of five packed values from three-input minima / maxima and XORs."""
import itertools

import numpy as np

NEUTRAL = 0                         # codes are positive: 0 is the neutral element of their maximum


def _rows(x, fn):
    y = np.empty(64)
    for r in range(0, 64, 16):
        y[r:r + 16] = fn(x[r:r + 16])
    return y


def _prefix(x): return _rows(x, np.maximum.accumulate)
def _suffix(x): return _rows(x, lambda v: np.maximum.accumulate(v[::-1])[::-1])
def _shr1(x): return _rows(x, lambda v: np.concatenate(([NEUTRAL], v[:-1])))     # row_shr:1 with bound_ctrl: the lane without a source reads 0
def _shl1(x): return _rows(x, lambda v: np.concatenate((v[1:], [NEUTRAL])))
def _ror8(x): return _rows(x, lambda v: np.roll(v, -8))


def test_fp_pair_horizontal_31_max_matches_the_definition():
    rng = np.random.default_rng(5)
    lane = np.arange(64)
    for trial in range(300):
        cols = rng.integers(1, 100, size=160)                     # virtual columns gx0-16 .. gx0+143
        if trial % 3 == 0:
            cols[rng.integers(0, 160, size=150)] = 1              # long runs of equal values
        A = cols[16:144]
        E, O = A[0::2].copy(), A[1::2].copy()
        B = rng.integers(1, 100, size=64)                         # dead lanes hold anything
        k = np.arange(8)
        B[k] = cols[144 + 2 * k]; B[8 + k] = cols[144 + 2 * k + 1]          # right halo: even columns, odd columns
        B[56 + k] = cols[2 * k]; B[48 + k] = cols[2 * k + 1]                # left halo (from gx0-16): even, odd
        bo = _ror8(B)
        pa, sa = _prefix(np.maximum(E, O)), _suffix(np.maximum(E, O))
        pb, sb = _prefix(np.maximum(B, bo)), _suffix(np.maximum(B, bo))
        # exclusive scans: which scan a lane hands on is chosen at the SOURCE lane, before the shift (two shifts, not four)
        px, sx = _shr1(np.where(lane < 7, pb, pa)), _shl1(np.where(lane > 56, sb, sa))
        so = np.maximum(np.where(lane >= 56, bo, O), sx)
        pe = np.maximum(np.where(lane < 8, B, E), px)
        m8, p8 = (lane - 8) % 64, (lane + 8) % 64
        dE, dO = np.maximum(so[m8], px[p8]), np.maximum(sx[m8], pe[p8])
        for l in range(64):
            c = 16 + 2 * l
            assert dE[l] == cols[c - 15:c + 16].max(), (trial, l)
            assert dO[l] == cols[c - 14:c + 17].max(), (trial, l)


def test_sort5_from_three_input_minima_maxima_and_xors():
    """q_sort5 (csrc/dcmt_kernels_fp_q16.h): sort3 of three values as min3 / max3 / XOR, sort2 of the other two, the merge of 3 + 2 by
    rank, the middle one as the XOR of all five and the other four.  Exhaustive on five values of five levels (every tie pattern)."""
    def sort5x(v):
        v0, v1, v2, v3, v4 = v
        a, c, t = min(v0, v1, v2), max(v0, v1, v2), v0 ^ v1 ^ v2
        b = t ^ a ^ c
        d, e = min(v3, v4), max(v3, v4)
        s0, s4 = min(a, d), max(c, e)
        s1, s3 = min(max(a, d), b, e), max(min(c, e), b, d)
        return [s0, s1, (t ^ v3 ^ v4) ^ (s0 ^ s1 ^ s3) ^ s4, s3, s4]
    for v in itertools.product((3, 1029, 7000, 7001, 31743), repeat=5):
        assert sort5x(v) == sorted(v), v
