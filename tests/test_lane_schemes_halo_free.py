"""k_fp_q's horizontal 31-maximum on a row whose holes all lie in lanes 8..55 (csrc/dcmt_kernels_fp_q16.h, fill_step): the scans of
the halo register B are left out there.  Restated in numpy in the manner of tests/test_lane_schemes.py: with everything derived
from B -- its two scans, its rotated copy, B itself where a halo lane closes its prefix -- replaced by arbitrary words, the fill
values of lanes 8..55 are the definition's.  (Lanes 0..7 and 56..63 are then anything: a fill value is looked at only in a hole
lane, and the kernel takes this path only when none of those sixteen lanes has a hole.)"""
import numpy as np

from test_lane_schemes import _prefix, _ror8, _shl1, _shr1, _suffix

HALO_LANES = 0xFF000000000000FF          # the wave-uniform test of fill_step: (vme | vmo) & HALO_LANES


def _columns(rng, trial):
    cols = rng.integers(1, 100, size=160)                         # virtual columns gx0-16 .. gx0+143
    if trial % 3 == 0:
        cols[rng.integers(0, 160, size=150)] = 1                  # long runs of equal values
    return cols


def _halo_register(rng, cols):
    B = rng.integers(1, 100, size=64)                             # dead lanes hold anything
    k = np.arange(8)
    B[k] = cols[144 + 2 * k]; B[8 + k] = cols[144 + 2 * k + 1]    # right halo: even columns, odd columns
    B[56 + k] = cols[2 * k]; B[48 + k] = cols[2 * k + 1]          # left halo (from gx0-16): even, odd
    return B


def _fill_values(E, O, B, bo, pb, sb, halo):
    """fill_step's hole path as the kernel has it: A's scans always, the words of B only where `halo`."""
    lane = np.arange(64)
    pp, ss = _prefix(np.maximum(E, O)), _suffix(np.maximum(E, O))
    ee, oo = E.copy(), O.copy()
    if halo:
        pp = np.where(lane < 7, pb, pp)
        ss = np.where(lane > 56, sb, ss)
        oo = np.where(lane >= 56, bo, oo)
        ee = np.where(lane < 8, B, ee)
    px, sx = _shr1(pp), _shl1(ss)
    so, pe = np.maximum(oo, sx), np.maximum(ee, px)
    m8, p8 = (lane - 8) % 64, (lane + 8) % 64
    return np.maximum(so[m8], px[p8]), np.maximum(sx[m8], pe[p8])


def test_lanes_8_to_55_do_not_look_at_the_halo_register():
    rng = np.random.default_rng(11)
    for trial in range(300):
        cols = _columns(rng, trial)
        A = cols[16:144]
        E, O = A[0::2].copy(), A[1::2].copy()
        B = _halo_register(rng, cols)
        # the A-only path, and the full path handed garbage for every word that comes from B
        junk = [rng.integers(0, 1 << 16, size=64) for _ in range(4)]
        for dE, dO in (_fill_values(E, O, None, None, None, None, halo=False), _fill_values(E, O, *junk, halo=True)):
            for l in range(8, 56):
                c = 16 + 2 * l
                assert dE[l] == cols[c - 15:c + 16].max(), (trial, l)
                assert dO[l] == cols[c - 14:c + 17].max(), (trial, l)


def test_the_split_form_with_the_halo_register_is_the_definition_in_every_lane():
    """The rewritten selects (the halo lanes overwrite A's words instead of choosing between two) against the definition, all 64 lanes."""
    rng = np.random.default_rng(12)
    for trial in range(300):
        cols = _columns(rng, trial)
        A = cols[16:144]
        E, O = A[0::2].copy(), A[1::2].copy()
        B = _halo_register(rng, cols)
        bo = _ror8(B)
        dE, dO = _fill_values(E, O, B, bo, _prefix(np.maximum(B, bo)), _suffix(np.maximum(B, bo)), halo=True)
        for l in range(64):
            c = 16 + 2 * l
            assert dE[l] == cols[c - 15:c + 16].max(), (trial, l)
            assert dO[l] == cols[c - 14:c + 17].max(), (trial, l)


def test_the_wave_uniform_test_names_exactly_the_halo_lanes():
    """Hole ballots with bits only in lanes 8..55 take the A-only path, any bit in lanes 0..7 or 56..63 the full one."""
    for l in range(64):
        assert bool((1 << l) & HALO_LANES) == (l < 8 or l >= 56), l
