"""The device shuffle's core (gym_xarm_amd/csrc/xarm_rollout_core.h) on the CPU: the g++ build (tests/rollout_host.py) - every row is a
permutation, rows differ between epochs, counters and seeds, the (element, position) counts are uniform - and the argument checks of
the C-ABI entry point through the real library (no device needed)."""
import ctypes as C

import numpy as np
import pytest

import rollout_host as RH

CALLS = (0, (1 << 32) + 5)          # the counter's low and high word both key the draw
# the 0.999 quantile of chi-square at (N - 1)^2 degrees of freedom, by Wilson-Hilferty: k (1 - 2 / (9 k) + 3.0902 sqrt(2 / (9 k)))^3
CHI2_LIMIT = {5: 39.4, 8: 85.4, 13: 202.2, 100: 10239.4}


def test_the_limits_are_the_wilson_hilferty_quantiles():
    for n, limit in CHI2_LIMIT.items():
        k = float((n - 1) ** 2)
        assert abs(k * (1.0 - 2.0 / (9.0 * k) + 3.0902 * (2.0 / (9.0 * k)) ** 0.5) ** 3 - limit) < 0.06


def test_domain_bits_have_a_floor_of_eight():
    L = RH.lib()
    assert [L.rh_perm_bits(n) for n in (1, 2, 5, 256, 257, 1000, 81925, (1 << 31) - 1)] == [8, 8, 8, 8, 9, 10, 17, 31]
    assert L.rh_perm_bits(1 << 31) == -1 and L.rh_perm_bits(-1) == -1


@pytest.mark.parametrize("N", RH.PERM_SIZES)
def test_every_row_is_a_permutation(N):
    want = np.arange(N, dtype=np.int32)
    rows = {}
    for calls in CALLS:
        for seed in (0, 7):
            perm, after = RH.perm_fill(3, N, seed, calls)
            assert after == calls + 1
            for ep in range(3):
                assert np.array_equal(np.sort(perm[ep]), want), (N, calls, seed, ep)
            rows[(calls, seed)] = perm
    if N == 1:
        assert all((p == 0).all() for p in rows.values())
    if N >= 64:
        p = rows[(0, 0)]
        assert not np.array_equal(p[0], p[1]) and not np.array_equal(p[1], p[2]) and not np.array_equal(p[0], p[2])
        assert not np.array_equal(p, rows[(CALLS[1], 0)]) and not np.array_equal(p, rows[(0, 7)])
        assert not np.array_equal(p[0], want)
    again, _ = RH.perm_fill(3, N, 7, CALLS[1])
    assert np.array_equal(again, rows[(CALLS[1], 7)])          # a function of (seed, calls, epoch, i) alone


@pytest.mark.parametrize("N,draws", ((5, 4096), (8, 4096), (13, 4096), (100, 8192)))
def test_shuffle_is_uniform_over_element_and_position(N, draws):
    """seed 0; draw c is row c & 3 of a 4-epoch fill with calls = c >> 2.  The N x N table of (element, position) counts against
    draws / N, chi-square below the 0.999 quantile at (N - 1)^2 degrees of freedom (the table's rows and columns each sum to
    `draws`).  The limits are derived, not measured; a failing case means the cipher is wrong."""
    counts = np.zeros((N, N), np.int64)
    pos = np.arange(N)
    for c in range(draws // 4):
        perm, _ = RH.perm_fill(4, N, 0, c)
        for ep in range(4):
            counts[perm[ep], pos] += 1
    assert counts.sum() == draws * N
    expect = draws / N
    chi2 = float((((counts - expect) ** 2) / expect).sum())
    print("N %d draws %d chi2 %.1f limit %.1f" % (N, draws, chi2, CHI2_LIMIT[N]))
    assert chi2 < CHI2_LIMIT[N]


def test_entry_point_checks_its_arguments():
    """through libxarm_hip.so; every refused call returns before it touches a device"""
    from gym_xarm_amd import _native
    L = _native.load()
    x = C.c_void_p(256)             # never dereferenced
    assert L.xarm_perm_fill(x, 0, 10, 0, x, None) == -1 and b"n_epochs" in L.xarm_last_error(None)
    assert L.xarm_perm_fill(x, 256, 10, 0, x, None) == -1
    assert L.xarm_perm_fill(x, 1, 1 << 31, 0, x, None) == -1 and b"N must" in L.xarm_last_error(None)
    assert L.xarm_perm_fill(x, 1, -1, 0, x, None) == -1
    assert L.xarm_perm_fill(None, 1, 10, 0, x, None) == -1 and L.xarm_perm_fill(x, 1, 10, 0, None, None) == -1
    assert L.xarm_perm_fill(None, 1, 0, 0, None, None) == 0
