"""CPU: the rule that hands the texture backward's 32-sample halves to workgroups and waves
(csrc/tex_partition.h, one source for the kernel and for the host entry point dsu_texture_live_partition):
every half exactly once and in order, live halves per workgroup and per wave equal up to one."""
import numpy as np
import pytest

from drawingspinup_amd import _lib, ops

WAVES = 4


def _words(half_live):
    words = np.zeros((len(half_live) + 31) // 32, dtype=np.uint32)
    for k in np.nonzero(half_live)[0]:
        words[k >> 5] |= np.uint32(1) << np.uint32(k & 31)
    return words


def _check(half_live, parts, words=None):
    halves = len(half_live)
    runs = ops.texture_live_partition(_words(half_live) if words is None else words, halves, parts, WAVES)
    flat = runs.reshape(-1, 2)
    # in order, nothing skipped, nothing twice
    assert flat[0, 0] == 0 and flat[-1, 1] == halves
    assert np.array_equal(flat[1:, 0], flat[:-1, 1])
    assert (flat[:, 1] >= flat[:, 0]).all()
    csum = np.concatenate([[0], np.cumsum(half_live)])
    per_wave = (csum[flat[:, 1]] - csum[flat[:, 0]]).reshape(parts, WAVES)
    per_part = per_wave.sum(1)
    assert per_part.sum() == half_live.sum()
    assert per_part.max() - per_part.min() <= 1, (halves, parts, per_part)
    assert (per_wave.max(1) - per_wave.min(1) <= 1).all(), (halves, parts)
    return runs


def _bitmaps():
    rng = np.random.default_rng(5)
    out = []
    for halves in (1, 2, 31, 32, 33, 129, 1000, 8192):
        out.append(np.zeros(halves, dtype=bool))                       # all dead
        out.append(np.ones(halves, dtype=bool))                        # all live
        for pos in sorted({0, halves // 2, halves - 1}):               # a single live half
            one = np.zeros(halves, dtype=bool)
            one[pos] = True
            out.append(one)
        for p in (0.05, 0.5, 0.9):
            out.append(rng.random(halves) < p)
        runs = np.repeat(rng.random(halves // 7 + 1) < 0.4, 7)[:halves]   # whole rays dead or live
        out.append(runs)
    return out


def test_every_half_once_and_live_halves_even_for_every_grid():
    maps = [(m, _words(m)) for m in _bitmaps()]
    for parts in range(1, 513):
        for m, words in (maps if parts in (1, 2, 3, 7, 192, 256, 511, 512) else maps[parts % 5::5]):
            _check(m, parts, words)


def test_dead_stretches_stay_with_the_neighbouring_live_half_and_dead_runs_are_cut_evenly():
    m = np.zeros(64, dtype=bool)
    m[[10, 50]] = True
    runs = _check(m, 2).reshape(-1, 2)
    # workgroup 0: the dead prefix and live half 10 up to (not including) live half 50
    assert runs[0, 0] == 0 and runs[WAVES - 1, 1] == 50 and runs[-1, 1] == 64
    runs = _check(np.zeros(64, dtype=bool), 4)
    assert np.array_equal(runs[:, 0, 0], [0, 16, 32, 48])
    assert np.array_equal(runs[0, :, 1], [4, 8, 12, 16])


def test_stale_bits_beyond_the_last_half_are_nobodys():
    words = np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    runs = ops.texture_live_partition(words, 40, 3, WAVES).reshape(-1, 2)
    assert runs[-1, 1] == 40 and runs.max() == 40


def test_argument_checks():
    lib = _lib.lib()
    assert lib.dsu_texture_live_partition(None, 8, 1, 4, None) == -1
    words = np.zeros(1, dtype=np.uint32)
    with pytest.raises(_lib.DsuError):
        ops.texture_live_partition(words, 0, 1)
    # more halves than the kernel's LDS scan holds: the kernel runs its static ranges there
    big = np.zeros(2049, dtype=np.uint32)
    assert lib.dsu_texture_live_partition(big.ctypes.data, 2049 * 32, 4, 4, np.zeros(32, np.int32).ctypes.data) == -3
