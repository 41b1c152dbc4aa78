"""tools/rank_sim.py: the CPU prediction of the balanced pass's pass-2 iterations per wave."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rank_sim  # noqa: E402


def test_block_fold_beats_wave_fold_on_config3_crop():
    counts = rank_sim.config_counts(3, (512, 64))
    assert counts.shape == (64, 512) and 0 <= counts.min() and counts.max() <= 64
    r = rank_sim.simulate(counts)
    assert r["wave"].size == 8 * 8 * 4 and r["block_ranked"].all()
    wave, block, floor = r["wave"].mean(), r["block"].mean(), r["floor"].mean()
    print(f"per-wave fold {wave:.3f}, per-block fold {block:.3f}, floor {floor:.3f}")
    assert block < wave
    assert wave >= floor and block >= floor
    assert (r["wave"] >= r["floor"]).all()  # wave by wave the floor binds the wave's own fold


def test_folds_on_known_counts():
    # One workgroup: wave 0 all 64 lights, wave 1 none, waves 2-3 half. Per wave: 64, 0, 32, 32; together every
    # thread pairs a full pixel with an empty one or two halves: 32 everywhere.
    counts = np.zeros((8, 64), np.int64)
    counts[0:2] = 64
    counts[4:8] = 32
    r = rank_sim.simulate(counts)
    assert r["wave"].tolist() == [64, 0, 32, 32]
    assert r["block"].tolist() == [32, 32, 32, 32]
    # a wave without geometry: the workgroup ranks per wave and that wave is not counted
    geo = np.ones((8, 64), bool)
    geo[2:4] = False
    r = rank_sim.simulate(counts, geo)
    assert r["wave"].tolist() == [64, 32, 32] and r["block"].tolist() == [64, 32, 32] and not r["block_ranked"].any()
