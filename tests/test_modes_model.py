"""The numpy model of the binned mode coverage (tests/helpers/modes_model.py) against brute force and hand-computed cases: group
sums, the rounding of the mean, the monotone objective of Lloyd's algorithm in integers, and the proportion test."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import modes_model as MM  # noqa: E402
import neighbours_model as NM  # noqa: E402


def triple(codes, flags=None):
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    return codes, NM.norms(codes), np.zeros(codes.shape[0], np.int32) if flags is None else np.asarray(flags, np.int32)


def test_group_sums_against_a_loop():
    rng = np.random.default_rng(1)
    codes = rng.integers(-128, 128, size=(9, 64), dtype=np.int8)
    order = np.array([3, 3, -1, 8, 9, 0, 5, 2, 2, 7, 1])          # repeats, -1 and N among valid ones
    starts = [2, 5, 5, 4, 40]          # ungrouped front, an empty group, one that decreases, one clamped
    want = np.zeros((4, 64), dtype=np.int64)
    for k, (lo, hi) in enumerate([(2, 5), (5, 5), (5, 4), (4, 11)]):
        for pos in range(lo, hi):
            if 0 <= order[pos] < 9:
                for j in range(64):
                    want[k, j] += int(codes[order[pos], j])
    assert np.array_equal(MM.group_sums(codes, order, starts, 4), want)
    assert MM.group_sizes(starts, 4, 11) == [3, 0, 0, 7] and not want[1].any() and not want[2].any()
    labels = np.array([2, -1, 0, 2, 1, 0, -1, 2, 2])
    order, starts = MM.grouping(labels, 4)
    assert order.tolist() == [1, 6, 2, 5, 4, 0, 3, 7, 8] and starts.tolist() == [2, 4, 5, 9, 9]
    sums = MM.group_sums(codes, order, starts, 4)
    assert all(np.array_equal(sums[k], codes[labels == k].astype(np.int64).sum(0)) for k in range(4))


def test_the_mean_is_rounded_by_floor_division():
    sums = np.zeros((6, 64), dtype=np.int64)
    sums[:4, 0] = (-3, -1, 1, 3)
    starts = [0, 2, 4, 6, 8, 8 + 5, 8 + 5 + 7]
    sums[4, :3] = (-128 * 5, 127 * 5, 0)
    sums[5, :3] = (-128 * 7, 127 * 7, 3)          # 3 / 7 rounds down, 4 / 7 up
    sums[5, 3] = 4
    previous = np.full((6, 64), 9, dtype=np.int8)
    codes, norms, moved = MM.centroids(sums, starts, 20, previous)
    assert codes[:4, 0].tolist() == [-1, 0, 1, 2]          # halves go towards +infinity: -1.5 -> -1, -0.5 -> 0, 0.5 -> 1, 1.5 -> 2
    assert codes[4, :3].tolist() == [-128, 127, 0] and codes[5, :4].tolist() == [-128, 127, 0, 1]
    assert not codes[:, 4:].any() and codes.dtype == np.int8
    assert norms.tolist() == [1, 0, 1, 4, 128 * 128 + 127 * 127, 128 * 128 + 127 * 127 + 1] and moved.tolist() == [64] * 6
    # an empty group keeps its centre and does not move
    kept, _, still = MM.centroids(sums, [0, 2, 2, 1, 8, 13, 20], 20, previous)
    assert (kept[1] == 9).all() and (kept[2] == 9).all() and still[1] == still[2] == 0 and kept[0, 0] == -1


def clustered(rng, N, K, row):
    centres = rng.integers(-100, 101, size=(K, row))
    return np.clip(centres[rng.integers(0, K, size=N)] + rng.integers(-6, 7, size=(N, row)), -128, 127).astype(np.int8)


@pytest.mark.parametrize("kind", ["random", "clustered", "duplicates"])
def test_inertia_never_increases(kind):
    rng = np.random.default_rng(7)
    N, K, row = 120, 9, 64
    codes = clustered(rng, N, 5, row) if kind == "clustered" else rng.integers(-128, 128, size=(N, row), dtype=np.int8)
    flags = np.zeros(N, np.int32)
    flags[[4, 50]] = 1
    initial = rng.permutation(np.flatnonzero(flags == 0))[:K]
    if kind == "duplicates":
        codes[initial[1]] = codes[initial[0]]          # two identical initial centres: the higher index gets nothing
        codes[initial[5]] = codes[initial[0]]
    centres, labels, counts, inertia, moved = MM.lloyd(triple(codes, flags), initial, 8)
    assert len(inertia) == 9 and all(a >= b for a, b in zip(inertia, inertia[1:])) and inertia[0] > inertia[-1]
    assert (labels[[4, 50]] == -1).all() and (labels[flags == 0] >= 0).all() and counts.sum() == N - 2
    if kind == "duplicates":
        assert counts[1] == 0 or counts[5] == 0 or not np.array_equal(centres[1], centres[5])
        assert np.array_equal(centres[5], codes[initial[0]])          # never fed: an empty cluster keeps its centre
    # the inertia is the objective of the labels against the centres they were assigned to
    last = ((codes[labels >= 0].astype(np.int64) - centres[labels[labels >= 0]].astype(np.int64)) ** 2).sum()
    assert last == inertia[-1]


def test_a_round_that_moves_nothing_repeats_itself():
    rng = np.random.default_rng(8)
    codes = clustered(rng, 90, 3, 64)
    initial = [0, 1, 2, 3]
    for rounds in range(1, 30):
        centres, labels, counts, inertia, moved = MM.lloyd(triple(codes), initial, rounds)
        if not moved[-1].any():
            break
    assert not moved[-1].any() and MM.converged_at(moved) == rounds
    again = MM.lloyd(triple(codes), initial, rounds + 3)
    assert np.array_equal(again[0], centres) and np.array_equal(again[1], labels) and not again[4][rounds - 1:].any()
    assert again[3][rounds - 1:] == [inertia[-1]] * 5 and MM.converged_at(again[4]) == rounds


def test_the_proportion_test_on_hand_computed_cases():
    same = MM.ndb_statistics([10, 20, 30], [20, 40, 60])
    assert same["z"] == [0.0] * 3 and same["ndb"] == 0 and same["js"] == 0.0 and same["missing"] == 0 and same["order"] == [0, 1, 2]
    apart = MM.ndb_statistics([50, 50, 0, 0], [0, 0, 50, 50])
    assert apart["js"] == pytest.approx(math.log(2), rel=1e-15) and apart["ndb"] == 4 and apart["missing"] == 2
    assert apart["order"] == [0, 1, 2, 3] and apart["z"][0] == apart["z"][1] < 0 < apart["z"][2]
    # n = m = 100, bin 0: p = 0.5, q = 0.3, P = 0.4: se = sqrt(0.4 0.6 0.02), z = -0.2 / se = -2.886...
    one = MM.ndb_statistics([50, 50], [30, 70])
    assert one["z"][0] == pytest.approx(-0.2 / math.sqrt(0.4 * 0.6 * 0.02), rel=1e-14) and one["z"][1] == pytest.approx(-one["z"][0], rel=1e-14)
    assert one["different"] == [True, True] and one["ndb_over_k"] == 1.0 and one["order"] == [0, 1] and one["missing"] == 0
    assert MM.ndb_statistics([50, 50], [45, 55])["ndb"] == 0          # |z| = 0.71
    # se == 0: a bin that holds nothing on either side (P = 0) and one that holds everything (P = 1)
    flat = MM.ndb_statistics([0, 7], [0, 3])
    assert flat["z"] == [0.0, 0.0] and flat["ndb"] == 0 and flat["js"] == 0.0
    assert MM.ndb_statistics([1, 2], [0, 0])["ndb"] is None and MM.ndb_statistics([0, 0], [1, 2])["js"] is None
    # alpha moves the critical value: |z| = 2.886 is inside 1 - 0.001
    assert MM.ndb_statistics([50, 50], [30, 70], alpha=0.001)["ndb"] == 0


def test_the_products_statistics_are_the_models():
    from locate_amd.modes import ndb_statistics
    rng = np.random.default_rng(9)
    for trial in range(20):
        K = int(rng.integers(1, 40))
        r, f = rng.integers(0, 200, size=K).tolist(), (rng.integers(0, 60, size=K) * (rng.random(K) > 0.3)).tolist()
        got, want = ndb_statistics(r, f), MM.ndb_statistics(r, f)
        assert sorted(got) == sorted(want)
        for key in ("ndb", "ndb_over_k", "missing", "different", "order"):
            assert got[key] == want[key], key
        if want["js"] is None:
            assert got["js"] is None and got["z"] is None
        else:
            assert got["js"] == pytest.approx(want["js"], rel=1e-12, abs=0.0) and got["z"] == pytest.approx(want["z"], rel=1e-12, abs=0.0)
