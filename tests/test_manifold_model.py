"""The numpy model of the manifold metrics (tests/helpers/manifold_model.py) against toys counted by hand and against the
properties the metrics are used for.  The GPU tests hold the kernels to this model with ==, so it has to be right on its own."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import manifold_model as M  # noqa: E402


def points(values, row=64):
    """one-dimensional points as code rows: the value in byte 0, zeros elsewhere"""
    codes = np.zeros((len(values), row), dtype=np.int8)
    codes[:, 0] = values
    return M.triple(codes)


def clusters(centres, per, seed, row=64, spread=3):
    """`per` rows around each centre value: every byte the centre plus noise in [-spread, spread], the SAME `per` noise rows around
    every centre - the modes are translates of each other, so whatever holds in one holds in all (nothing reaches the clamp)"""
    noise = np.random.default_rng(seed).integers(-spread, spread + 1, size=(per, row))
    assert min(centres) - spread >= -128 and max(centres) + spread <= 127
    return M.triple(np.concatenate([c + noise for c in centres]))


def test_three_collinear_points_counted_by_hand():
    """reals at 0, 10, 30 and k = 1: radii^2 100, 100, 400.  Fakes at 1, 12, 100: radii^2 121, 121, 88^2.
    fake 1  : d2 to the reals 1, 81, 841       -> in the balls of 0 and 10                    hits 2
    fake 12 : 144, 4, 324                      -> in the balls of 10 and 30                   hits 2
    fake 100: 10000, 8100, 4900                -> in none                                     hits 0
    covered: real 0 by one fake, 10 by two, 30 by one.
    real 0  : d2 to the fakes 1, 144, 10000    -> in the ball of 1 (121) only                 hits 1
    real 10 : 81, 4, 8100                      -> in the balls of 1 and 12, not of 100 (7744) hits 2
    real 30 : 841, 324, 4900                   -> in the ball of 100                          hits 1"""
    r, g = points([0, 10, 30]), points([1, 12, 100])
    assert M.kth_radius(r, 1).tolist() == [100, 100, 400] and M.kth_radius(g, 1).tolist() == [121, 121, 88 * 88]
    hits_g, cov_r = M.within(M.distances(g[0], r[0]), M.kth_radius(r, 1))
    assert hits_g.tolist() == [2, 2, 0] and cov_r.tolist() == [1, 2, 1]
    hits_r, _ = M.within(M.distances(r[0], g[0]), M.kth_radius(g, 1))
    assert hits_r.tolist() == [1, 2, 1]
    value = M.between(g, r, 1)
    assert value["counts"] == {"precise": 2, "recalled": 3, "hit_sum": 4, "covered": 3}
    assert (value["precision"], value["recall"], value["density"], value["coverage"]) == (2 / 3, 1.0, 4 / 3, 1.0)
    assert (value["images"], value["real_images"], value["k"], value["nonfinite"], value["baseline"]) == (3, 3, 1, 0, None)


def test_within_rules():
    d2 = np.array([[0, 5, 9], [5, 0, 4]], dtype=np.int64)
    assert [a.tolist() for a in M.within(d2, [5, 5, 5])] == [[2, 3], [2, 2, 1]]          # <= : the boundary counts
    assert [a.tolist() for a in M.within(d2, [4, 4, 4])] == [[1, 2], [1, 1, 1]]
    assert [a.tolist() for a in M.within(d2, [-1, 9, 9])] == [[2, 2], [0, 2, 2]]         # a negative radius: no ball
    assert [a.tolist() for a in M.within(d2, [9, 9, 9], qflags=[1, 0])] == [[0, 3], [1, 1, 1]]
    assert [a.tolist() for a in M.within(d2, [9, 9, 9], rflags=[0, 2, 0])] == [[2, 2], [2, 0, 2]]
    assert [a.tolist() for a in M.within(d2, [9, 9, 9], skip=[0, -1])] == [[2, 3], [1, 2, 2]]


def test_kth_radius_no_ball():
    x = points([0, 3, 7])
    assert M.kth_radius(x, 2).tolist() == [49, 16, 49] and M.kth_radius(x, 3).tolist() == [-1, -1, -1]
    flagged = (x[0], x[1], np.array([0, 1, 0], np.int32))
    assert M.kth_radius(flagged, 1).tolist() == [49, -1, 49]          # the flagged row has no ball and is nobody's neighbour


def test_a_set_against_itself():
    a = clusters([-90, -30, 30, 90], 8, seed=1)
    for k in (1, 3):
        value = M.between(a, a, k)
        assert value["precision"] == value["recall"] == value["coverage"] == 1.0 and value["density"] >= 1.0


def test_two_far_apart_clusters():
    value = M.between(clusters([-100], 12, seed=2), clusters([100], 12, seed=3), 3)
    assert (value["precision"], value["recall"], value["density"], value["coverage"]) == (0.0, 0.0, 0.0, 0.0)


def test_dropping_half_of_the_modes():
    """the fakes are fresh draws around the reals' modes; those of the last two modes are then left out.  The modes are translates
    of each other and far apart, so each holds the same share of precise fakes: precision is unchanged, exactly; half of the reals
    have no fake near"""
    real = clusters([-90, -30, 30, 90], 16, seed=4)
    fake = clusters([-90, -30, 30, 90], 16, seed=5)
    half = tuple(t[:32] for t in fake)
    full, dropped = M.between(fake, real, 3), M.between(half, real, 3)
    assert full["precision"] == dropped["precision"] > 0.0 and 2 * dropped["counts"]["precise"] == full["counts"]["precise"]
    assert dropped["recall"] < full["recall"] and dropped["coverage"] < full["coverage"]
    assert dropped["recall"] <= 0.5 and dropped["coverage"] <= 0.5


def test_a_flagged_sample_stays_in_the_denominators():
    real = clusters([0], 8, seed=6)
    fake = clusters([0], 8, seed=7)
    flags = np.zeros(8, np.int32)
    flags[2] = 5
    clean, bad = M.between(fake, real, 2), M.between((fake[0], fake[1], flags), real, 2)
    assert bad["nonfinite"] == 1 and bad["images"] == 8 and bad["counts"]["precise"] == clean["counts"]["precise"] - 1
    assert bad["precision"] == bad["counts"]["precise"] / 8


def test_the_record_from_images():
    rng = np.random.default_rng(8)
    real, fake = (rng.uniform(-1, 1, size=(6, 3, 4, 4)).astype(np.float32) for _ in range(2))
    fake[1, 0, 0, 0] = np.nan
    value = M.record(fake, real, 2, baseline={"precision": 1.0})
    assert sorted(value) == ["baseline", "counts", "coverage", "density", "images", "k", "nonfinite", "precision", "real_images", "recall"]
    assert value["nonfinite"] == 1 and value["baseline"] == {"precision": 1.0} and value["density"] == value["counts"]["hit_sum"] / 12
