"""The host model of the non-finite contract (tests/helpers/nonfinite_model.py), on the CPU: classify / inject / check_contract held
to hand-made tensors - each rule must catch a deliberately laundered one - and every case list of tests/test_gpu_nonfinite.py held
to its own admission rule: the float32 and the float64 reference agree on the class of every element (disagreements allowed: none),
so that the injected special is the only source of non-finite values."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import nonfinite_model as M  # noqa: E402

NAN, INF = float("nan"), float("inf")
FMAX = torch.finfo(torch.float32).max


def test_classify_codes():
    t = torch.tensor([0.0, -1.5, NAN, INF, -INF, FMAX, -FMAX, 1e-45])
    assert M.classify(t).tolist() == [M.FINITE, M.FINITE, M.NAN, M.PINF, M.NINF, M.FINITE, M.FINITE, M.FINITE]
    assert M.classify(t.double()).tolist() == M.classify(t).tolist()
    assert M.classify(torch.zeros(2, 3)).shape == (2, 3)


def test_inject_writes_only_the_chosen_places():
    x = torch.arange(12.0).reshape(3, 4)
    y = M.inject(x, [0, 11, (1, 2)], [NAN, INF, -INF])
    assert torch.equal(x, torch.arange(12.0).reshape(3, 4)), "the input is left alone"
    c = M.classify(y)
    assert c[0, 0] == M.NAN and c[2, 3] == M.PINF and c[1, 2] == M.NINF and int((c != M.FINITE).sum()) == 3
    keep = c == M.FINITE
    assert torch.equal(y[keep], x[keep])
    assert int((M.classify(M.inject(x, [1, 2], NAN)) == M.NAN).sum()) == 2


def _want():
    w = torch.linspace(-3.0, 5.0, 64)
    w[7], w[20], w[41] = NAN, INF, -INF
    return w


def test_contract_accepts_the_reference_itself_and_noise_inside_the_tolerance():
    w = _want()
    assert M.check_contract(w.clone(), w, w.double(), 0.0) is None
    noisy = w.clone()
    noisy[3] += 4e-6                      # 5 is the largest finite magnitude: 4e-6 / 5 < 1e-6
    assert M.check_contract(noisy, w, w.double(), 1e-6) is None


def test_contract_rejects_nan_laundered_to_zero():
    w = _want()
    got = w.clone()
    got[7] = 0.0
    msg = M.check_contract(got, w, w.double(), 1e-6)
    assert msg is not None and "laundered" in msg and "index 7" in msg and "NaN" in msg, msg
    assert "laundered" in M.check_contract(got, w, w.double(), 1e-6, strict_class=False)


def test_contract_rejects_inf_laundered_to_the_largest_finite_value():
    w = _want()
    for idx, val in ((20, FMAX), (41, -FMAX)):
        got = w.clone()
        got[idx] = val
        for strict in (True, False):
            msg = M.check_contract(got, w, w.double(), 1e-6, strict_class=strict)
            assert msg is not None and "laundered" in msg and "index %d" % idx in msg, msg


def test_contract_rejects_one_finite_element_off_by_ten_tolerances():
    w = _want()
    tol = 1e-5
    got = w.clone()
    got[30] += 10 * tol * 5.0             # the rest is exact; 5 is the largest finite expected magnitude
    msg = M.check_contract(got, w, w.double(), tol)
    assert msg is not None and "finite and wrong" in msg and "index 30" in msg, msg
    # ... and the escape for scaled forms does not cover it: non-finite is allowed there, finite and wrong never is
    assert "finite and wrong" in M.check_contract(got, w, w.double(), tol, strict_class=False, allow_nonfinite_for_finite=True)


def test_contract_class_rules():
    w = _want()
    got = w.clone()
    got[20] = NAN                          # an Inf that arrives as a NaN: a contraction may, a stream kernel may not
    assert "laundered" in M.check_contract(got, w, w.double(), 1e-6)
    assert M.check_contract(got, w, w.double(), 1e-6, strict_class=False) is None
    got = w.clone()
    got[20] = -INF
    assert "laundered" in M.check_contract(got, w, w.double(), 1e-6)
    got = w.clone()
    got[2] = NAN                           # a finite reference element that comes out non-finite
    assert "poisoned" in M.check_contract(got, w, w.double(), 1e-6)
    assert "poisoned" in M.check_contract(got, w, w.double(), 1e-6, strict_class=False)
    assert M.check_contract(got, w, w.double(), 1e-6, strict_class=False, allow_nonfinite_for_finite=True) is None


def test_contract_normalises_by_the_largest_finite_magnitude_only():
    w = torch.tensor([1.0, 2.0, INF, 1e30])
    w[3] = INF
    got = w.clone()
    got[0] = 1.0 + 1e-3                    # 5e-4 of the largest FINITE magnitude 2 (an Inf in the denominator would hide it)
    assert "finite and wrong" in M.check_contract(got, w, w.double(), 1e-4)
    assert M.check_contract(got, w, w.double(), 1e-3) is None


def test_contract_refuses_references_that_disagree_and_wrong_shapes():
    w64 = torch.tensor([1.0, 1e39], dtype=torch.float64)
    w32 = w64.float()                      # overflows to +Inf in float32 only
    assert M.references_agree(w32, w64) == 1
    with pytest.raises(AssertionError, match="references disagree"):
        M.check_contract(w32.clone(), w32, w64, 1e-6)
    assert "shape" in M.check_contract(torch.zeros(3), torch.zeros(2), torch.zeros(2).double(), 1e-6)


def test_named_places():
    assert M.vector_places(7) == {"first": 0, "last": 6, "tail": 4}
    p = M.vector_places(1027)
    assert p["body"] % 4 not in (0, 3) and p["body"] < 1024 and p["tail"] == 1024 and p["last"] == 1026
    assert M.vector_places(3) == {"first": 0, "last": 2}
    p = M.plane_places((5, 7, 2, 4))
    assert p == {"first": 0, "last": 279, "plane_first": 33 * 8, "plane_last": 33 * 8 + 7}
    assert M.plane_places((3, 5, 1, 1)) == {"first": 0, "last": 14, "plane_first": 13}
    assert M.plane_places((2, 3, 4, 4), 1, 0) == {"first": 0, "last": 95, "plane_first": 48, "plane_last": 63}
    assert M.row_places(3, 1028) == {"row_first": 1028, "row_last": 2055, "pad_neighbour": 1028 + 1026}
    assert M.row_places(3, 4094) == {"row_first": 4094, "row_last": 8187, "pad_neighbour": 4094 + 4091}
    assert M.row_places(3, 3) == {"row_first": 3, "row_last": 5}


def test_finite_values_are_bounded_and_reproducible():
    a, b = M.finite_values((1000,), 8.0, 3), M.finite_values((1000,), 8.0, 3)
    assert torch.equal(a, b) and a.dtype == torch.float32 and float(a.abs().max()) <= 8.0 and float(a.abs().max()) > 7.0
    assert not torch.equal(a, M.finite_values((1000,), 8.0, 4))


@pytest.mark.parametrize("family,cfg", M.stream_configs(), ids=lambda v: str(v).replace(" ", ""))
def test_stream_references_agree_on_every_class(family, cfg):
    """Every case of every stream-kernel list: float32 and float64 reference give the same class at every element of every output,
    the special reaches at least one output, and the inputs hold exactly the injected specials."""
    _, cases, _, tols = M.STREAM_FAMILIES[family]
    n = 0
    for case in cases(cfg):
        n += 1
        specials = sum(int((M.classify(t) != M.FINITE).sum()) for t in case.inputs.values())
        assert specials >= 1, case.id
        for k, t in case.inputs.items():
            bound = M.G_BOUND if k in ("g", "g_add", "acc") or (family == "stencil" and cfg[0] in ("add3", "fork3")) else M.X_BOUND
            fin = t[torch.isfinite(t)]
            assert t.dtype == torch.float32 and (fin.numel() == 0 or float(fin.abs().max()) <= bound), (case.id, k)
        w32, w64 = M.both_references(family, case)
        assert set(w32) == set(w64) and set(w64) <= set(tols), case.id
        touched = 0
        for k in w64:
            assert w32[k].dtype == torch.float32 and w64[k].dtype == torch.float64, (case.id, k)
            assert M.references_agree(w32[k], w64[k]) == 0, "%s: %s: the references disagree on %d element(s)" % (
                case.id, k, M.references_agree(w32[k], w64[k]))
            # the reference's own float32 arithmetic keeps the contract at the operation's tolerance
            msg = M.check_contract(w32[k], w32[k], w64[k], tols[k])
            assert msg is None, "%s: %s: %s" % (case.id, k, msg)
            touched += int((M.classify(w64[k]) != M.FINITE).sum())
        # (a saturating operation may absorb an Inf - tanh(+Inf) = 1 with derivative 0 - but never a NaN; the 2x2 mean of an odd map
        # never reads its last row and column)
        if any(bool(torch.isnan(t).any()) for t in case.inputs.values()) and not (family == "stencil" and cfg[0] == "avgpool"):
            assert touched >= 1, "%s: the NaN reaches no output of the reference" % case.id
    assert n >= 2


@pytest.mark.parametrize("name", sorted(M.CONTRACTIONS))
def test_contraction_references_agree_on_every_class(name):
    """The same admission rule for the contractions' case list, through the oracle's spectral norm."""
    n = 0
    for case in M.contraction_cases(name):
        n += 1
        w32, w64 = M.contraction_reference(case, torch.float32), M.contraction_reference(case, torch.float64)
        touched = 0
        for k in w64:
            assert M.references_agree(w32[k], w64[k]) == 0, "%s: %s: the references disagree on %d element(s)" % (
                case.id, k, M.references_agree(w32[k], w64[k]))
            msg = M.check_contract(w32[k], w32[k], w64[k], M.CONTRACTION_TOL[k])
            assert msg is None, "%s: %s: %s" % (case.id, k, msg)
            touched += int((M.classify(w64[k]) != M.FINITE).sum())
        assert touched >= 1, "%s: the special reaches no output of the reference" % case.id
        operand, cls = M.special_of(case)
        assert operand in ("x", "w", "g") and cls in (M.NAN, M.PINF, M.NINF)
    assert n in (9, 12)
