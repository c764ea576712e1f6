"""The leave-one-out closed forms (tests/loo_ref.py) against n_T brute-force refits, their two forms against
each other, the leverage's identity with the reliability, and the host side of the interface (no GPU).

The GPU tests compare against loo_ref at 1e-9; here loo_ref is shown to be within 1e-9 (relative to max
|y^_loo|) of refitting without each animal, and the reference's own min(1 - h_tt) over every case the GPU tests use
is shown to be >= 0.05: the error of the closed form grows as 1 / (1 - h_tt), so with that the bound leaves the
1e-14 seen here its headroom.
"""
import os
import re

import numpy as np
import pytest

from tests import loo_ref as Z
from tests import model_ref as R
from tests import reliability_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9      # the project's EBV_RTOL
GAP = 0.05

BRUTE = [(s, k, br) for s in ((127, 5), (129, 64)) for k, br in ((Z.K40, "snp"), (Z.K300, "snp"), (400, "gblup"))]


@pytest.mark.parametrize("s,k,br", BRUTE)
def test_closed_form_matches_refits(s, k, br):
    pn = Z.panel()
    T = pn["splits"][s][0]
    assert k > R.N_ANIMALS or br == "snp"
    brute = Z.loo_brute(pn["genomes"][k], T, pn["geno"], pn["pheno"], Z.H2, br)
    scale = float(np.max(np.abs(brute)))
    worst = 0.0
    for form in ("snp", "kernel"):
        ref = Z.loo_ref(pn["genomes"][k], T, pn["geno"], pn["pheno"], Z.H2, br, form=form)
        assert ref["pred"].shape == (s[0],) and np.all(np.isfinite(ref["pred"]))
        err = float(np.max(np.abs(ref["pred"] - brute))) / scale
        worst = max(worst, err)
        assert err <= TOL, (s, k, br, form, err)
        assert ref["gap"] >= GAP
        np.testing.assert_allclose(ref["press"], np.sum((pn["pheno"][T] - brute) ** 2), rtol=1e-8)
    print("\nLOO host %s k=%s %s: max rel err against %d refits %.3e" % (s, k, br, s[0], worst))


def test_forms_agree_and_leverages_leave_room():
    """Every case the GPU tests use: the two forms agree, and min(1 - h_tt) >= 0.05."""
    pn = Z.panel()
    worst, lo = 0.0, 1.0
    for name, s, k, br in Z.cases():
        ref = Z.case_ref(name)
        assert np.all(np.isfinite(ref["pred"])) and np.all(np.isfinite(ref["leverage"])), name
        assert ref["gap"] >= GAP, (name, ref["gap"])
        assert np.all(ref["leverage"] > 0.0), name
        lo = min(lo, ref["gap"])
        other = Z.loo_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], Z.H2, br,
                          form="kernel" if len(pn["genomes"][k]) <= s[0] else "snp")
        scale = float(np.max(np.abs(ref["pred"])))
        worst = max(worst, float(np.max(np.abs(other["pred"] - ref["pred"]))) / scale,
                    float(np.max(np.abs(other["leverage"] - ref["leverage"]))))
        assert np.max(np.abs(other["pred"] - ref["pred"])) <= TOL * scale, name
        assert np.max(np.abs(other["leverage"] - ref["leverage"])) <= TOL, name
    deep = Z.deep_ref()
    assert deep["gap"] >= GAP
    lo = min(lo, deep["gap"])
    for tr in range(1, 4):      # the other phenotype columns share the leverages: only the split matters
        assert Z.case_ref("auto-129-64-200", tr)["gap"] == Z.case_ref("auto-129-64-200")["gap"]
    print("\nLOO host: max form difference %.3e, min(1 - h_tt) over the GPU cases %.3f" % (worst, lo))


def test_leverage_is_the_reliability_identity():
    """gblup: h_tt = K_tt (1 - rel_t) / lambda for a training animal (PEV_t = K_tt - k_t' V^-1 k_t = lambda h_tt)."""
    pn = Z.panel()
    for s, k in (((127, 5), 400), ((257, 70), 200)):
        T = pn["splits"][s][0]
        idx = pn["genomes"][k]
        ref = Z.loo_ref(idx, T, pn["geno"], pn["pheno"], Z.H2, "gblup")
        rel = Q.rel_ref(idx, T, pn["geno"], Z.H2, "gblup")[T]
        w, _, d, lam = Q._setup(idx, T, pn["geno"], Z.H2, "gblup", np.float64)
        ktt = np.sum(w[T] * w[T], axis=1) / d
        assert np.max(np.abs(ref["leverage"] - ktt * (1.0 - rel) / lam)) <= 1e-11


def test_monomorphic_panel_is_nan():
    pn = Z.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    T = pn["splits"][129, 64][0]
    ref = Z.loo_ref(np.array([0]), T, geno, pn["pheno"], Z.H2)
    assert np.all(np.isnan(ref["pred"])) and np.isnan(ref["fitness"])


def test_header_and_signature_table():
    from tblup_amd import _native
    src = open(os.path.join(ROOT, "include", "tblup_gpu.h")).read()
    m = re.search(r"int tblup_loo_batch\(([^;]*)\);", src)
    assert m, "include/tblup_gpu.h does not declare tblup_loo_batch"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 12
    assert args[7:] == ["double* fitness", "double* loo_pred", "double* leverage", "double* press",
                        "double* eval_fitness"]
    restype, argtypes = _native.SIGNATURES["tblup_loo_batch"]
    assert len(argtypes) == 12


def test_python_surface():
    import inspect
    from tblup_amd.engine import GpuBlupEngine
    from tblup_amd.evaluator import BlupParallelEvaluator
    sig = inspect.signature(GpuBlupEngine.loo)
    assert list(sig.parameters)[1:7] == ["genomes", "train", "valid", "h2", "branch", "return_leverage"]
    assert sig.parameters["branch"].default == "auto" and sig.parameters["return_leverage"].default is False
    sig = inspect.signature(BlupParallelEvaluator.loo)
    assert list(sig.parameters)[1:5] == ["population", "final", "train", "valid"]
    assert sig.parameters["final"].default is True


def test_fixed_effects_are_refused():
    """LOO under covariates or a class factor is not built: a ValueError that says so, before anything runs."""
    from tblup_amd.engine import GpuBlupEngine
    e = object.__new__(GpuBlupEngine)      # no context: the refusal comes first
    e._ctx = None
    e._pending = None
    for kw in ({"covariates": np.zeros((4, 1))}, {"groups": np.zeros(4, dtype=np.int64)}):
        with pytest.raises(ValueError, match="LOO under fixed effects .* is not built"):
            e.loo([np.array([0])], [0, 1], [2, 3], 0.4, **kw)


def test_loo_result_shapes_and_residuals():
    from tblup_amd.model import LooResult
    rng = np.random.default_rng(5)
    n, nT, B = 20, 7, 3
    train = rng.permutation(n)[:nT]
    y = rng.standard_normal(n)
    pred = rng.standard_normal((B, nT))
    r = LooResult(np.ones(B), pred, np.ones(B), np.full((B, nT), 0.1), np.ones(B), train)
    assert r.pred.shape == (B, nT) and r.leverage.shape == (B, nT) and r.press.shape == (B,)
    np.testing.assert_array_equal(r.train, train)
    np.testing.assert_array_equal(r.residuals(y), y[train][None, :] - pred)
    np.testing.assert_array_equal(r.residuals(y[:, None]), r.residuals(y))
    Y = rng.standard_normal((n, 2))
    pred2 = rng.standard_normal((B, 2, nT))
    r2 = LooResult(np.ones(B), pred2, np.ones((B, 2)), None, np.ones(B), train)
    assert r2.leverage is None
    res = r2.residuals(Y)
    assert res.shape == (B, 2, nT)
    np.testing.assert_array_equal(res[:, 1, :], Y[train, 1][None, :] - pred2[:, 1, :])
    with pytest.raises(ValueError):
        r2.residuals(y)
    with pytest.raises(ValueError):
        r.residuals(Y)
    with pytest.raises(ValueError):
        LooResult(np.ones(B), pred, np.ones(B + 1), None, np.ones(B), train)
    with pytest.raises(ValueError):
        LooResult(np.ones(B), pred[:, :-1], np.ones(B), None, np.ones(B), train)
