"""The restatement behind tests/test_gpu_reliab_cov.py, checked on the CPU, and the host side of the reliabilities
under fixed-effect covariates.

  * the mixed-model-equation route (tests/reliab_cov_ref.py::mme_ref, float64) against the header's V-form
    formulas in np.longdouble, within covar_ref.HOST_TOL of the largest |ref| (rel_cov, pev_total, cov_cov)
  * rel_cov <= the plain reliability (tests/reliability_ref.py) for every animal: estimating b can only add
    error variance.  Both are float64 restatements by different routes, so the comparison allows HOST_TOL
  * cov_cov[-1, -1] of the model with [Q, x_j] is 1 / v_P(j) of tests/score_cov_ref.py: the Schur complement of
    the appended column in G.  Bound: ROUTE_TOL = 1e-8 max(1, |ref|), the bound tests/test_score_cov_host.py
    gives the same appended-column route -- eps times the condition of the (c + 1) x (c + 1) system, which
    cond(G) <= COND_MAX and the SNPs' share outside the covariates' span (v_P >= 1e-6 v) keep below 1e8
  * the inputs keep the GPU tolerance meaningful: cond(G) <= covar_ref.COND_MAX and K_aa > 0, asserted in mme_ref
  * GpuBlupEngine's argument validation of the new keywords (no device), CovReliability, the binding and the header
"""
import os
from collections import OrderedDict

import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tests import reliab_cov_ref as Q
from tests import reliability_ref as RQ
from tests import score_cov_ref as A
from tests import score_ref as S

ROUTE_TOL = 1e-8
# every split, form and covariate count (tests/test_score_cov_host.py's selection)
NAMES = ["auto-127-5-64", "auto-127-5-332", "auto-128-2-1", "auto-128-2-129", "auto-129-64-65", "auto-129-64-dup",
         "auto-129-64-332", "auto-257-70-200", "auto-257-70-neg", "snp-129-64-200", "snp-257-70-400",
         "gblup-127-5-%s" % R.GBLUP_KS[0], "gblup-257-70-%s" % R.GBLUP_KS[-1], "deep"]


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / float(np.max(np.abs(ref))))


def test_names_are_cases():
    known = {c[0] for c in Q.cases()}
    assert set(NAMES) <= known
    assert {c[5] for c in Q.cases() if c[0] in NAMES} == {1, 5, 16}


@pytest.mark.parametrize("name", NAMES)
def test_mme_route_against_the_v_form_in_longdouble(name):
    idx, T, V, geno, pheno, cov, br = Q.case_inputs(name)
    ref = Q.case_ref(name)                                  # asserts cond(G) <= COND_MAX and K_aa > 0
    for f in ("rel", "pev", "cov_cov"):
        assert np.all(np.isfinite(ref[f])), (name, f)
    assert np.all(ref["pev"] > 0) and np.all(np.diag(ref["cov_cov"]) > 0)
    # (the deeper panel: its 520-row longdouble factorisation once, 65 animals behind it)
    an = Q.animal_list(geno.shape[0], T, 65) if name == "deep" else np.arange(geno.shape[0])
    wide = Q.vform_wide(idx, T, geno, cov, Q.H2, br, animals=an)
    for f in ("rel", "pev", "cov_cov"):
        err = _rel(ref[f] if f == "cov_cov" else ref[f][an], wide[f])
        print("  %-24s %-8s %.3e" % (name, f, err))
        assert err <= Q.HOST_TOL, (name, f, err)
    lst = Q.animal_list(geno.shape[0], T, 17)
    part = Q.mme_ref(idx, T, geno, cov, Q.H2, br, animals=lst)
    assert S.close(part["rel"], ref["rel"][lst]) <= 1e-13      # an animal's value: not the list's
    assert S.close(part["pev"], ref["pev"][lst]) <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_never_above_the_plain_reliability(name):
    idx, T, V, geno, pheno, cov, br = Q.case_inputs(name)
    plain = RQ.rel_ref(idx, T, geno, Q.H2, br)
    ref = Q.case_ref(name)
    assert np.all(ref["rel"] <= plain + Q.HOST_TOL), (name, float(np.max(ref["rel"] - plain)))
    # and the predicted value's error variance is at least the genomic value's own PEV
    assert np.all(ref["pev"] >= (1 - plain) * ref["kaa"] - Q.HOST_TOL * np.max(ref["kaa"]))


@pytest.mark.parametrize("name", [n for n in NAMES if n != "deep"])
def test_cov_cov_of_the_appended_snp_is_the_score_tests_information(name):
    idx, T, V, geno, pheno, cov, br = Q.case_inputs(name)
    if cov.shape[1] >= C.MAX_COV:
        cov = np.ascontiguousarray(cov[:, :C.MAX_COV - 1])
    snps = S.wrap(A.cand_list(idx, geno.shape[1], 4), geno.shape[1])
    vp = A.adj_ref(idx, T, geno, pheno, cov, Q.H2, br, snps=snps)["v"]
    assert np.all(vp > 0)
    none = np.zeros(0, dtype=np.int64)
    gblup = R._branch(len(np.asarray(idx)), geno.shape[0], br) == "gblup"
    for j, col in enumerate(snps):
        x = np.asarray(geno)[:, [col]].astype(np.float64)
        if gblup:            # w_j's own centre (all animals): the gblup model centres no covariate itself
            x = x - x.mean()
        q1 = np.ascontiguousarray(np.hstack([cov, x]))
        cc = Q.mme_ref(idx, T, geno, q1, Q.H2, br, animals=none, check=False)["cov_cov"]
        ref = 1.0 / vp[j]
        assert abs(cc[-1, -1] - ref) <= ROUTE_TOL * max(1.0, abs(ref)), (name, col, cc[-1, -1], ref)


def test_degenerate_inputs_of_the_restatement():
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    q = Q.make_cov(R.N_ANIMALS, 3)
    out = Q.mme_ref(np.array([0]), T, geno, q, Q.H2, check=False)
    assert np.all(np.isnan(out["rel"])) and np.all(np.isnan(out["cov_cov"]))
    two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 2]], axis=1))
    out = Q.vform_ref(pn["genomes"][64], T, pn["geno"], two, Q.H2)
    assert np.all(np.isnan(out["rel"])) and np.all(np.isnan(out["pev"]))
    with pytest.raises(AssertionError):
        Q.mme_ref(np.array([0]), T, geno, q, Q.H2)


# ---------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------
class _NoLib:
    """Any call into the library fails the test: validation comes first."""

    def __getattr__(self, name):
        raise AssertionError("library called: " + name)


def _engine(n=50, p=40, nt=1):
    from tblup_amd.engine import GpuBlupEngine
    eng = GpuBlupEngine.__new__(GpuBlupEngine)
    eng._lib, eng._ctx, eng._splits, eng._next_split, eng._pending = _NoLib(), None, OrderedDict(), 0, None
    eng.n_animals, eng.n_snps, eng.n_traits = n, p, nt
    return eng


def test_engine_validates_the_new_keywords_before_any_call():
    eng = _engine()
    T, V, g = np.arange(30), np.arange(30, 40), [np.arange(5)]
    bad = [np.zeros((49, 2)), np.zeros((50, 17)), np.zeros((50, 0)), np.zeros((50, 2, 1)),
           np.full((50, 2), np.nan), np.full((50, 1), np.inf)]
    for q in bad:
        with pytest.raises(ValueError):
            eng.reliability_cov(g, T, V, 0.4, [1, 2], covariates=q)
    with pytest.raises(ValueError):
        eng.reliability_cov(g, T, V, 0.4, [[1, 2]], covariates=np.zeros((50, 2)))
    # reliability() itself keeps its parameters: the covariate keywords belong to reliability_cov alone
    for kw in ("covariates", "return_pev", "return_cov_cov", "return_models"):
        with pytest.raises(TypeError):
            eng.reliability(g, T, V, 0.4, [1, 2], **{kw: True})
    with pytest.raises(TypeError):
        eng.reliability_cov(g, T, V, 0.4, [1, 2])            # covariates are not optional there
    # fit(reliability_of=, covariates=) stays an error and says where to go
    with pytest.raises(ValueError):
        eng.fit(g, T, V, 0.4, reliability_of=[1, 2], covariates=np.zeros((50, 2)))
    assert "return_models=True" in type(eng).fit.__doc__


def test_cov_reliability_and_its_standard_errors():
    from tblup_amd.model import CovReliability
    rng = np.random.default_rng(0)
    rel, pev = rng.random((2, 5)), rng.random((2, 5))
    g = rng.standard_normal((2, 3, 3))
    cc = g @ np.swapaxes(g, 1, 2) + np.eye(3)
    r = CovReliability(rel, pev, cc)
    assert r.models is None
    np.testing.assert_array_equal(r.reliability, rel)
    s2 = np.array([2.0, 0.5])
    want = np.sqrt(s2[:, None] * np.stack([np.diag(cc[0]), np.diag(cc[1])]))
    got = r.cov_stderr(s2)
    assert got.shape == (2, 1, 3)
    np.testing.assert_allclose(got[:, 0], want, rtol=1e-15)
    s2t = np.array([[2.0, 1.0, 3.0, 4.0], [0.5, 0.25, 1.0, 2.0]])
    got = r.cov_stderr(s2t)
    assert got.shape == (2, 4, 3)
    np.testing.assert_allclose(got[1, 3], np.sqrt(2.0 * np.diag(cc[1])), rtol=1e-15)
    assert np.all(np.isnan(CovReliability(rel, None, np.full((2, 3, 3), np.nan)).cov_stderr(s2)))
    with pytest.raises(ValueError):
        CovReliability(rel).cov_stderr(s2)
    with pytest.raises(ValueError):
        r.cov_stderr(np.ones(3))
    for bad in (dict(pev_total=pev[:1]), dict(cov_cov=cc[:1]), dict(cov_cov=cc[:, :2]), dict(models=[None])):
        with pytest.raises(ValueError):
            CovReliability(rel, **bad)
    with pytest.raises(ValueError):
        CovReliability(rel[0])


def test_binding_header_and_library_declare_the_entry():
    from tblup_amd import _native
    name, nargs = "tblup_reliability_cov_batch", 20
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tblup_gpu.h")) as f:
        header = f.read()
    assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
    assert "int %s(" % name in header
    assert hasattr(_native.load(), name)
