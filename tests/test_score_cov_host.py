"""The restatement behind tests/test_gpu_score_cov.py and tests/test_gpu_loglik_cov.py, checked on the CPU, and
the host side of the covariate-adjusted score statistics and likelihood.

  * float64 against np.longdouble within score_ref.HOST_TOL of the largest |ref| (u_P, v_P, q_P, sigma2_g;
    l_R relative to max(1, |l_R|))
  * two independent routes: u_P / v_P is the last GLS effect of covar_ref.gls_ref with the SNP appended as
    covariate c + 1; l_R and q_P are the explicit-contrast computation's (an SVD basis of the complement of
    [1 Q~_T], no identity of the restatement).  Bound: ROUTE_TOL = 1e-8 max(1, max |ref|), the bound
    tests/test_covar_host.py gives its own second route -- eps (1.1e-16) times the condition of the
    (c + 1) x (c + 1) system of the appended model, which cond(G) <= COND_MAX = 1e6 and the SNPs' share outside
    the covariates' span keep below 1e8; the contrast route differs by eps cond(V) N, below the same bound.
  * without covariates the formulas are score_ref's and loglik_ref's
  * the inputs keep the GPU tolerance meaningful: cond(G) <= covar_ref.COND_MAX, v_P >= 1e-6 v for every
    listed SNP, dof > 0
  * GpuBlupEngine's argument validation (no device), the binding and the header
"""
import os
from collections import OrderedDict

import numpy as np
import pytest

from tests import covar_ref as C
from tests import loglik_ref as LR
from tests import model_ref as R
from tests import score_cov_ref as A
from tests import score_ref as S

ROUTE_TOL = 1e-8
# every split, form and covariate count, without walking all 57 cases twice
NAMES = ["auto-127-5-64", "auto-127-5-332", "auto-128-2-1", "auto-128-2-129", "auto-129-64-65", "auto-129-64-dup",
         "auto-129-64-332", "auto-257-70-200", "auto-257-70-neg", "snp-129-64-200", "snp-257-70-400",
         "gblup-127-5-%s" % R.GBLUP_KS[0], "gblup-257-70-%s" % R.GBLUP_KS[-1], "deep"]


def test_names_are_cases():
    known = {c[0] for c in A.cases()}
    assert set(NAMES) <= known
    assert {c[5] for c in A.cases() if c[0] in NAMES} == {1, 5, 16}


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / float(np.max(np.abs(ref))))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_conditions_and_wide(name):
    idx, T, V, geno, pheno, cov, br = A.case_inputs(name)
    ref = A.case_ref(name)
    assert ref["dof"] > 0
    assert np.linalg.cond(ref["G"]) <= C.COND_MAX, name
    assert np.all(ref["v"] >= A.SPAN_MIN * ref["v_plain"]), name
    for f in ("u", "v", "q", "loglik", "sigma2_g", "b"):
        assert np.all(np.isfinite(ref[f])), (name, f)
    if name == "deep":       # one longdouble factorisation of 520 rows is enough for the largest panel
        return
    snps = A.cand_list(idx, geno.shape[1], 65)
    r64 = A.adj_ref(idx, T, geno, pheno, cov, A.H2, br, snps=snps)
    wide = A.adj_wide(idx, T, geno, pheno, cov, A.H2, br, snps=snps)
    for f in ("u", "v", "q", "sigma2_g", "b"):
        assert _rel(r64[f], wide[f]) <= A.HOST_TOL, (name, f, _rel(r64[f], wide[f]))
    assert LR.close(r64["loglik"], wide["loglik"].astype(np.float64)) <= A.HOST_TOL, name
    assert S.close(r64["u"], ref["u"][:, S.wrap(snps, geno.shape[1])]) <= 1e-13      # a SNP's value: not the list's


@pytest.mark.parametrize("name", [n for n in NAMES if n != "deep"])
def test_route_gls_effect_of_the_appended_snp(name):
    idx, T, V, geno, pheno, cov, br = A.case_inputs(name)
    if cov.shape[1] >= C.MAX_COV:
        cov = np.ascontiguousarray(cov[:, :C.MAX_COV - 1])
    snps = S.wrap(A.cand_list(idx, geno.shape[1], 5), geno.shape[1])
    ref = A.adj_ref(idx, T, geno, pheno, cov, A.H2, br, snps=snps)
    eff = ref["u"][0] / ref["v"]
    for j, col in enumerate(snps):
        # the appended column is w_j: under gblup (no mean fitted unless Q carries the ones) the column less
        # its mean over all animals; under snp gls_ref centres it over the train rows itself
        x = geno[:, [col]].astype(np.float64)
        q1 = np.ascontiguousarray(np.hstack([cov, x - x.mean() if ref["branch"] == "gblup" else x]))
        g = C.gls_ref(idx, T, geno, pheno, q1, A.H2, br)
        assert abs(g["b"][0, -1] - eff[j]) <= ROUTE_TOL * max(1.0, float(np.max(np.abs(eff)))), (name, j)
        # and the other effects are those of the model without the SNP, moved by its effect
        assert np.all(np.isfinite(g["b"]))


@pytest.mark.parametrize("name", ["auto-127-5-64", "auto-128-2-129", "auto-129-64-65", "snp-129-64-200",
                                  "gblup-127-5-%s" % R.GBLUP_KS[0], "gblup-257-70-%s" % R.GBLUP_KS[-1]])
def test_route_explicit_contrasts(name):
    idx, T, V, geno, pheno, cov, br = A.case_inputs(name)
    for h2 in A.H2S:
        ll, s2 = A.case_loglik(name, h2)
        ref = A.adj_ref(idx, T, geno, pheno, cov, h2, br, snps=[0])
        lc, qc = A.contrast_ref(idx, T, geno, pheno, cov, h2, br)
        assert abs(lc - ll) <= ROUTE_TOL * max(1.0, abs(lc)), (name, h2, lc, ll)
        assert abs(qc - ref["q"][0]) <= ROUTE_TOL * max(1.0, abs(qc)), (name, h2)
        assert abs(s2 - qc / ref["dof"]) <= ROUTE_TOL * max(1.0, abs(s2))


@pytest.mark.parametrize("name", ["auto-129-64-65", "auto-129-64-332", "snp-257-70-400"])
def test_without_covariates_it_is_the_plain_restatement(name):
    idx, T, V, geno, pheno, _, br = A.case_inputs(name)
    snps = A.cand_list(idx, geno.shape[1], 17)
    got = A.adj_ref(idx, T, geno, pheno, None, A.H2, br, snps=snps)
    u, v, q = S.score_ref(idx, T, geno, pheno, A.H2, br, snps=snps, form="kernel")
    np.testing.assert_allclose(got["u"], u, rtol=0, atol=1e-12 * max(1.0, np.max(np.abs(u))))
    np.testing.assert_allclose(got["v"], v, rtol=0, atol=1e-12 * max(1.0, np.max(np.abs(v))))
    np.testing.assert_allclose(got["q"], q, rtol=0, atol=1e-12 * max(1.0, np.max(np.abs(q))))
    assert got["dof"] == S.dof(idx, T, geno, br)
    ll, s2 = LR.loglik_ref(idx, T, geno, pheno, A.H2, br)
    assert abs(got["loglik"][0] - ll) <= 1e-10 * max(1.0, abs(ll))
    assert abs(got["sigma2_g"][0] - s2) <= 1e-10 * max(1.0, abs(s2))


def test_degenerate_inputs_of_the_restatement():
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    g = pn["genomes"][64]
    q = A.make_cov(R.N_ANIMALS, 3)
    two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 2]], axis=1))
    ref = A.adj_ref(g, T, pn["geno"], pn["pheno"], two, A.H2, snps=[3, 4])
    assert all(np.all(np.isnan(ref[f])) for f in ("u", "v", "q", "loglik", "sigma2_g", "b"))
    # a listed SNP equal to a covariate column: exact zeros
    q2 = q.copy()
    q2[:, 1] = pn["geno"][:, 11]
    ref = A.adj_ref(g, T, pn["geno"], pn["pheno"], q2, A.H2, snps=[11, 12])
    assert ref["u"][0, 0] == 0 and ref["v"][0] == 0 and ref["v"][1] > 0
    # c >= N - r
    few = T[:17]
    ref = A.adj_ref(g[:5], few, pn["geno"], pn["pheno"], A.make_cov(R.N_ANIMALS, 16), A.H2, "snp", snps=[3])
    assert ref["dof"] == 0 and np.all(np.isnan(ref["u"])) and np.all(np.isnan(ref["loglik"]))


def test_estimate_inputs_separate_the_two_models():
    """The phenotype of the estimate_h2 test: the estimate with Q differs from the one without by far more than
    the last round's step, on the restatement."""
    e = A.est_inputs()
    with_q = A.estimate_ref(e["genome"], e["T"], e["geno"], e["pheno"], e["cov"])
    without = A.estimate_ref(e["genome"], e["T"], e["geno"], e["pheno"], None)
    assert not with_q["at_bound"]
    assert abs(with_q["h2"] - without["h2"]) > 10 * max(with_q["step"], without["step"]), (with_q, without)


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


def test_engine_validates_covariates_before_any_call():
    eng = _engine()
    T, V, g = np.arange(30), np.arange(30, 40), [np.arange(5)]
    bad = [np.zeros((49, 2)), np.zeros((50, 17)), np.zeros((50, 0)), np.zeros((50, 2, 1)),
           np.full((50, 2), np.nan), np.full((50, 1), np.inf)]
    for q in bad:
        with pytest.raises(ValueError):
            eng.snp_scores(g, T, V, 0.4, [1, 2], covariates=q)
        with pytest.raises(ValueError):
            eng.log_likelihood_cov(g, T, V, 0.4, covariates=q)
        with pytest.raises(ValueError):
            eng.estimate_h2_cov(g, T, V, covariates=q)
    with pytest.raises(ValueError):
        eng.snp_scores(g, T, V, 0.4, [[1, 2]], covariates=np.zeros((50, 2)))


def test_snp_scores_carries_dof_and_cov_effects():
    from tblup_amd.model import SnpScores
    rng = np.random.default_rng(0)
    u, v, q = rng.standard_normal((2, 1, 3)), rng.random((2, 3)) + 1, rng.random((2, 1)) + 5
    b = rng.standard_normal((2, 1, 4))
    sc = SnpScores(u, v, q, np.array([94.0, 95.0]), [1, 2, 3], cov_effects=b)
    np.testing.assert_array_equal(sc.cov_effects, b)
    np.testing.assert_allclose(sc.effect(), u / v[:, None, :])
    np.testing.assert_allclose(sc.chi2(), u * u / (v[:, None, :] * (q / sc.dof[:, None])[:, :, None]))
    assert SnpScores(u, v, q, np.array([94.0, 95.0]), [1, 2, 3]).cov_effects is None
    with pytest.raises(ValueError):
        SnpScores(u, v, q, np.array([94.0, 95.0]), [1, 2, 3], cov_effects=b[:1])


def test_binding_header_and_library_declare_the_entries():
    from tblup_amd import _native
    want = {"tblup_snp_score_cov_batch": 16, "tblup_loglik_cov_batch": 14}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tblup_gpu.h")) as f:
        header = f.read()
    lib = _native.load()
    for name, nargs in want.items():
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
        assert "int %s(" % name in header
        assert hasattr(lib, name)
