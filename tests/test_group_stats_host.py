"""The restatement behind tests/test_gpu_group_stats.py, checked on the CPU, and the host side of the score
statistics and the likelihood under a class fixed effect (no GPU).

  * tests/group_stats_ref.py is score_cov_ref on group_ref.expand's design: float64 against np.longdouble within
    score_ref.HOST_TOL of the largest |ref| (u_P, v_P, q_P, sigma2_g, b; l_R relative to max(1, |l_R|)), and the
    inputs keep the GPU tolerance meaningful -- v_P >= SPAN_MIN v for every SNP, cond(G) <= COND_MAX, every likelihood
    finite -- for every design x split x genome x branch of the GPU tests, over all 600 SNPs
  * the likelihood against the explicit-contrast computation (an SVD basis, no identity of the restatement) on an
    expanded design.  Bound: test_score_cov_host.py's ROUTE_TOL, for its reasons
  * the new names and defaults of the Python surface, SnpScores' new fields, the exported symbols and the header
  * the argument errors that need no device
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import covar_ref as C
from tests import group_stats_ref as GS
from tests import loglik_ref as LR
from tests import model_ref as R
from tests.test_score_cov_host import ROUTE_TOL

N = R.N_ANIMALS


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / float(np.max(np.abs(ref))))


@pytest.mark.parametrize("name", list(GS.DESIGNS))
def test_restatement_error_and_conditions(name):
    pn = GS.panel()
    worst = {"stat": 0.0, "loglik": 0.0, "span": np.inf, "cond": 0.0}
    L, c = GS.DESIGNS[name]
    for s in GS.DESIGN_SPLITS[name]:
        T, _ = pn["splits"][s]
        cov, g = GS.design_inputs(name, s)
        for key in GS.HOST_KEYS:
            for br in ("auto", "gblup", "snp"):
                args = (pn["genomes"][key], T, pn["geno"], pn["pheno"], cov, g, GS.H2, br)
                r64, wide = GS.adj_ref(*args), GS.adj_wide(*args)
                snp = GS.fitted_branch(pn["genomes"][key], pn["geno"], br) == "snp"
                assert r64["dof"] == len(T) - snp - (c + L - snp) and r64["b"].shape == (1, c + L - snp)
                if r64["dof"] <= 0:      # L113c15 has no such split here; L18 / L40c3 neither
                    continue
                for f in ("u", "v", "q", "sigma2_g", "b", "loglik"):
                    assert np.all(np.isfinite(r64[f])), (name, s, key, br, f)
                for f in ("u", "v", "q", "sigma2_g", "b"):
                    worst["stat"] = max(worst["stat"], _rel(r64[f], wide[f]))
                worst["loglik"] = max(worst["loglik"], LR.close(r64["loglik"], wide["loglik"].astype(np.float64)))
                worst["span"] = min(worst["span"], float(np.min(r64["v"] / r64["v_plain"])))
                worst["cond"] = max(worst["cond"], float(np.linalg.cond(r64["G"])))
    print("\nGROUP-STATS host %s: float64 vs longdouble %.3e (loglik %.3e), min v_P / v %.3e, worst cond(G) %.3e"
          % (name, worst["stat"], worst["loglik"], worst["span"], worst["cond"]))
    assert worst["stat"] <= GS.HOST_TOL and worst["loglik"] <= GS.HOST_TOL
    assert worst["span"] >= GS.SPAN_MIN and worst["cond"] <= GS.COND_MAX


@pytest.mark.parametrize("name,split,key,branch", [("L18", (129, 64), 64, "auto"), ("L40c3", (257, 70), 332, "auto"),
                                                   ("L40c3", (128, 2), 200, "snp"), ("L18", (127, 5), 64, "gblup")])
def test_likelihood_is_that_of_the_error_contrasts(name, split, key, branch):
    pn = GS.panel()
    T, _ = pn["splits"][split]
    cov, g = GS.design_inputs(name, split)
    for h2 in GS.H2S:
        ref = GS.case_ref(name, split, key, branch, h2, False)
        lc, qc = GS.contrast_ref(pn["genomes"][key], T, pn["geno"], pn["pheno"], cov, g, h2, branch)
        assert abs(lc - ref["loglik"][0]) <= ROUTE_TOL * max(1.0, abs(lc)), (name, h2, lc, ref["loglik"][0])
        assert abs(qc - ref["q"][0]) <= ROUTE_TOL * max(1.0, abs(qc)), (name, h2)
        assert abs(ref["sigma2_g"][0] - qc / ref["dof"]) <= ROUTE_TOL * max(1.0, abs(qc / ref["dof"]))


def test_a_narrow_design_is_the_covariate_restatement():
    """the expansion of 3 levels and 2 covariates is a 5-column (gblup) / 4-column (snp) covariate matrix"""
    from tests import score_cov_ref as A
    pn = GS.panel()
    T, _ = pn["splits"][129, 64]
    cov, g = C.make_cov(N, 2), GS.make_groups(N, 3, T)
    for key in (64, 332):
        X, lev = GS.design(pn["genomes"][key], T, pn["geno"], cov, g)
        assert X.shape[1] == (5 if key == 332 else 4) and len(lev) == 3
        a = GS.adj_ref(pn["genomes"][key], T, pn["geno"], pn["pheno"], cov, g, GS.H2, snps=[1, 2, 3])
        b = A.adj_ref(pn["genomes"][key], T, pn["geno"], pn["pheno"], X, GS.H2, snps=[1, 2, 3])
        for f in ("u", "v", "q", "loglik", "b"):
            np.testing.assert_array_equal(a[f], b[f])


def test_estimate_ref_on_the_expanded_design():
    e = GS.est_inputs()
    est = GS.estimate_ref(e["genome"], e["T"], e["geno"], e["pheno"], e["cov"], e["groups"], refine=1, points=5)
    assert 0.02 < est["h2"] < 0.98 and not est["at_bound"] and np.isfinite(est["loglik"])


# ---------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_engine_and_evaluator_surface():
    from tblup_amd.engine import GpuBlupEngine as E
    from tblup_amd.evaluator import BlupParallelEvaluator as V
    none, empty = None, inspect.Parameter.empty
    assert _params(E.snp_scores_group) == [("genomes", empty), ("train", empty), ("valid", empty), ("h2", empty),
                                           ("groups", empty), ("snps", none), ("branch", "auto"), ("covariates", none)]
    assert _params(E.log_likelihood_group) == [("genomes", empty), ("train", empty), ("valid", empty), ("h2", empty),
                                               ("groups", empty), ("covariates", none), ("branch", "auto"),
                                               ("return_sigma2", False)]
    est = _params(E.estimate_h2_group)
    assert [n for n, _ in est] == ["genomes", "train", "valid", "groups", "covariates", "branch", "grid", "refine", "points"]
    ref = dict(_params(E.estimate_h2_cov))
    got = dict(est)
    assert got["covariates"] is None and got["branch"] == "auto" and (got["refine"], got["points"]) == (3, 9)
    np.testing.assert_array_equal(got["grid"], ref["grid"])
    for name in ("snp_scores_group", "log_likelihood_group", "estimate_h2_group"):
        assert callable(getattr(V, name)), name
    assert [n for n, _ in _params(V.snp_scores_group)][:3] == ["population", "groups", "snps"]
    assert [n for n, _ in _params(V.log_likelihood_group)][:3] == ["population", "h2", "groups"]
    assert [n for n, _ in _params(V.estimate_h2_group)][:2] == ["population", "groups"]
    # the pinned signatures and the refusals stay
    assert [n for n, _ in _params(E.log_likelihood)] == ["genomes", "train", "valid", "h2", "branch", "return_sigma2"]
    assert [n for n, _ in _params(E.estimate_h2)] == ["genomes", "train", "valid", "branch", "grid", "refine", "points"]
    for what in ("snp_scores()", "log_likelihood_cov()", "estimate_h2_cov()", "reliability_cov()", "evaluate()"):
        with pytest.raises(ValueError, match="groups"):
            E._no_groups([1], what)
    with pytest.raises(ValueError, match="snp_scores_group"):
        E._no_groups([1], "snp_scores()")


def test_snp_scores_group_fields():
    from tblup_amd.model import SnpScores
    base = (np.zeros((2, 1, 3)), np.ones((2, 3)), np.ones((2, 1)), np.array([5.0, 6.0]), [1, 2, 3])
    plain = SnpScores(*base)
    assert plain.group_effects is None and plain.group_levels is None and plain.cov_effects is None
    sc = SnpScores(*base, group_effects=np.zeros((2, 1, 4)), group_levels=np.array(["a", "b", "c", "d"]))
    assert sc.group_effects.shape == (2, 1, 4) and list(sc.group_levels) == ["a", "b", "c", "d"] and sc.cov_effects is None
    with pytest.raises(ValueError):
        SnpScores(*base, group_effects=np.zeros((2, 1, 4)))                       # the two come together
    with pytest.raises(ValueError):
        SnpScores(*base, group_effects=np.zeros((2, 1, 4)), group_levels=[1, 2, 3])


def _stub(n):
    """an engine without a context: enough for the argument validation"""
    from tblup_amd.engine import GpuBlupEngine
    e = object.__new__(GpuBlupEngine)
    e.n_animals, e.n_snps, e._ctx, e._pending = n, 50, None, None
    return e


def test_argument_errors_without_a_device():
    e = _stub(40)
    T, V = np.arange(30), np.arange(30, 40)
    g = np.arange(40) % 6
    genomes = [np.arange(5), np.arange(45)]                      # snp, gblup (k > n)
    lev, codes, q, cols = e._group_design(genomes, T, V, "auto", np.ones((40, 2)), g)
    assert list(lev) == list(range(6)) and q.shape == (40, 2) and list(cols) == [7, 8]
    assert list(e._group_design(genomes, T, V, "snp", None, g)[3]) == [5, 5]
    for wrong in (g[:-1], g.astype(np.float64), np.stack([g, g], axis=1)):
        with pytest.raises(ValueError):
            e._group_design(genomes, T, V, "auto", None, wrong)
    unseen = g.copy()
    unseen[V[2]] = 99
    with pytest.raises(ValueError, match="99"):
        e._group_design(genomes, T, V, "auto", None, unseen)
    with pytest.raises(ValueError):
        e._group_design(genomes, T, V, "auto", np.full((40, 2), np.nan), g)
    # 129 columns: 113 levels + 16 covariates under gblup; 128 under snp pass
    e = _stub(400)
    T, V = np.arange(300), np.arange(300, 400)
    g113 = np.arange(400) % 113
    with pytest.raises(ValueError, match="129"):
        e._group_design([np.arange(10)], T, V, "gblup", np.ones((400, 16)), g113)
    assert list(e._group_design([np.arange(10)], T, V, "snp", np.ones((400, 16)), g113)[3]) == [128]
    with pytest.raises(ValueError, match="129"):
        e._group_design([np.arange(10), np.arange(10)], T, V, "gblup", np.ones((400, 16)), g113)


def test_binding_header_and_null_context():
    from tblup_amd import _native
    assert len(_native.SIGNATURES["tblup_snp_score_group_batch"][1]) == 19
    assert len(_native.SIGNATURES["tblup_loglik_group_batch"][1]) == 17
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "tblup_gpu.h")).read()
    for name in ("tblup_snp_score_group_batch", "tblup_loglik_group_batch"):
        assert re.search(r"int %s\(" % name, header), name
    assert "dof = N - r - C_m" in header and "log|F~_T^T F~_T|" in header
    lib = _native.load()
    assert hasattr(lib, "tblup_snp_score_group_batch") and hasattr(lib, "tblup_loglik_group_batch")
    # a null context is a status, not a crash
    z = np.zeros(4, dtype=np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    assert lib.tblup_snp_score_group_batch(None, 0, None, 0, z.ctypes.data_as(i64), 1, None, 0, None, None, 0, 0.4, 0,
                                           None, None, None, None, None, None) != 0
    assert lib.tblup_loglik_group_batch(None, 0, None, 0, z.ctypes.data_as(i64), 1, None, None, 0, None, 0, 0, None,
                                        None, None, None, None) != 0
