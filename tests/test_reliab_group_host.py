"""The restatement behind tests/test_gpu_reliab_group.py, checked on the CPU, and the host side of the uncertainty
under a class fixed effect (no GPU).

  * tests/reliab_group_ref.py::mme_ref -- reliab_cov_ref's mixed-model-equation route in SNP space on
    group_ref.expand's design, float64 -- against the header's V-form in np.longdouble, within covar_ref.HOST_TOL of
    the largest |ref| (reliability, pev_total, fixed_cov), for every design x split x genome x branch of the GPU
    tests over all 331 animals.  mme_ref asserts what keeps the GPU tolerance meaningful: cond(G) <= COND_MAX and
    K_aa > 0; no case is skipped
  * the ordering reliability_group <= reliability_cov(Q alone) <= reliability() between three float64 restatements,
    up to HOST_TOL
  * fixed_cov's layout (the zero reference row under snp), the unseen label's NaN pev_total, and a narrow design being
    the covariate restatement of [Q, Z]
  * GroupReliability and its two stderr methods, the signatures, the refusals' wording, the binding and the header
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tests import reliab_cov_ref as Q
from tests import reliab_group_ref as RG
from tests import reliability_ref as RQ

N = R.N_ANIMALS


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / float(np.max(np.abs(ref))))


@pytest.mark.parametrize("name", list(RG.DESIGNS))
def test_mme_route_against_the_v_form_in_longdouble(name):
    pn = RG.panel()
    L, c = RG.DESIGNS[name]
    worst, cond, n_cases = 0.0, 0.0, 0
    for s in RG.DESIGN_SPLITS[name]:
        T, _ = pn["splits"][s]
        cov, g = RG.design_inputs(name, s)
        for key in RG.HOST_KEYS:
            for br in ("auto", "gblup", "snp"):
                args = (pn["genomes"][key], T, pn["geno"], cov, g, RG.H2, br)
                ref = RG.mme_ref(*args)                     # asserts cond(G) <= COND_MAX and K_aa > 0
                snp = ref["branch"] == "snp"
                assert ref["cov_cov"].shape == (c + L - snp,) * 2 and ref["fixed_cov"].shape == (c + L,) * 2
                for f in ("rel", "pev", "fixed_cov"):
                    assert np.all(np.isfinite(ref[f])), (name, s, key, br, f)
                assert np.all(ref["pev"] > 0) and np.all(np.diag(ref["cov_cov"]) > 0)
                wide = RG.vform_wide(*args)
                for f in ("rel", "pev", "fixed_cov"):
                    worst = max(worst, _rel(ref[f], wide[f]))
                cond = max(cond, float(np.linalg.cond(ref["cov_cov"])))
                n_cases += 1
    print("\nRELIAB-GROUP host %s: %d cases, float64 MME vs longdouble V-form %.3e, worst cond(G) %.3e"
          % (name, n_cases, worst, cond))
    assert n_cases == 12 * len(RG.DESIGN_SPLITS[name])
    assert worst <= RG.HOST_TOL and cond <= RG.COND_MAX


@pytest.mark.parametrize("name,split,key,branch", [("L18", (129, 64), 64, "auto"), ("L40c3", (257, 70), 332, "auto"),
                                                   ("L113c15", (257, 70), 200, "snp")])
def test_ordering_of_the_three_reliabilities(name, split, key, branch):
    pn = RG.panel()
    T, _ = pn["splits"][split]
    cov, g = RG.design_inputs(name, split)
    idx = pn["genomes"][key]
    grp = RG.case_ref(name, split, key, branch)["rel"]
    plain = RQ.rel_ref(idx, T, pn["geno"], RG.H2, branch)
    mid = plain if cov is None else Q.mme_ref(idx, T, pn["geno"], cov, RG.H2, branch)["rel"]
    assert np.all(grp <= mid + RG.HOST_TOL) and np.all(mid <= plain + RG.HOST_TOL)
    assert float(np.max(mid - grp)) > 1e-6                  # the factor is not free


def test_layout_unseen_labels_and_the_narrow_design():
    pn = RG.panel()
    T, V = pn["splits"][129, 64]
    idx = pn["genomes"][64]                                  # snp under auto
    cov, g = C.make_cov(N, 2), RG.make_groups(N, 3, T)
    out = RG.mme_ref(idx, T, pn["geno"], cov, g, RG.H2)
    X, lev = RG.design(idx, T, pn["geno"], cov, g)
    flat = Q.mme_ref(idx, T, pn["geno"], X, RG.H2)
    assert X.shape[1] == 4 and len(lev) == 3 and not np.any(out["unseen"])
    np.testing.assert_array_equal(out["rel"], flat["rel"])
    np.testing.assert_array_equal(out["pev"], flat["pev"])
    fc = out["fixed_cov"]
    assert fc.shape == (5, 5) and np.all(fc[2] == 0) and np.all(fc[:, 2] == 0)
    np.testing.assert_array_equal(fc[np.ix_([0, 1, 3, 4], [0, 1, 3, 4])], flat["cov_cov"])
    gb = RG.mme_ref(pn["genomes"][332], T, pn["geno"], cov, g, RG.H2)
    assert gb["branch"] == "gblup" and np.all(np.diag(gb["fixed_cov"]) > 0)
    # a label that no train animal has, on animals outside the split
    out_rows = np.setdiff1d(np.arange(N), np.concatenate([T, V]))[:3]
    g2 = g.copy()
    g2[out_rows] = 77
    lst = np.concatenate([out_rows, T[:2]])
    un = RG.mme_ref(idx, T, pn["geno"], cov, g2, RG.H2, animals=lst)
    assert list(un["unseen"]) == [True] * 3 + [False] * 2
    assert np.all(np.isnan(un["pev"][:3])) and np.all(np.isfinite(un["pev"][3:])) and np.all(np.isfinite(un["rel"]))
    np.testing.assert_array_equal(un["rel"], out["rel"][lst])   # the reliability needs no design row


# ---------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_signatures():
    from tblup_amd.engine import GpuBlupEngine as E
    from tblup_amd.evaluator import BlupParallelEvaluator as V
    none, empty = None, inspect.Parameter.empty
    assert _params(E.reliability_group) == [
        ("genomes", empty), ("train", empty), ("valid", empty), ("h2", empty), ("animals", empty), ("groups", empty),
        ("covariates", none), ("branch", "auto"), ("return_pev", False), ("return_fixed_cov", False),
        ("return_models", False)]
    assert [n for n, _ in _params(V.reliability_group)][:3] == ["population", "animals", "groups"]
    # the pinned signatures stay
    assert [n for n, _ in _params(E.reliability)] == ["genomes", "train", "valid", "h2", "animals", "branch"]
    assert [n for n, _ in _params(E.reliability_cov)][-1] == "groups"


def test_the_refusals_name_the_new_method():
    from tblup_amd.engine import GpuBlupEngine as E
    with pytest.raises(ValueError, match=r"reliability_group\(\)"):
        E._no_groups([1], "reliability_cov()")
    with pytest.raises(ValueError, match="groups"):
        E._no_groups([1], "reliability_cov()")
    with pytest.raises(ValueError, match=r"reliability_group\(\)"):
        E._no_groups([1], "evaluate()")
    e = object.__new__(E)
    e.n_animals, e.n_snps, e.n_traits, e._ctx, e._pending = 40, 50, 1, None, None
    T, V, g = np.arange(30), np.arange(30, 40), np.arange(40) % 4
    with pytest.raises(ValueError, match="reliability_group"):
        e.fit([np.arange(5)], T, V, 0.4, reliability_of=[1, 2], groups=g)
    with pytest.raises(ValueError, match="reliability_group"):
        e.reliability_cov([np.arange(5)], T, V, 0.4, [1, 2], np.zeros((40, 2)), groups=g)
    # validation before any call: the animal list, the labels, the column limit
    with pytest.raises(ValueError):
        e.reliability_group([np.arange(5)], T, V, 0.4, [[1, 2]], g)
    for wrong in (g[:-1], g.astype(np.float64), np.stack([g, g], axis=1)):
        with pytest.raises(ValueError):
            e.reliability_group([np.arange(5)], T, V, 0.4, [1, 2], wrong)
    unseen = g.copy()
    unseen[V[2]] = 99
    with pytest.raises(ValueError, match="99"):
        e.reliability_group([np.arange(5)], T, V, 0.4, [1, 2], unseen)
    e.n_animals = 400
    with pytest.raises(ValueError, match="129"):
        e.reliability_group([np.arange(10)], np.arange(300), np.arange(300, 400), 0.4, [1], np.arange(400) % 113,
                            covariates=np.ones((400, 16)), branch="gblup")


def test_group_reliability_and_its_standard_errors():
    from tblup_amd.model import GroupReliability
    rng = np.random.default_rng(1)
    rel, pev = rng.random((2, 5)), rng.random((2, 5))
    a = rng.standard_normal((2, 6, 6))
    fc = a @ np.swapaxes(a, 1, 2) + np.eye(6)
    lev = np.array(["a", "b", "c", "d"])
    r = GroupReliability(rel, lev, 2, pev, fc)
    assert r.models is None and r.n_cov == 2 and list(r.group_levels) == list(lev)
    np.testing.assert_array_equal(r.reliability, rel)
    np.testing.assert_array_equal(r.pev_total, pev)
    s2 = np.array([2.0, 0.5])
    diag = np.stack([np.diag(fc[0]), np.diag(fc[1])])
    got_c, got_g = r.cov_stderr(s2), r.group_stderr(s2)
    assert got_c.shape == (2, 1, 2) and got_g.shape == (2, 1, 4)
    np.testing.assert_allclose(got_c[:, 0], np.sqrt(s2[:, None] * diag[:, :2]), rtol=1e-15)
    np.testing.assert_allclose(got_g[:, 0], np.sqrt(s2[:, None] * diag[:, 2:]), rtol=1e-15)
    s2t = np.array([[2.0, 1.0, 3.0], [0.5, 0.25, 1.0]])
    assert r.cov_stderr(s2t).shape == (2, 3, 2) and r.group_stderr(s2t).shape == (2, 3, 4)
    np.testing.assert_allclose(r.group_stderr(s2t)[1, 2], np.sqrt(diag[1, 2:]), rtol=1e-15)
    # no covariates: an empty covariate block; the reference level's zero gives a zero error
    fz = fc[:, 2:, 2:].copy()
    fz[:, 0, :] = fz[:, :, 0] = 0.0
    r0 = GroupReliability(rel, lev, 0, None, fz)
    assert r0.cov_stderr(s2).shape == (2, 1, 0) and np.all(r0.group_stderr(s2)[:, :, 0] == 0)
    assert np.all(np.isnan(GroupReliability(rel, lev, 2, None, np.full((2, 6, 6), np.nan)).group_stderr(s2)))
    with pytest.raises(ValueError):
        GroupReliability(rel, lev).group_stderr(s2)
    with pytest.raises(ValueError):
        r.group_stderr(np.ones(3))
    for bad in (dict(pev_total=pev[:1]), dict(fixed_cov=fc[:1]), dict(fixed_cov=fc[:, :5, :5]), dict(models=[None]),
                dict(n_cov=-1)):
        with pytest.raises(ValueError):
            GroupReliability(rel, lev, **{"n_cov": 2, **bad})
    with pytest.raises(ValueError):
        GroupReliability(rel[0], lev)
    with pytest.raises(ValueError):
        GroupReliability(rel, np.zeros((2, 2)))


def test_binding_header_and_null_context():
    from tblup_amd import _native
    name = "tblup_reliability_group_batch"
    assert len(_native.SIGNATURES[name][1]) == 24
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "tblup_gpu.h")).read()
    assert re.search(r"int %s\(" % name, header)
    assert "fixed_cov" in header and "f~_a" in header
    lib = _native.load()
    assert hasattr(lib, name)
    # a null context is a status, not a crash
    z = np.zeros(4, dtype=np.int64)
    i64 = ctypes.POINTER(ctypes.c_int64)
    assert getattr(lib, name)(None, 0, None, 0, z.ctypes.data_as(i64), 1, None, 0, None, None, 0, 0.4, 0,
                              *([None] * 11)) != 0
