"""Reliabilities, the error variance of predicted records and the sampling covariance of the fixed effects under the
model with a class fixed effect (tblup_reliability_group_batch: k_fixed_subst and k_fixed_gls in keep mode, k_reliab's
wide-design instances, k_fixed_cov; a model of up to 16 columns through tblup_reliability_cov_batch) on the GPU, against
tests/reliab_group_ref.py: reliab_cov_ref's mixed-model equations in SNP space on group_ref.expand's design (within
1e-11 of the header's V-form in longdouble: tests/test_reliab_group_host.py).

Panels: group_ref's 331 x 600 with the designs L18 (17 / 18 columns: one column in a second slab), L40c3 (a partial
last slab) and L113c15 (127 / 128 columns, the limit) on their splits; the deeper 700 x 800 panel with 40 levels; the
1200 x 1100 panel with 24 levels + 3 covariates whose systems have exactly 1024 rows (right-hand sides in LDS) and 1152.

  A  against the restatement, all animals as the list: the auto branch on the ragged batch AUTO_KEYS (kernel form,
     gblup and snp models of different C_m in one call) and each genome of k <= n_T alone (SNP form), forced gblup,
     forced snp at k > n_T, the deeper panel; reliability, pev_total, fixed_cov with its zero reference row under snp
  B  the 1200 x 1100 panel: 1024 and 1152 rows, with and without TBLUP_RELIAB_LDS=0
  C  animal lists of length 1, 15, 16, 17, 33 with repeats and rows outside the split: the all-animal call's bits
  D  the same bits with TBLUP_WORKSPACE_MB=1, for the call twice, for a model alone against inside a batch
  E  four traits: one value per (model, animal); with return_models the models are fit(groups=)'s bit for bit
  F  a design of <= 16 columns is reliability_cov(covariates=[Q, Z]) bit for bit; reliability_group <=
     reliability_cov(Q alone) <= reliability() up to TOL; one level: fixed_cov against cov_cov; string labels;
     group_stderr finite and positive for fitted levels
  G  an unseen label on a listed animal (finite reliability, NaN pev_total), a covariate equal to a level's indicator
     (NaN model), 113 levels + 15 covariates on 127 train animals (NaN), a monomorphic panel and K_aa = 0, the argument
     errors, the empty batch and the empty list
  H  BlupParallelEvaluator.reliability_group

Tolerance: |got - ref| <= 1e-9 max(1, max |ref|) (tests/score_ref.py::TOL) over the model's animals, over the matrix
for fixed_cov.  Each group prints the largest error it saw (pytest -s); no printed figure is a threshold.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tests import reliab_cov_ref as Q
from tests import reliab_group_ref as RG
from tests import score_cov_ref as A
from tests import score_ref as S
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = RG.H2
TOL = RG.TOL
N, P = R.N_ANIMALS, R.N_SNPS
HERD = np.arange(N)
I64, F64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
ALL = dict(return_pev=True, return_fixed_cov=True)
FIELDS = ("reliability", "pev_total", "fixed_cov")


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = S.close(got, ref)
        self.v = max(self.v, err)
        print("  %-52s %.3e" % (name, err))
        assert err <= TOL, (name, err)

    def check(self, got, b, ref, name, an=None):
        """model b of a GroupReliability against a reliab_group_ref.mme_ref dictionary (an: the listed animals of an
        all-animal ref; every listed animal has a fitted label)."""
        rel, pev = (ref["rel"], ref["pev"]) if an is None else (ref["rel"][an], ref["pev"][an])
        self.close(got.reliability[b], rel, name + " rel")
        self.close(got.pev_total[b], pev, name + " pev")
        fc = got.fixed_cov[b]
        self.close(fc, ref["fixed_cov"], name + " fixed_cov")
        np.testing.assert_array_equal(fc, fc.T, err_msg=name)
        if ref["branch"] == "snp":      # the reference level: exact zeros
            assert np.all(fc[got.n_cov] == 0) and np.all(fc[:, got.n_cov] == 0), name
        keep = [j for j in range(fc.shape[0]) if not (ref["branch"] == "snp" and j == got.n_cov)]
        assert np.all(np.diag(fc)[keep] > 0), name

    def show(self):
        print("\nRELIAB-GROUP %s: worst error / max(1, max |ref|) %.3e" % (self.label, self.v))


def _same(a, b, msg=""):
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f + " " + msg)


@pytest.fixture(scope="module")
def eng(gpu):
    pn = RG.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RG.DESIGNS))
def test_a_auto_branch(eng, name):
    pn = RG.panel()
    L, c = RG.DESIGNS[name]
    genomes = [pn["genomes"][k] for k in RG.AUTO_KEYS]
    w = _Worst("A auto " + name)
    for s in RG.DESIGN_SPLITS[name]:
        T, V = pn["splits"][s]
        cov, g = RG.design_inputs(name, s)
        batch = eng.reliability_group(genomes, T, V, H2, HERD, g, covariates=cov, **ALL)
        assert batch.reliability.shape == (len(genomes), N) and batch.fixed_cov.shape == (len(genomes), c + L, c + L)
        assert batch.models is None and batch.n_cov == c and len(batch.group_levels) == L
        for i, k in enumerate(RG.AUTO_KEYS):
            ref = RG.case_ref(name, s, k, "auto")
            assert ref["branch"] == ("gblup" if k > N else "snp")
            w.check(batch, i, ref, "%s %s k=%d (batch)" % (name, s, k))
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                one = eng.reliability_group([genomes[i]], T, V, H2, HERD, g, covariates=cov, **ALL)
                w.check(one, 0, ref, "%s %s k=%d (alone)" % (name, s, k))
    w.show()


@pytest.mark.parametrize("name", list(RG.DESIGNS))
def test_a_forced_branches(eng, name):
    pn = RG.panel()
    w = _Worst("A forced " + name)
    for s in RG.DESIGN_SPLITS[name]:
        T, V = pn["splits"][s]
        cov, g = RG.design_inputs(name, s)
        for br, keys in (("gblup", RG.GBLUP_KEYS), ("snp", RG.snp_keys(s[0]))):   # snp at k > n_T: the kernel form
            got = eng.reliability_group([pn["genomes"][k] for k in keys], T, V, H2, HERD, g, covariates=cov, branch=br,
                                        **ALL)
            for i, k in enumerate(keys):
                w.check(got, i, RG.case_ref(name, s, k, br), "%s %s %s k=%d" % (name, s, br, k))
    w.show()


def test_a_deeper_panel(gpu):
    dp = RG.deep_panel()
    n = len(dp["pheno"])
    cov, g = RG.deep_inputs()
    w = _Worst("A deep")
    with _engine(dp["geno"], dp["pheno"]) as e:
        got = e.reliability_group([dp["genome"]], dp["train"], dp["valid"], H2, np.arange(n), g, covariates=cov, **ALL)
    w.check(got, 0, RG.deep_ref(), "deep")
    w.show()


# ---------------------------------------------------------------------------------------------
# B. LDS at its limit and the workspace path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in A.big_cases()])
def test_b_systems_of_1024_rows_and_above(gpu, name):
    bp = RG.big_panel()
    _, gk, t, v, _, br, rows, lds = next(x for x in A.big_cases() if x[0] == name)
    cov, g = RG.big_inputs(t)
    ref = RG.big_ref(name)                                  # asserts cond(G) <= COND_MAX and K_aa > 0
    herd = np.arange(A.BIG_N)
    w = _Worst("B " + name)
    got = {}
    for knob in ("1", "0"):
        with _engine(bp["geno"], bp["pheno"], {"TBLUP_RELIAB_LDS": knob}) as e:
            got[knob] = e.reliability_group([bp[gk]], bp[t], bp[v], H2, herd, g, covariates=cov, branch=br, **ALL)
    w.check(got["1"], 0, ref, "%s (%d rows)" % (name, rows))
    _same(got["0"], got["1"], "TBLUP_RELIAB_LDS=0")
    w.show()


# ---------------------------------------------------------------------------------------------
# C. animal lists
# ---------------------------------------------------------------------------------------------
def test_c_animal_lists(eng):
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    cov, g = RG.design_inputs("L40c3", s)
    genomes = [pn["genomes"][k] for k in (64, 200, 332, 400)]            # kernel form (332, 400: gblup)
    snp_form = [pn["genomes"][k] for k in (64, 200)]
    full = {0: eng.reliability_group(genomes, T, V, H2, HERD, g, covariates=cov, **ALL),
            1: eng.reliability_group(snp_form, T, V, H2, HERD, g, covariates=cov, **ALL)}
    outside = np.setdiff1d(HERD, np.concatenate([T, V]))
    assert len(outside) > 0
    for m in RG.LIST_LENGTHS:
        lst = RG.animal_list(N, T, m)
        if m >= 2:
            lst[1] = outside[m % len(outside)]            # in no split role at all
        for which, batch in ((0, genomes), (1, snp_form)):
            got = eng.reliability_group(batch, T, V, H2, lst, g, covariates=cov, **ALL)
            assert got.reliability.shape == (len(batch), m) and got.pev_total.shape == (len(batch), m)
            np.testing.assert_array_equal(got.reliability, full[which].reliability[:, lst], err_msg=str(m))
            np.testing.assert_array_equal(got.pev_total, full[which].pev_total[:, lst], err_msg=str(m))
            np.testing.assert_array_equal(got.fixed_cov, full[which].fixed_cov, err_msg=str(m))
            if m >= 3:      # the list's last entry repeats its first
                np.testing.assert_array_equal(got.reliability[:, -1], got.reliability[:, 0])


# ---------------------------------------------------------------------------------------------
# D. the same bits
# ---------------------------------------------------------------------------------------------
def test_d_same_bits(eng):
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    cov, g = RG.design_inputs("L113c15", s)
    snp = [pn["genomes"][k] for k in (64, 127, 200)]                       # SNP form (every k <= n_T)
    mixed = snp + [pn["genomes"][400]]                                     # kernel form, both branches
    lst = RG.animal_list(N, T, 33)
    ref = {(i, j): eng.reliability_group(b, T, V, H2, a, g, covariates=cov, **ALL)
           for i, b in enumerate((snp, mixed)) for j, a in enumerate((HERD, lst))}
    _same(eng.reliability_group(snp, T, V, H2, lst, g, covariates=cov, **ALL), ref[0, 1], "twice")
    _same(eng.reliability_group(mixed, T, V, H2, lst, g, covariates=cov, **ALL), ref[1, 1], "twice")
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_WORKSPACE_MB": "1"}) as e:
        for i, b in enumerate((snp, mixed)):
            for j, a in enumerate((HERD, lst)):
                _same(e.reliability_group(b, T, V, H2, a, g, covariates=cov, **ALL), ref[i, j], "TBLUP_WORKSPACE_MB=1")
    # a model alone against inside a batch of the same form
    for b in (0, 2):
        one = eng.reliability_group([snp[b]], T, V, H2, lst, g, covariates=cov, **ALL)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(one, f)[0], getattr(ref[0, 1], f)[b], err_msg="alone " + f)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": "1"}) as e:
        one = e.reliability_group([mixed[1]], T, V, H2, lst, g, covariates=cov, **ALL)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(one, f)[0], getattr(ref[1, 1], f)[1], err_msg="alone, kernel form " + f)
    # the optional outputs change nothing in the ones that are asked for
    bare = eng.reliability_group(mixed, T, V, H2, lst, g, covariates=cov)
    assert bare.pev_total is None and bare.fixed_cov is None and bare.models is None
    np.testing.assert_array_equal(bare.reliability, ref[1, 1].reliability)
    _same(eng.reliability_group(mixed, T, V, H2, lst, g, covariates=cov, return_models=True, **ALL), ref[1, 1],
          "with the models")


# ---------------------------------------------------------------------------------------------
# E. traits
# ---------------------------------------------------------------------------------------------
def test_e_four_traits(gpu):
    pn = RG.panel()
    s = (129, 64)
    T, V = pn["splits"][s]
    cov, g = RG.design_inputs("L18", s)
    batches = [[pn["genomes"][k] for k in (64, 127)],                # SNP form
               [pn["genomes"][k] for k in (64, 200, 400)]]           # kernel form (k = 400: gblup)
    lst = RG.animal_list(N, T, 33)
    w = _Worst("E traits")
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, 0])) as e:
        single = [e.reliability_group(b, T, V, H2, lst, g, covariates=cov, **ALL) for b in batches]
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :4])) as e:
        for i, b in enumerate(batches):
            got = e.reliability_group(b, T, V, H2, lst, g, covariates=cov, return_models=True, **ALL)
            assert got.reliability.shape == (len(b), len(lst)) and got.fixed_cov.shape == (len(b), 18, 18)
            _same(got, single[i], "no phenotype enters")
            fitted = e.fit(b, T, V, H2, groups=g, covariates=cov)
            _, s2 = e.log_likelihood_group(b, T, V, H2, g, covariates=cov, return_sigma2=True)
            se = got.group_stderr(s2)
            assert se.shape == (len(b), 4, 18) and got.cov_stderr(s2).shape == (len(b), 4, 0)
            for m, gm in enumerate(b):
                for f in ("indices", "effects", "intercept", "center", "group_effects", "group_center", "group_levels"):
                    np.testing.assert_array_equal(getattr(got.models[m], f), getattr(fitted[m], f), err_msg=f)
                assert got.models[m].fitness == fitted[m].fitness and got.models[m].effects.shape == (4, len(gm))
                w.check(got, m, RG.mme_ref(gm, T, pn["geno"], cov, g, H2, animals=lst), "4 traits %d %d" % (i, m))
    w.show()


def test_e_models_are_fit_groups_models(eng):
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    lst = RG.animal_list(N, T, 17)
    for name in ("L40c3", "L113c15"):
        cov, g = RG.design_inputs(name, s)
        for genomes in ([pn["genomes"][k] for k in (64, 200)], [pn["genomes"][k] for k in RG.AUTO_KEYS]):
            got = eng.reliability_group(genomes, T, V, H2, lst, g, covariates=cov, return_models=True)
            fitted = eng.fit(genomes, T, V, H2, groups=g, covariates=cov)
            assert len(got.models) == len(fitted)
            for a, b in zip(got.models, fitted):
                for f in ("indices", "effects", "intercept", "center", "cov_effects", "cov_center", "group_effects",
                          "group_center", "group_levels"):
                    np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=name + " " + f)
                assert a.fitness == b.fitness and a.branch == b.branch


# ---------------------------------------------------------------------------------------------
# F. against the other entries
# ---------------------------------------------------------------------------------------------
def test_f_a_narrow_design_is_the_covariate_entry(eng):
    """3 levels + 2 covariates: 4 columns under snp, 5 under gblup -- tblup_reliability_cov_batch on [Q, Z] bit for
    bit, fixed_cov its cov_cov at the model's columns; and 14 levels + 2 covariates, where the gblup models have
    exactly 16 columns."""
    pn = RG.panel()
    T, V = pn["splits"][129, 64]
    lst = RG.animal_list(N, T, 33)
    genomes = [pn["genomes"][k] for k in RG.AUTO_KEYS]
    w = _Worst("F narrow")
    for L in (3, 14):
        cov, g = C.make_cov(N, 2), RG.make_groups(N, L, T)
        got = eng.reliability_group(genomes, T, V, H2, lst, g, covariates=cov, return_models=True, **ALL)
        fitted = eng.fit(genomes, T, V, H2, groups=g, covariates=cov)
        for i, k in enumerate(RG.AUTO_KEYS):
            br = "gblup" if k > N else "snp"
            X, _ = RG.G.expand(cov, g, T, br)
            flat = eng.reliability_cov([genomes[i]], T, V, H2, lst, covariates=X, branch=br, return_pev=True,
                                       return_cov_cov=True)
            np.testing.assert_array_equal(got.reliability[i], flat.reliability[0])
            np.testing.assert_array_equal(got.pev_total[i], flat.pev_total[0])
            keep = [j for j in range(2 + L) if not (br == "snp" and j == 2)]
            np.testing.assert_array_equal(got.fixed_cov[i][np.ix_(keep, keep)], flat.cov_cov[0])
            np.testing.assert_array_equal(got.models[i].group_effects, fitted[i].group_effects)
            np.testing.assert_array_equal(got.models[i].effects, fitted[i].effects)
            w.check(got, i, RG.mme_ref(genomes[i], T, pn["geno"], cov, g, H2, animals=lst), "L=%d k=%d" % (L, k))
    w.show()


def test_f_ordering_one_level_strings_and_stderr(eng):
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    genomes = [pn["genomes"][k] for k in RG.AUTO_KEYS]
    w = _Worst("F other entries")
    # reliability_group <= reliability_cov(Q alone) <= reliability()
    for name in ("L40c3", "L113c15"):
        cov, g = RG.design_inputs(name, s)
        grp = eng.reliability_group(genomes, T, V, H2, HERD, g, covariates=cov, **ALL)
        mid = eng.reliability_cov(genomes, T, V, H2, HERD, covariates=cov).reliability
        plain = eng.reliability(genomes, T, V, H2, HERD)
        assert np.all(grp.reliability <= mid + TOL), (name, float(np.max(grp.reliability - mid)))
        assert np.all(mid <= plain + TOL) and np.all(grp.pev_total > 0)
        # the standard errors of the fitted levels: finite and positive (0 at the reference level under snp)
        _, s2 = eng.log_likelihood_group(genomes, T, V, H2, g, covariates=cov, return_sigma2=True)
        se, sc = grp.group_stderr(s2), grp.cov_stderr(s2)
        assert se.shape == (len(genomes), 1, len(grp.group_levels)) and sc.shape == (len(genomes), 1, grp.n_cov)
        assert np.all(np.isfinite(se)) and np.all(np.isfinite(sc)) and np.all(sc > 0)
        for i, k in enumerate(RG.AUTO_KEYS):
            assert np.all(se[i, 0, 1:] > 0) and (se[i, 0, 0] > 0) == (k > N), (name, k)
    # string labels: the levels are np.unique's, the values the integer codes' bit for bit
    cov, g = RG.design_inputs("L40c3", s)
    names = np.array(["herd%03d" % v for v in g])
    a = eng.reliability_group(genomes, T, V, H2, HERD[:40], names, covariates=cov, **ALL)
    b = eng.reliability_group(genomes, T, V, H2, HERD[:40], g, covariates=cov, **ALL)
    _same(a, b, "string labels")
    assert a.group_levels.dtype.kind == "U" and list(a.group_levels) == ["herd%03d" % v for v in range(40)]
    # one level: under snp the factor drops out (the covariate model), under gblup it is a column of ones
    q5, one = C.make_cov(N, 5), np.zeros(N, dtype=np.int64)
    for br, ks in (("snp", (64, 200)), ("gblup", (64, 200))):
        gs = [pn["genomes"][k] for k in ks]
        got = eng.reliability_group(gs, T, V, H2, HERD[:20], one, covariates=q5, branch=br, **ALL)
        qx = q5 if br == "snp" else np.ascontiguousarray(np.hstack([q5, np.ones((N, 1))]))
        flat = eng.reliability_cov(gs, T, V, H2, HERD[:20], covariates=qx, branch=br, return_pev=True,
                                   return_cov_cov=True)
        assert got.fixed_cov.shape == (2, 6, 6)
        w.close(got.fixed_cov[:, :5, :5], flat.cov_cov[:, :5, :5], "one level, %s: covariate block" % br)
        w.close(got.reliability, flat.reliability, "one level, %s: rel" % br)
        w.close(got.pev_total, flat.pev_total, "one level, %s: pev" % br)
        if br == "snp":
            assert np.all(got.fixed_cov[:, 5] == 0) and np.all(got.fixed_cov[:, :, 5] == 0)
    w.show()


# ---------------------------------------------------------------------------------------------
# G. edges
# ---------------------------------------------------------------------------------------------
def test_g_unseen_label_on_a_listed_animal(eng):
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    outside = np.setdiff1d(HERD, np.concatenate([T, V]))[:2]
    lst = np.array([int(outside[0]), int(T[0]), int(outside[1]), int(V[0])], dtype=np.int64)
    w = _Worst("G unseen label")
    for name, keys in (("L40c3", RG.AUTO_KEYS), ("L40c3", (64, 200))):       # kernel form, SNP form
        cov, g = RG.design_inputs(name, s)
        g2 = g.copy()
        g2[outside] = 9999
        genomes = [pn["genomes"][k] for k in keys]
        got = eng.reliability_group(genomes, T, V, H2, lst, g2, covariates=cov, **ALL)
        base = eng.reliability_group(genomes, T, V, H2, lst, g, covariates=cov, **ALL)
        np.testing.assert_array_equal(got.reliability, base.reliability)     # it needs no design row
        assert np.all(np.isfinite(got.reliability))
        assert np.all(np.isnan(got.pev_total[:, [0, 2]]))
        np.testing.assert_array_equal(got.pev_total[:, [1, 3]], base.pev_total[:, [1, 3]])
        np.testing.assert_array_equal(got.fixed_cov, base.fixed_cov)
        for i, k in enumerate(keys):
            ref = RG.mme_ref(genomes[i], T, pn["geno"], cov, g2, H2, animals=lst)
            w.close(got.reliability[i], ref["rel"], "k=%d rel" % k)
            w.close(got.pev_total[i, [1, 3]], ref["pev"][[1, 3]], "k=%d pev" % k)
    # a narrow design takes the same rule
    cov, g = C.make_cov(N, 2), RG.make_groups(N, 3, T)
    g[outside] = 9999
    got = eng.reliability_group([pn["genomes"][64]], T, V, H2, lst, g, covariates=cov, **ALL)
    assert np.all(np.isfinite(got.reliability)) and np.all(np.isnan(got.pev_total[0, [0, 2]]))
    assert np.all(np.isfinite(got.pev_total[0, [1, 3]]))
    # on a validation row it stays an error
    g[V[3]] = 9999
    with pytest.raises(ValueError, match="9999"):
        eng.reliability_group([pn["genomes"][64]], T, V, H2, lst, g, covariates=cov)
    w.show()


def test_g_collinear_designs_give_nan(eng):
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    cov, g = RG.design_inputs("L40c3", s)
    bad = cov.copy()
    bad[:, 1] = (g == 7)                                    # a covariate equal to a level's indicator
    for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][400]]):    # SNP form, kernel form
        got = eng.reliability_group(genomes, T, V, H2, [3, 4, 5], g, covariates=bad, return_models=True, **ALL)
        for f in FIELDS:
            assert np.all(np.isnan(getattr(got, f))), f
        assert all(np.all(np.isnan(m.group_effects)) and np.all(np.isnan(m.effects)) for m in got.models)
    # 113 levels + 15 covariates on 127 train animals: more columns than records
    T, V = pn["splits"][127, 5]
    cov = C.make_cov(N, 15)
    g = RG.make_groups(N, 113, T)
    got = eng.reliability_group([pn["genomes"][64], pn["genomes"][400]], T, V, H2, [3, 4, 5], g, covariates=cov, **ALL)
    for f in FIELDS:
        assert np.all(np.isnan(getattr(got, f))), f


def test_g_monomorphic_panel_and_an_animal_with_zero_k_aa(gpu):
    pn = RG.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][128, 2]
    # column 2: mean exactly 1 over the 128 train rows, and a candidate outside the split that sits on it
    geno[T[:64], 2] = 0
    geno[T[64:], 2] = 2
    a0 = int(np.setdiff1d(HERD, np.concatenate([T, V]))[0])
    geno[a0, 2] = 1
    geno[V[0], 2] = 2
    cov, g = RG.design_inputs("L40c3", (128, 2))
    lst = np.array([int(T[0]), a0, int(V[0]), a0], dtype=np.int64)
    for form in ("2", "1"):
        with _engine(geno, pn["pheno"], {"TBLUP_FORM": form}) as e:
            genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64], np.array([2])]
            got = e.reliability_group(genomes, T, V, H2, lst, g, covariates=cov, branch="snp", **ALL)
            for f in FIELDS:
                assert np.all(np.isnan(getattr(got, f)[:2])), (form, f)
            ref = RG.mme_ref(genomes[2], T, geno, cov, g, H2, "snp", animals=lst)
            _Worst("G beside the NaN models").check(got, 2, ref, "form " + form)
            # K_aa = 0: NaN for that animal alone
            assert np.all(np.isnan(got.reliability[3, [1, 3]])) and np.all(np.isnan(got.pev_total[3, [1, 3]])), form
            assert np.all(np.isfinite(got.reliability[3, [0, 2]])) and np.all(np.isfinite(got.fixed_cov[3])), form
            one = RG.mme_ref(genomes[3], T, geno, cov, g, H2, "snp", animals=lst[[0, 2]])
            w = _Worst("G beside the K_aa = 0 animal")
            w.close(got.reliability[3, [0, 2]], one["rel"], "rel form " + form)
            w.close(got.pev_total[3, [0, 2]], one["pev"], "pev form " + form)


def test_g_errors_and_empty_lists(eng):
    from tblup_amd import _native
    from tblup_amd._native import TblupError, TblupIndexError
    from tblup_amd.engine import concat_genomes
    pn = RG.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    gen = [pn["genomes"][64]]
    cov, g = RG.design_inputs("L40c3", s)
    with pytest.raises(TblupIndexError):
        eng.reliability_group([np.array([0, P])], T, V, H2, [1], g, covariates=cov)
    with pytest.raises(TblupError):
        eng.reliability_group(gen, T, V, H2, [0, N], g, covariates=cov)
    for wrong in (g[:-1], g.astype(np.float64), np.stack([g, g], axis=1)):      # shape, float labels
        with pytest.raises(ValueError):
            eng.reliability_group(gen, T, V, H2, [1], wrong, covariates=cov)
    with pytest.raises(ValueError, match="129"):                                 # 113 levels + 16 covariates, gblup
        eng.reliability_group(gen, T, V, H2, [1], RG.make_groups(N, 113, T), covariates=C.make_cov(N, 16),
                              branch="gblup")
    # empty lists: no animals -- fixed_cov and the models are still filled; no models -- empty arrays
    empty = eng.reliability_group(gen * 3, T, V, H2, [], g, covariates=cov, return_models=True, **ALL)
    assert empty.reliability.shape == (3, 0) and empty.pev_total.shape == (3, 0)
    full = eng.reliability_group(gen * 3, T, V, H2, [1, 2], g, covariates=cov, return_models=True, **ALL)
    np.testing.assert_array_equal(empty.fixed_cov, full.fixed_cov)
    assert np.all(np.isfinite(empty.fixed_cov))
    np.testing.assert_array_equal(empty.models[2].group_effects, full.models[2].group_effects)
    only_fc = eng.reliability_group(gen * 3, T, V, H2, [], g, covariates=cov, return_fixed_cov=True)
    np.testing.assert_array_equal(only_fc.fixed_cov, full.fixed_cov)
    bare = eng.reliability_group(gen * 3, T, V, H2, [], g, covariates=cov)
    assert bare.reliability.shape == (3, 0) and bare.fixed_cov is None
    for kw in ({}, ALL):
        none = eng.reliability_group([], T, V, H2, [1, 2], g, covariates=cov, return_models=True, **kw)
        assert none.reliability.shape == (0, 2) and none.models == []
        assert none.fixed_cov is None or none.fixed_cov.shape == (0, 43, 43)
    # the entry's own argument checks
    idx, off = concat_genomes(gen)
    lst = np.array([1, 2], dtype=np.int64)
    rel = np.empty((1, 2))
    sid = eng.split_id(T, V)
    codes = np.ascontiguousarray(g, dtype=np.int64)

    def call(ctx, q, nc, grp=codes, L=40, animals=lst, rel_out=rel, **out):
        ptr = {k: v.ctypes.data_as(F64) for k, v in out.items()}
        return eng._lib.tblup_reliability_group_batch(
            ctx, sid, None if q is None else q.ctypes.data_as(F64), nc, None if grp is None else grp.ctypes.data_as(I64),
            L, animals.ctypes.data_as(I64), len(animals), idx.ctypes.data_as(I64), off.ctypes.data_as(I64), 1, H2, 0,
            None, ptr.get("cov_effects"), ptr.get("cov_center"), ptr.get("group_effects"), ptr.get("group_center"),
            ptr.get("intercept"), ptr.get("center"), ptr.get("effects"),
            None if rel_out is None else rel_out.ctypes.data_as(F64), None, None)
    err = eng._lib.tblup_last_error
    assert call(eng._ctx, np.zeros((N, 17)), 17) == _native.ERR_ARG and b"n_cov" in err()
    assert call(eng._ctx, None, 3) == _native.ERR_ARG
    nanq = cov.copy()
    nanq[7, 1] = np.nan
    assert call(eng._ctx, nanq, 3) == _native.ERR_ARG and b"finite" in err()
    assert call(eng._ctx, cov, 3, grp=None) == _native.ERR_ARG and b"group" in err()
    assert call(eng._ctx, cov, 3, L=0) == _native.ERR_ARG and b"n_levels" in err()
    assert call(eng._ctx, cov, 3, L=39) == _native.ERR_ARG and b"code" in err()           # a code of 39 with 39 levels
    assert call(eng._ctx, cov, 3, L=41) == _native.ERR_ARG and b"no train row" in err()
    hole = codes.copy()
    hole[V[1]] = -1
    assert call(eng._ctx, cov, 3, grp=hole) == _native.ERR_ARG and b"no level" in err()  # -1 on a validation row
    free = codes.copy()
    free[np.setdiff1d(HERD, np.concatenate([T, V]))] = -1
    assert call(eng._ctx, cov, 3, grp=free) == 0                                          # -1 outside the split
    for bad in (np.array([1, N], dtype=np.int64), np.array([-1, 2], dtype=np.int64)):
        assert call(eng._ctx, cov, 3, animals=bad) == _native.ERR_ARG and b"animal" in err()
    assert call(eng._ctx, cov, 3, rel_out=None) == _native.ERR_ARG
    assert call(eng._ctx, cov, 3, group_effects=np.empty((1, 1, 40))) == _native.ERR_ARG   # the group, or none of it
    assert call(eng._ctx, cov, 3) == 0
    assert call(eng._ctx, None, 0) == 0
    ctx = ctypes.c_void_p()
    assert eng._lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        assert call(ctx, cov, 3) == _native.ERR_STATE and b"panel" in err()
    finally:
        eng._lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# H. evaluator level
# ---------------------------------------------------------------------------------------------
def test_h_evaluator_reliability_group(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = RG.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, H2, False)
    rem.removed = np.array((5, 17, 301, 599), dtype=np.float64)
    cov = C.make_cov(N, 3)
    w = _Worst("H")
    with E.BlupParallelEvaluator(gp, pp, H2, snp_remover=rem) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        g = RG.make_groups(N, 30, train)
        lst = RG.animal_list(N, train, 33)
        got = ev.reliability_group(pop, lst, g, covariates=cov, **ALL)
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        _same(got, ev.engine.reliability_group(genomes, train, ev.testing_indices, H2, lst, g, covariates=cov, **ALL))
        for i, gm in enumerate(genomes):
            w.check(got, i, RG.mme_ref(gm, train, pn["geno"], cov, g, H2, animals=lst), "model %d" % i)
        assert np.all(got.reliability <= ev.reliability(pop, lst) + TOL)
    w.show()
