"""A class fixed effect in the fitted model (tblup_fit_group_batch; k_fixed_subst, k_fixed_gls, k_fixed_fitness)
on the GPU, against tests/group_ref.py: covar_ref's dense float64 restatement on the expanded design [Q, Z]
(within 1e-14 of its longdouble form: tests/test_group_host.py).

Panel: 331 animals x 600 SNPs with its splits (n_T, n_V), and the deeper 700 x 800 panel (n_T = 520, k = 513).
Designs (tests/group_ref.py): 18 levels (17 columns under snp: the first wide case, one column in the second
slab), 40 levels + 3 covariates (three slabs, the last partial), 113 levels + 15 covariates at (257, 70) (127
columns under snp, 128 under gblup: the limit).  Labels are uniform over the levels, the first L train animals
hold levels 0 .. L-1; covariates are covar_ref.make_cov's.

  A  against the restatement: group_effects, group_center, cov_effects, cov_center, ebv, fitness, intercept,
     center, effects -- auto branch (a ragged batch: kernel form, gblup and snp models mixed; a genome alone: SNP
     form), forced gblup, forced snp at k > n_T; the deeper panel in both forms.  cond(G) <= 1e6 in every case.
  B  against existing entries: 5 levels + 3 covariates is fit(covariates=expanded) bit for bit under both
     branches; one level is fit() under snp and a column of ones under gblup; an engine whose phenotype is the returned y* gives evaluate()'s ebv / fitness and fit()'s effects
  C  TBLUP_FORM=1 against 2 within tolerance; TBLUP_WORKSPACE_MB=1, TBLUP_SCORE_LDS=0, the same call twice, a
     model alone against inside a batch of the same form: the same bits
  D  1 to 4 traits: group_center identical, each trait within tolerance of its single-trait run
  E  permuted level codes (another reference level under snp): y*, ebv, fitness, SNP effects within tolerance
  F  a covariate equal to a level's indicator, a column of ones beside gblup groups, a monomorphic panel: NaN,
     no error; an unseen validation label and 129 columns: ValueError; a code >= n_levels, -1 on a train row, a
     level without a train row, n_cov = 17: TBLUP_ERR_ARG; an empty batch; a context without a panel
  G  BlupParallelEvaluator.fit_models(groups=); PanelModel.predict(.., groups=) / adjust on the host

Tolerance: covar_ref.TOL, |got - ref| <= 1e-9 max(1, max |ref|) per array.  Each group prints the largest error
it saw (pytest -s); the printed figures are no thresholds.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import group_ref as G
from tests import model_ref as R
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = G.H2
TOL = G.TOL
N, P = R.N_ANIMALS, R.N_SNPS
GFIELDS = ("group_effects", "group_center")
MFIELDS = ("effects", "center", "intercept")


class _Worst:
    def __init__(self, label):
        self.label, self.v, self.cond = label, 0.0, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = C.close(got, ref)
        self.v = max(self.v, err)
        assert err <= TOL, (name, err)

    def check(self, model, ebv, ref, name):
        """one PanelModel and its validation EBVs against a group_ref dictionary."""
        self.cond = max(self.cond, ref["cond"])
        assert ref["cond"] <= G.COND_MAX, (name, ref["cond"])
        fields = GFIELDS + MFIELDS + (("cov_effects", "cov_center") if ref["cov_effects"].shape[1] else ())
        for f in fields:
            self.close(getattr(model, f), ref[f], name + " " + f)
        if not ref["cov_effects"].shape[1]:
            assert model.cov_effects is None and model.cov_center is None
        np.testing.assert_array_equal(model.group_levels, ref["group_levels"])
        self.close(np.atleast_2d(ebv), ref["ebv"], name + " ebv")
        self.close(model.fitness, ref["fitness"], name + " fitness")

    def show(self):
        print("\nGROUP %s: worst error / max(1, max |ref|) %.3e, worst cond(G) %.3e" % (self.label, self.v, self.cond))


def _fields(m):
    return GFIELDS + MFIELDS + (("cov_effects", "cov_center") if m.cov_effects is not None else ())


def _same(ma, ea, mb, eb, msg=""):
    assert (ma.cov_effects is None) == (mb.cov_effects is None)
    for f in _fields(ma) + ("indices", "group_levels"):
        np.testing.assert_array_equal(getattr(ma, f), getattr(mb, f), err_msg=f + " " + msg)
    assert ma.fitness == mb.fitness or (np.isnan(ma.fitness) and np.isnan(mb.fitness)), msg
    np.testing.assert_array_equal(ea, eb, err_msg="ebv " + msg)


def _all_nan(m, ebv):
    return all(np.all(np.isnan(getattr(m, f))) for f in _fields(m)) and np.isnan(m.fitness) and np.all(np.isnan(ebv))


@pytest.fixture(scope="module")
def eng(gpu):
    pn = G.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", list(G.DESIGNS))
def test_a_auto_branch(eng, design):
    pn = G.panel()
    genomes = [pn["genomes"][k] for k in G.AUTO_KEYS]
    w = _Worst("A auto " + design)
    for s in G.DESIGN_SPLITS[design]:
        T, V = pn["splits"][s]
        q, g = G.design_inputs(design, s)
        models, ebv = eng.fit(genomes, T, V, H2, covariates=q, groups=g, return_ebv=True)
        assert ebv.shape == (len(genomes), len(V))
        assert {m.branch for m in models} == {"gblup", "snp"}          # mixed modes in one kernel-form batch
        for i, k in enumerate(G.AUTO_KEYS):
            ref = G.case_ref(design, s, k, "auto")
            assert models[i].branch == ref["branch"] and models[i].n_levels == G.DESIGNS[design][0]
            w.check(models[i], ebv[i], ref, "%s %s %s (batch)" % (design, s, k))
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                m1, e1 = eng.fit([genomes[i]], T, V, H2, covariates=q, groups=g, return_ebv=True)
                w.check(m1[0], e1[0], ref, "%s %s %s (alone)" % (design, s, k))
    w.show()


@pytest.mark.parametrize("design", list(G.DESIGNS))
def test_a_forced_branches(eng, design):
    pn = G.panel()
    w = _Worst("A forced " + design)
    for s in G.DESIGN_SPLITS[design]:
        T, V = pn["splits"][s]
        q, g = G.design_inputs(design, s)
        for branch, keys in (("gblup", G.GBLUP_KEYS), ("snp", G.snp_keys(s[0]))):
            models, ebv = eng.fit([pn["genomes"][k] for k in keys], T, V, H2, branch=branch, covariates=q, groups=g,
                                  return_ebv=True)
            for i, k in enumerate(keys):
                if branch == "gblup":
                    assert np.all(models[i].group_center == 0.0)
                else:
                    assert np.all(models[i].group_effects[:, 0] == 0.0)
                w.check(models[i], ebv[i], G.case_ref(design, s, k, branch), "%s %s %s %s" % (design, branch, s, k))
    w.show()


def test_a_deeper_panel(gpu):
    dp = G.deep_panel()
    q, g = G.deep_inputs()
    w = _Worst("A deep")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            m, ebv = e.fit([dp["genome"]], dp["train"], dp["valid"], H2, covariates=q, groups=g, return_ebv=True)
            got[form] = (m[0], ebv[0])
            w.check(m[0], ebv[0], G.deep_ref(), "form " + form)
    w.close(got["1"][0].group_effects, got["2"][0].group_effects, "form 1 vs 2")
    w.show()


# ---------------------------------------------------------------------------------------------
# B. against existing entries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["snp", "gblup"])
def test_b_narrow_design_is_fit_covariates_bit_for_bit(eng, branch):
    """5 levels + 3 covariates: 7 columns under snp, 8 under gblup -- k_covar's own path on the expanded matrix."""
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    q, g = C.make_cov(N, 3), G.make_groups(N, 5, T)
    X, lev = G.expand(q, g, T, branch)
    genomes = [pn["genomes"][k] for k in (64, 127, 200)]
    m, e = eng.fit(genomes, T, V, H2, branch=branch, covariates=q, groups=g, return_ebv=True)
    mx, ex = eng.fit(genomes, T, V, H2, branch=branch, covariates=X, return_ebv=True)
    lo = 1 if branch == "snp" else 0
    for a, b in zip(m, mx):
        assert np.all(np.isfinite(a.group_effects))
        np.testing.assert_array_equal(a.cov_effects, b.cov_effects[:, :3])
        np.testing.assert_array_equal(a.cov_center, b.cov_center[:3])
        np.testing.assert_array_equal(a.group_effects[:, lo:], b.cov_effects[:, 3:])
        np.testing.assert_array_equal(a.group_center[lo:], b.cov_center[3:])
        if lo:
            assert np.all(a.group_effects[:, 0] == 0.0) and a.group_center[0] == np.mean(g[T] == lev[0])
        for f in MFIELDS:
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
        assert a.fitness == b.fitness
    np.testing.assert_array_equal(e, ex)


def test_b_one_level(eng):
    """One level for everybody: no fixed column at all under snp (the reference level alone: fit()'s model), a
    column of ones under gblup (fit(covariates=ones) bit for bit)."""
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    genomes = [pn["genomes"][k] for k in (64, 200)]
    g = np.full(N, 4)
    w = _Worst("B one level")
    ms, es = eng.fit(genomes, T, V, H2, branch="snp", groups=g, return_ebv=True)
    plain = eng.fit(genomes, T, V, H2, branch="snp")
    _, pe = eng.evaluate(genomes, T, V, H2, branch="snp", return_ebv=True)
    for a, b, x, y in zip(ms, plain, es, pe):
        assert a.group_effects.shape == (1, 1) and a.group_effects[0, 0] == 0.0 and a.group_center[0] == 1.0
        for f in MFIELDS:
            w.close(getattr(a, f), getattr(b, f), f)
        w.close(a.fitness, b.fitness, "fitness")
        w.close(x, y, "ebv")
    mg, eg = eng.fit(genomes, T, V, H2, branch="gblup", groups=g, return_ebv=True)
    mo, eo = eng.fit(genomes, T, V, H2, branch="gblup", covariates=np.ones(N), return_ebv=True)
    for a, b in zip(mg, mo):
        np.testing.assert_array_equal(a.group_effects, b.cov_effects)
        np.testing.assert_array_equal(a.effects, b.effects)
        assert a.group_center[0] == 0.0 and a.fitness == b.fitness
    np.testing.assert_array_equal(eg, eo)
    w.show()


def test_b_engine_on_adjusted_phenotype(gpu):
    """groups= only, the wide path: an engine whose phenotype is the returned y* reproduces the genomic model."""
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    g = G.make_groups(N, 40, T)
    keys = (64, 200, 400)
    genomes = [pn["genomes"][k] for k in keys]
    w = _Worst("B y*")
    with _engine(pn["geno"], pn["pheno"]) as e:
        models, ebv = e.fit(genomes, T, V, H2, groups=g, return_ebv=True)
    for i, gen in enumerate(genomes):
        assert models[i].cov_effects is None
        ys = models[i].adjust(pn["pheno"], groups=g)
        rows = np.concatenate([T, V])
        ysf = np.where(np.isnan(ys), 0.0, ys)          # (animals outside the split may hold unseen labels)
        assert np.all(np.isfinite(ys[rows]))
        with _engine(pn["geno"], ysf) as e2:
            f2, e2v = e2.evaluate([gen], T, V, H2, return_ebv=True)
            m2 = e2.fit([gen], T, V, H2)[0]
        w.close(ebv[i], e2v[0], "ebv %s" % (keys[i],))
        w.close(models[i].fitness, f2[0], "fitness %s" % (keys[i],))
        w.close(models[i].effects, m2.effects, "effects %s" % (keys[i],))
        w.close(models[i].intercept, m2.intercept, "intercept %s" % (keys[i],))
    w.show()


# ---------------------------------------------------------------------------------------------
# C. form and bits
# ---------------------------------------------------------------------------------------------
def test_c_forms_agree(gpu):
    pn = G.panel()
    s, design = (257, 70), "L40c3"
    T, V = pn["splits"][s]
    q, g = G.design_inputs(design, s)
    keys = [64, 127, 200]
    genomes = [pn["genomes"][k] for k in keys]
    w = _Worst("C forms")
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.fit(genomes, T, V, H2, covariates=q, groups=g, return_ebv=True)
    for i, k in enumerate(keys):
        ref = G.case_ref(design, s, k, "auto")
        for form, (m, ebv) in got.items():
            w.check(m[i], ebv[i], ref, "form %s %s" % (form, k))
        for f in GFIELDS + MFIELDS + ("cov_effects",):
            w.close(getattr(got["1"][0][i], f), getattr(got["2"][0][i], f), "form 1 vs 2 " + f)
        w.close(got["1"][1][i], got["2"][1][i], "form 1 vs 2 ebv")
    w.show()


@pytest.mark.parametrize("form", ["1", "2"])
def test_c_same_bits(gpu, form):
    """Chunked by a 1 MB workspace, right-hand sides in the workspace instead of LDS, the same call twice, a
    model alone against the batch (one form for all: TBLUP_FORM): bit-identical."""
    pn = G.panel()
    s, design = (257, 70), "L40c3"
    T, V = pn["splits"][s]
    q, g = G.design_inputs(design, s)
    genomes = [pn["genomes"][k] for k in (1, 64, 127, "dup", 200)]
    kw = dict(branch="snp", covariates=q, groups=g, return_ebv=True)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
        m0, e0 = e.fit(genomes, T, V, H2, **kw)
        m1, e1 = e.fit(genomes, T, V, H2, **kw)
        alone = [e.fit([x], T, V, H2, **kw) for x in genomes[-3:]]
    assert all(np.all(np.isfinite(m.group_effects)) for m in m0)
    for i in range(len(genomes)):
        _same(m0[i], e0[i], m1[i], e1[i], "twice")
    for j, (ma, ea) in enumerate(alone):
        i = len(genomes) - 3 + j
        _same(m0[i], e0[i], ma[0], ea[0], "alone")
    for env in ({"TBLUP_WORKSPACE_MB": "1"}, {"TBLUP_SCORE_LDS": "0"}, {"TBLUP_SCORE_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], dict(env, TBLUP_FORM=form)) as e:
            m2, e2 = e.fit(genomes, T, V, H2, **kw)
        for i in range(len(genomes)):
            _same(m0[i], e0[i], m2[i], e2[i], str(env))


def test_c_mixed_batch_keeps_each_model_s_bits(gpu):
    """A snp model of 42 columns inside a kernel-form batch with gblup models of 43 (a wider call stride, another
    slab count beside it) against the same model among snp models only: the same bits."""
    pn = G.panel()
    s, design = (257, 70), "L40c3"
    T, V = pn["splits"][s]
    q, g = G.design_inputs(design, s)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": "1"}) as e:
        ma, ea = e.fit([pn["genomes"][k] for k in (64, 400, 200)], T, V, H2, covariates=q, groups=g, return_ebv=True)
        mb, eb = e.fit([pn["genomes"][k] for k in (200, 64)], T, V, H2, covariates=q, groups=g, return_ebv=True)
    assert [m.branch for m in ma] == ["snp", "gblup", "snp"]
    _same(ma[0], ea[0], mb[1], eb[1], "64")
    _same(ma[2], ea[2], mb[0], eb[0], "200")


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits(gpu):
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    g = G.make_groups(N, 18, T)
    w = _Worst("D traits")
    for genomes in ([pn["genomes"][k] for k in (64, 127)], [pn["genomes"][k] for k in (64, 200)]):   # SNP / kernel form
        single = []
        for t in range(4):
            with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, t])) as e:
                single.append(e.fit(genomes, T, V, H2, groups=g, return_ebv=True))
        for nt in (1, 2, 3, 4):
            with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
                models, ebv = e.fit(genomes, T, V, H2, groups=g, return_ebv=True)
            for b, m in enumerate(models):
                np.testing.assert_array_equal(m.group_center, single[0][0][b].group_center)
                assert m.group_effects.shape == (nt, 18)
                fits = []
                for t in range(nt):
                    ms, es = single[t][0][b], single[t][1][b]
                    w.close(m.group_effects[t], ms.group_effects[0], "b trait %d of %d" % (t, nt))
                    w.close(ebv[b] if nt == 1 else ebv[b, t], es, "ebv trait %d of %d" % (t, nt))
                    w.close(m.effects[t], ms.effects[0], "effects trait %d of %d" % (t, nt))
                    fits.append(ms.fitness)
                w.close(m.fitness, np.mean(fits), "fitness of %d traits" % nt)
    w.show()


# ---------------------------------------------------------------------------------------------
# E. reparametrisation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["snp", "gblup"])
def test_e_another_reference_level(eng, branch):
    pn = G.panel()
    s, design = (257, 70), "L40c3"
    T, V = pn["splits"][s]
    q, g = G.design_inputs(design, s)
    L = G.DESIGNS[design][0]
    perm = (7 * np.arange(L) + 5) % L              # a permutation (7 and 40 are coprime) that moves level 0
    keys = [64, 400] if branch == "snp" else [64, 200]
    genomes = [pn["genomes"][k] for k in keys]
    w = _Worst("E " + branch)
    ma, ea = eng.fit(genomes, T, V, H2, branch=branch, covariates=q, groups=g, return_ebv=True)
    mb, eb = eng.fit(genomes, T, V, H2, branch=branch, covariates=q, groups=perm[g], return_ebv=True)
    for a, b, xa, xb in zip(ma, mb, ea, eb):
        w.close(b.adjust(pn["pheno"], q, perm[g]), a.adjust(pn["pheno"], q, g), "y*")
        w.close(xb, xa, "ebv")
        w.close(b.fitness, a.fitness, "fitness")
        w.close(b.effects, a.effects, "effects")
        w.close(b.cov_effects, a.cov_effects, "cov_effects")
    w.show()


# ---------------------------------------------------------------------------------------------
# F. degenerate and bad input
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["1", "2"])
def test_f_collinear_designs_give_nan(gpu, form):
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    g = G.make_groups(N, 40, T)
    genomes = [pn["genomes"][64], pn["genomes"][127]]
    q = C.make_cov(N, 3)
    ind = q.copy()
    ind[:, 1] = (g == 7)                            # a covariate equal to a level's indicator
    ones = q.copy()
    ones[:, 2] = 1.0                                # a column of ones beside gblup groups
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
        for branch, bad in (("snp", ind), ("gblup", ind), ("gblup", ones)):
            models, ebv = e.fit(genomes, T, V, H2, branch=branch, covariates=bad, groups=g, return_ebv=True)
            for m, x in zip(models, ebv):
                assert _all_nan(m, x), branch
        # a good call after a bad one is clean
        models, ebv = e.fit(genomes, T, V, H2, branch="snp", covariates=q, groups=g, return_ebv=True)
        assert all(np.all(np.isfinite(m.group_effects)) and np.all(np.isfinite(x)) for m, x in zip(models, ebv))


def test_f_monomorphic_panel_gives_nan(gpu):
    pn = G.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    g = G.make_groups(N, 18, T)
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        models, ebv = e.fit(genomes, T, V, H2, groups=g, return_ebv=True)
        assert _all_nan(models[0], ebv[0]) and _all_nan(models[1], ebv[1])
        ref = G.group_ref(genomes[2], T, V, geno, pn["pheno"], None, g, H2)
        _Worst("F").check(models[2], ebv[2], ref, "beside monomorphic models")


def test_f_errors(eng):
    from tblup_amd import _native
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    gen = [pn["genomes"][64]]
    g = G.make_groups(N, 18, T)
    unseen = g.copy()
    unseen[V[3]] = 99
    with pytest.raises(ValueError, match="99"):
        eng.fit(gen, T, V, H2, groups=unseen)
    named = np.array(["h%02d" % x for x in g], dtype="U12")
    named[V[3]] = "elsewhere"
    with pytest.raises(ValueError, match="elsewhere"):
        eng.fit(gen, T, V, H2, groups=named)
    outside = g.copy()
    outside[np.setdiff1d(np.arange(N), np.concatenate([T, V]))[:5]] = 99        # unseen outside the split: fine
    a, b = eng.fit(gen, T, V, H2, groups=outside)[0], eng.fit(gen, T, V, H2, groups=g)[0]
    np.testing.assert_array_equal(a.group_effects, b.group_effects)
    for wrong in (g[:-1], g.astype(np.float64), np.stack([g, g], axis=1)):
        with pytest.raises(ValueError):
            eng.fit(gen, T, V, H2, groups=wrong)
    with pytest.raises(ValueError):
        eng.fit(gen, T, V, H2, groups=g, reliability_of=[1, 2])
    # 129 columns: 113 levels + 16 covariates under gblup (128 under snp is fitted)
    T2, V2 = pn["splits"][257, 70]
    g113, q16 = G.make_groups(N, 113, T2), C.make_cov(N, 16)
    with pytest.raises(ValueError, match="129"):
        eng.fit(gen, T2, V2, H2, branch="gblup", covariates=q16, groups=g113)
    assert np.all(np.isfinite(eng.fit(gen, T2, V2, H2, branch="snp", covariates=q16, groups=g113)[0].group_effects))
    # the entries that do not take the class factor say so
    for call in (lambda: eng.evaluate(gen, T, V, H2, groups=g), lambda: eng.snp_scores(gen, T, V, H2, [1], groups=g),
                 lambda: eng.log_likelihood_cov(gen, T, V, H2, C.make_cov(N, 2), groups=g),
                 lambda: eng.estimate_h2_cov(gen, T, V, C.make_cov(N, 2), groups=g),
                 lambda: eng.reliability_cov(gen, T, V, H2, [1], C.make_cov(N, 2), groups=g)):
        with pytest.raises(ValueError, match="groups"):
            call()
    models, ebv = eng.fit([], T, V, H2, groups=g, return_ebv=True)
    assert models == [] and ebv.shape == (0, len(V))
    # the C entry itself
    lib = _native.load()
    i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    sid = eng.split_id(T, V)
    idx = np.ascontiguousarray(gen[0], dtype=np.int64)
    off = np.array([0, len(idx)], dtype=np.int64)
    q = C.make_cov(N, 5)
    wide = np.zeros((N, 17))
    ce, cc, ge, gc, fit = (np.full(n, 7.0) for n in (17, 17, 18, 18, 1))

    def call(codes, L=18, cov=q, nc=5, batch=1):
        codes = np.ascontiguousarray(codes, dtype=np.int64)
        return lib.tblup_fit_group_batch(eng._ctx, sid, cov.ctypes.data_as(f64), nc, codes.ctypes.data_as(i64), L,
                                         idx.ctypes.data_as(i64), off.ctypes.data_as(i64), batch, H2, 0,
                                         fit.ctypes.data_as(f64), None, ce.ctypes.data_as(f64), cc.ctypes.data_as(f64),
                                         ge.ctypes.data_as(f64), gc.ctypes.data_as(f64), None, None, None)
    high, low, hole, gap = g.copy(), g.copy(), g.copy(), g.copy()
    high[5] = 18                      # a code >= n_levels
    low[5] = -2
    hole[T[40]] = -1                  # -1 on a train row
    gap[g == 17] = 16                 # level 17 has no train row
    bad = q.copy()
    bad[17, 2] = np.nan
    for rc in (call(high), call(low), call(hole), call(gap), call(g, cov=wide, nc=17), call(g, nc=-1), call(g, L=0),
               call(g, cov=bad)):
        assert rc == _native.ERR_ARG
    novalid = g.copy()
    novalid[V[0]] = -1                # -1 on a validation row
    assert call(novalid) == _native.ERR_ARG
    assert call(g, batch=0) == 0
    assert all(np.all(a == 7.0) for a in (ce, cc, ge, gc, fit))
    assert call(g) == 0 and np.all(ce[:5] != 7.0) and np.all(ce[5:] == 7.0) and np.all(ge != 7.0)
    assert ge[0] == 0.0 and abs(gc.sum() - 1.0) < 1e-12


def test_f_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        o1, o2 = np.zeros(1), np.zeros(1)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_fit_group_batch(ctx, 0, None, 0, one.ctypes.data_as(i64), 1, one.ctypes.data_as(i64),
                                       off.ctypes.data_as(i64), 1, 0.4, 0, None, None, None, None, o1.ctypes.data_as(f64),
                                       o2.ctypes.data_as(f64), None, None, None)
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# G. drop-in and host
# ---------------------------------------------------------------------------------------------
def test_g_evaluator_fit_models(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = G.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    q = C.make_cov(N, 3)
    w = _Worst("G")
    with E.BlupParallelEvaluator(gp, pp, H2) as ev:
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        test = np.asarray(ev.testing_indices)
        g = G.make_groups(N, 40, train)
        g[test] = g[train][np.arange(len(test)) % len(train)]          # every testing animal holds a fitted level
        named = np.array(["herd%02d" % x for x in g])
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 129, 200)]
        models = ev.fit_models(pop, covariates=q, groups=named)
        gs = [np.sort(i.genome) for i in pop]          # (no removed SNPs: the final genome is the sorted set)
        direct, ebv = ev.engine.fit(gs, train, test, H2, covariates=q, groups=named, return_ebv=True)
        for call in (lambda: ev.snp_scores(pop, [1], groups=named), lambda: ev.log_likelihood(pop, H2, groups=named),
                     lambda: ev.estimate_h2(pop, groups=named)):
            with pytest.raises(ValueError, match="groups"):
                call()
        for b, (m, d) in enumerate(zip(models, direct)):
            _same(m, ebv[b], d, ebv[b], "fit_models vs engine.fit")
            ref = G.group_ref(gs[b], train, test, pn["geno"], pn["pheno"], q, named, H2)
            w.check(m, ebv[b], ref, "model %d" % b)
            fixed = (q[test] - m.cov_center) @ m.cov_effects[0] + \
                ((named[test][:, None] == m.group_levels[None, :]) - m.group_center) @ m.group_effects[0]
            w.close(m.predict(pn["geno"][test], covariates=q[test], groups=named[test]), ebv[b] + fixed, "predict %d" % b)
            w.close(m.predict(pn["geno"][test]), ebv[b], "predict genomic %d" % b)
            rows = np.concatenate([train, test])
            w.close(m.adjust(pn["pheno"][rows], q[rows], named[rows]), ref["ystar"][rows, 0], "adjust %d" % b)
    w.show()
