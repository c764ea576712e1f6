"""Fixed-effect covariates in the fitted model (tblup_fit_cov_batch, k_covar, k_cov_fitness) on the GPU, against
the dense float64 restatement of tests/covar_ref.py (itself within 1e-11 of a longdouble computation and
checked against Henderson's mixed-model equations: tests/test_covar_host.py).

Panel: 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64), (257, 70), the genomes of
tests/reliability_ref.py; a deeper panel (700 x 800, n_T = 520, k = 513: 5 tile columns in either form).
Covariate counts 1, 5 and 16 go round with the split (tests/covar_ref.py).

  A  against the restatement: cov_effects, cov_center, ebv, fitness, intercept, center, effects -- auto
     branch (ragged batch: kernel form; one genome alone: SNP form where k <= n_T), forced gblup with a column
     of ones, forced snp at n_T < k <= n and k > n, the deeper panel in both forms
  B  against existing entries: an engine whose phenotype is the returned y* gives evaluate()'s ebv / fitness
     and fit()'s effects within tolerance; with one covariate = SNP column j under snp, b = score / info of
     snp_scores for j, in both forms
  C  TBLUP_FORM=1 against 2 and TBLUP_PAD_FIRST=0 within tolerance; TBLUP_WORKSPACE_MB=1, TBLUP_SCORE_LDS=0,
     the same call twice, a model alone against inside a batch of the same form: the same bits
  D  1 to 4 traits: cov_center identical, each trait's b and ebv within tolerance of the single-trait run
  E  covariates that do nothing (the phenotype is already adjusted for them: b numerically zero): fitness and
     effects within tolerance of fit()'s
  F  collinear columns, a column constant over the train rows under snp, a monomorphic panel: NaN, no error;
     NaN in Q, 0 or 17 columns, a wrong row count: ValueError / TBLUP_ERR_ARG; out-of-range indices:
     IndexError; an empty batch; a context without a panel
  G  BlupParallelEvaluator.fit_models(covariates=) and PanelModel.predict(.., covariates=) on the host

Tolerance: |got - ref| <= 1e-9 max(1, max |ref|) per array, tests/score_ref.py::TOL.  Each group prints the
largest error it saw (pytest -s); the printed figures are no thresholds.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = C.H2
TOL = C.TOL
N, P = R.N_ANIMALS, R.N_SNPS
FIELDS = ("cov_effects", "cov_center", "effects", "center", "intercept")


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = C.close(got, ref)
        self.v = max(self.v, err)
        assert err <= TOL, (name, err)

    def check(self, model, ebv, ref, name):
        """one PanelModel and its validation EBVs against a cov_ref dictionary."""
        for f in FIELDS:
            self.close(getattr(model, f), ref[f], name + " " + f)
        self.close(np.atleast_2d(ebv), ref["ebv"], name + " ebv")
        self.close(model.fitness, ref["fitness"], name + " fitness")

    def show(self):
        print("\nCOVAR %s: worst error / max(1, max |ref|) %.3e" % (self.label, self.v))


def _same(ma, ea, mb, eb, msg=""):
    for f in FIELDS + ("indices",):
        np.testing.assert_array_equal(getattr(ma, f), getattr(mb, f), err_msg=f + " " + msg)
    assert ma.fitness == mb.fitness or (np.isnan(ma.fitness) and np.isnan(mb.fitness)), msg
    np.testing.assert_array_equal(ea, eb, err_msg="ebv " + msg)


def _cov(c, ones=False):
    return C.make_cov(N, c, ones=ones)


@pytest.fixture(scope="module")
def eng(gpu):
    pn = C.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    pn = C.panel()
    genomes = [pn["genomes"][k] for k in C.AUTO_KEYS]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.SPLIT_COV[s])
        models, ebv = eng.fit(genomes, T, V, H2, covariates=q, return_ebv=True)
        assert ebv.shape == (len(genomes), len(V))
        for i, k in enumerate(C.AUTO_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            ref = C.case_ref(name)
            assert models[i].branch == ref["branch"] and models[i].n_covariates == C.SPLIT_COV[s]
            w.check(models[i], ebv[i], ref, name + " (batch)")
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                m1, e1 = eng.fit([genomes[i]], T, V, H2, covariates=q, return_ebv=True)
                w.check(m1[0], e1[0], ref, name + " (alone)")
    w.show()


def test_a_forced_gblup_with_ones(eng):
    pn = C.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.GBLUP_COV[s], ones=True)
        models, ebv = eng.fit([pn["genomes"][k] for k in R.GBLUP_KS], T, V, H2, branch="gblup", covariates=q,
                              return_ebv=True)
        for i, k in enumerate(R.GBLUP_KS):
            assert np.all(models[i].cov_center == 0.0)
            w.check(models[i], ebv[i], C.case_ref("gblup-%d-%d-%s" % (s + (k,))), "gblup %s %s" % (s, k))
    w.show()


def test_a_forced_snp_dual(eng):
    pn = C.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in (200, 332, 400) if k > s[0]]
        models, ebv = eng.fit([pn["genomes"][k] for k in ks], T, V, H2, branch="snp", covariates=_cov(C.SPLIT_COV[s]),
                              return_ebv=True)
        for i, k in enumerate(ks):
            w.check(models[i], ebv[i], C.case_ref("snp-%d-%d-%s" % (s + (k,))), "snp %s %s" % (s, k))
    w.show()


def test_a_deeper_panel(gpu):
    dp = C.deep_panel()
    q = C.make_cov(len(dp["pheno"]), C.DEEP_COV)
    w = _Worst("A deep")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            m, ebv = e.fit([dp["genome"]], dp["train"], dp["valid"], H2, covariates=q, return_ebv=True)
            got[form] = (m[0], ebv[0])
            w.check(m[0], ebv[0], C.case_ref("deep"), "form " + form)
    w.close(got["1"][0].cov_effects, got["2"][0].cov_effects, "form 1 vs 2")
    w.show()


# ---------------------------------------------------------------------------------------------
# B. against existing entries
# ---------------------------------------------------------------------------------------------
def test_b_engine_on_adjusted_phenotype(gpu):
    pn = C.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(5)
    keys = (64, 200, "neg")
    genomes = [pn["genomes"][k] for k in keys]
    w = _Worst("B y*")
    with _engine(pn["geno"], pn["pheno"]) as e:
        models, ebv = e.fit(genomes, T, V, H2, covariates=q, return_ebv=True)
    for i, g in enumerate(genomes):
        ys = models[i].adjust(pn["pheno"], q)
        with _engine(pn["geno"], ys) as e2:
            f2, e2v = e2.evaluate([g], T, V, H2, return_ebv=True)
            m2 = e2.fit([g], T, V, H2)[0]
        w.close(ebv[i], e2v[0], "ebv %s" % (keys[i],))
        w.close(models[i].fitness, f2[0], "fitness %s" % (keys[i],))
        w.close(models[i].effects, m2.effects, "effects %s" % (keys[i],))
        w.close(models[i].intercept, m2.intercept, "intercept %s" % (keys[i],))
    w.show()


@pytest.mark.parametrize("form", ["1", "2"])
def test_b_one_snp_as_covariate_is_the_score_effect(gpu, form):
    """c = 1 with Q = SNP column j: b = u / v of snp_scores for j (the SNP fitted as a covariate beside the
    panel), under snp in either form."""
    pn = C.panel()
    T, V = pn["splits"][257, 70]
    genomes = [pn["genomes"][k] for k in (64, 129, 200)]
    w = _Worst("B score/info form " + form)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
        for j in (3, 411):
            sc = e.snp_scores(genomes, T, V, H2, [j], branch="snp")
            models = e.fit(genomes, T, V, H2, branch="snp", covariates=pn["geno"][:, j].astype(np.float64))
            for b, m in enumerate(models):
                w.close(m.cov_effects[0, 0], sc.score[b, 0, 0] / sc.info[b, 0], "snp %d model %d" % (j, b))
    w.show()


# ---------------------------------------------------------------------------------------------
# C. other arithmetic within tolerance, the same bits where promised
# ---------------------------------------------------------------------------------------------
def _snp_keys():
    return [1, 64, 65, 127, "dup", "neg"]


def _run(env, genomes, s, c, **kw):
    pn = C.panel()
    T, V = pn["splits"][s]
    with _engine(pn["geno"], pn["pheno"], env) as e:
        return e.fit(genomes, T, V, H2, covariates=_cov(c), return_ebv=True, **kw)


def test_c_forms_and_padding_agree(gpu):
    pn = C.panel()
    keys = _snp_keys()
    genomes = [pn["genomes"][k] for k in keys]
    w = _Worst("C forms / padding")
    for s in ((129, 64), (257, 70)):
        got = {name: _run(env, genomes, s, C.SPLIT_COV[s]) for name, env in
               (("1", {"TBLUP_FORM": "1"}), ("2", {"TBLUP_FORM": "2"}),
                ("pad", {"TBLUP_FORM": "2", "TBLUP_PAD_FIRST": "0"}))}
        for i, k in enumerate(keys):
            ref = C.case_ref("auto-%d-%d-%s" % (s + (k,)))
            for name, (m, ebv) in got.items():
                w.check(m[i], ebv[i], ref, "%s %s %s" % (name, s, k))
            w.close(got["1"][0][i].cov_effects, got["2"][0][i].cov_effects, "form 1 vs 2")
            w.close(got["pad"][1][i], got["2"][1][i], "padding")
    w.show()


@pytest.mark.parametrize("form", ["1", "2"])
def test_c_same_bits(gpu, form):
    """Chunked by a 1 MB workspace, right-hand sides in the workspace instead of LDS, the same call twice,
    a model alone against the batch (one form for all: TBLUP_FORM): bit-identical."""
    pn = C.panel()
    s, c = (257, 70), 5
    T, V = pn["splits"][s]
    genomes = [pn["genomes"][k] for k in _snp_keys() + [200]]
    q = _cov(c)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
        m0, e0 = e.fit(genomes, T, V, H2, branch="snp", covariates=q, return_ebv=True)
        m1, e1 = e.fit(genomes, T, V, H2, branch="snp", covariates=q, return_ebv=True)
        alone = [e.fit([g], T, V, H2, branch="snp", covariates=q, return_ebv=True) for g in genomes[-3:]]
    assert all(np.all(np.isfinite(m.cov_effects)) for m in m0)
    for i in range(len(genomes)):
        _same(m0[i], e0[i], m1[i], e1[i], "twice")
    for j, (ma, ea) in enumerate(alone):
        i = len(genomes) - 3 + j
        _same(m0[i], e0[i], ma[0], ea[0], "alone")
    for env in ({"TBLUP_WORKSPACE_MB": "1"}, {"TBLUP_SCORE_LDS": "0"}, {"TBLUP_SCORE_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], dict(env, TBLUP_FORM=form)) as e:
            m2, e2 = e.fit(genomes, T, V, H2, branch="snp", covariates=q, return_ebv=True)
        for i in range(len(genomes)):
            _same(m0[i], e0[i], m2[i], e2[i], str(env))


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits(gpu):
    pn = C.panel()
    s, c = (129, 64), 5
    T, V = pn["splits"][s]
    q = _cov(c)
    w = _Worst("D traits")
    for genomes in ([pn["genomes"][k] for k in (64, 127)], [pn["genomes"][k] for k in (64, 200)]):   # SNP / kernel form
        single = []
        for t in range(4):
            with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, t])) as e:
                single.append(e.fit(genomes, T, V, H2, covariates=q, return_ebv=True))
        for nt in (1, 2, 3, 4):
            with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
                models, ebv = e.fit(genomes, T, V, H2, covariates=q, return_ebv=True)
            for b, m in enumerate(models):
                np.testing.assert_array_equal(m.cov_center, single[0][0][b].cov_center)
                assert m.cov_effects.shape == (nt, c)
                fits = []
                for t in range(nt):
                    ms, es = single[t][0][b], single[t][1][b]
                    w.close(m.cov_effects[t], ms.cov_effects[0], "b trait %d of %d" % (t, nt))
                    w.close(ebv[b] if nt == 1 else ebv[b, t], es, "ebv trait %d of %d" % (t, nt))
                    w.close(m.effects[t], ms.effects[0], "effects trait %d of %d" % (t, nt))
                    fits.append(ms.fitness)
                w.close(m.fitness, np.mean(fits), "fitness of %d traits" % nt)
    w.show()


# ---------------------------------------------------------------------------------------------
# E. covariates that do nothing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["snp", "gblup"])
def test_e_pre_adjusted_phenotype(gpu, branch):
    """The phenotype is already adjusted for Q (y* of a first fit), so the GLS effects of Q on it are zero up
    to rounding, and the covariate call's fitness and effects are fit()'s."""
    pn = C.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(5, ones=(branch == "gblup"))
    genomes = [pn["genomes"][k] for k in (64, 200)]
    w = _Worst("E " + branch)
    with _engine(pn["geno"], pn["pheno"]) as e:
        first = e.fit(genomes, T, V, H2, branch=branch, covariates=q)
    for i, g in enumerate(genomes):
        ys = first[i].adjust(pn["pheno"], q)
        with _engine(pn["geno"], ys) as e2:
            m = e2.fit([g], T, V, H2, branch=branch, covariates=q)[0]
            plain = e2.fit([g], T, V, H2, branch=branch)[0]
        w.close(m.cov_effects, np.zeros_like(m.cov_effects), "b")
        w.close(m.fitness, plain.fitness, "fitness")
        w.close(m.effects, plain.effects, "effects")
        np.testing.assert_array_equal(m.center, plain.center)
    w.show()


# ---------------------------------------------------------------------------------------------
# F. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def _all_nan(m, ebv):
    return (all(np.all(np.isnan(getattr(m, f))) for f in FIELDS) and np.isnan(m.fitness) and np.all(np.isnan(ebv)))


@pytest.mark.parametrize("form", ["1", "2"])
def test_f_collinear_and_constant_columns_give_nan(gpu, form):
    pn = C.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(3)
    genomes = [pn["genomes"][64], pn["genomes"][127]]
    two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 0], q[:, 2]], axis=1))
    const = q.copy()
    const[T, 1] = 3.0
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
        for bad in (two, const):
            models, ebv = e.fit(genomes, T, V, H2, branch="snp", covariates=bad, return_ebv=True)
            for m, x in zip(models, ebv):
                assert _all_nan(m, x)
        # the same column is no trouble under gblup (no centring), and a good call after a bad one is clean
        models, ebv = e.fit(genomes, T, V, H2, branch="gblup", covariates=const, return_ebv=True)
        assert all(np.all(np.isfinite(m.cov_effects)) and np.all(np.isfinite(x)) for m, x in zip(models, ebv))


def test_f_monomorphic_panel_gives_nan(gpu):
    pn = C.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    q = _cov(5)
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        models, ebv = e.fit(genomes, T, V, H2, covariates=q, return_ebv=True)
        assert _all_nan(models[0], ebv[0]) and _all_nan(models[1], ebv[1])
        ref = C.cov_ref(genomes[2], T, V, geno, pn["pheno"], q, H2)
        _Worst("F").check(models[2], ebv[2], ref, "beside monomorphic models")


def test_f_errors(eng):
    from tblup_amd import _native
    pn = C.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    q = _cov(5)
    bad = q.copy()
    bad[17, 2] = np.nan
    for wrong in (bad, np.where(np.isnan(bad), np.inf, bad), np.zeros((N, 0)), np.zeros((N, 17)), q[:-1], np.zeros((2, N, 3))):
        with pytest.raises(ValueError):
            eng.fit(g, T, V, H2, covariates=wrong)
    with pytest.raises(ValueError):
        eng.fit(g, T, V, H2, covariates=q, reliability_of=[1, 2])
    for out in (P, -P - 1):
        with pytest.raises(_native.TblupIndexError):
            eng.fit(g + [np.array([3, out, 5])], T, V, H2, covariates=q)
    models, ebv = eng.fit([], T, V, H2, covariates=q, return_ebv=True)
    assert models == [] and ebv.shape == (0, len(V))
    # the C entry itself: NaN in cov, n_cov of 0 and 17 are TBLUP_ERR_ARG; an empty batch writes nothing
    lib = _native.load()
    i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    sid = eng.split_id(T, V)
    idx = np.ascontiguousarray(g[0], dtype=np.int64)
    off = np.array([0, len(idx)], dtype=np.int64)
    wide = np.zeros((N, 17))
    be, bc, fit = np.full(17, 7.0), np.full(17, 7.0), np.full(1, 7.0)

    def call(cov, nc, batch=1):
        return lib.tblup_fit_cov_batch(eng._ctx, sid, cov.ctypes.data_as(f64), nc, idx.ctypes.data_as(i64),
                                       off.ctypes.data_as(i64), batch, H2, 0, fit.ctypes.data_as(f64), None,
                                       be.ctypes.data_as(f64), bc.ctypes.data_as(f64), None, None, None)
    assert call(bad, 5) == -1 and call(wide, 0) == -1 and call(wide, 17) == -1
    assert call(q, 5, batch=0) == 0
    assert np.all(be == 7.0) and np.all(bc == 7.0) and np.all(fit == 7.0)
    assert call(q, 5) == 0 and np.all(be[:5] != 7.0) and np.all(be[5:] == 7.0)


def test_f_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        q, o1, o2 = np.zeros(4), np.zeros(1), np.zeros(1)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_fit_cov_batch(ctx, 0, q.ctypes.data_as(f64), 1, one.ctypes.data_as(i64), off.ctypes.data_as(i64),
                                     1, 0.4, 0, None, None, o1.ctypes.data_as(f64), o2.ctypes.data_as(f64), None, None,
                                     None)
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# G. evaluator level
# ---------------------------------------------------------------------------------------------
def test_g_evaluator_fit_models(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = C.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    q = _cov(5)
    w = _Worst("G")
    with E.BlupParallelEvaluator(gp, pp, H2) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        models = ev.fit_models(pop, covariates=q)
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        test = np.asarray(ev.testing_indices)
        gs = [np.sort(i.genome) for i in pop]          # (no removed SNPs: the final genome is the sorted set)
        direct, ebv = ev.engine.fit(gs, train, test, H2, covariates=q, return_ebv=True)
        for b, (m, d) in enumerate(zip(models, direct)):
            _same(m, ebv[b], d, ebv[b], "fit_models vs engine.fit")
            ref = C.cov_ref(gs[b], train, test, pn["geno"], pn["pheno"], q, H2)
            w.check(m, ebv[b], ref, "model %d" % b)
            full = m.predict(pn["geno"][test], covariates=q[test])
            w.close(full, ebv[b] + (q[test] - m.cov_center) @ m.cov_effects[0], "predict with covariates %d" % b)
            w.close(m.predict(pn["geno"][test]), ebv[b], "predict %d" % b)
            w.close(m.adjust(pn["pheno"], q), ref["ystar"][:, 0], "adjust %d" % b)
    w.show()
