"""Restricted likelihood of h2 with fixed-effect covariates (tblup_loglik_cov_batch: k_covar in keep mode and
k_loglik's corrections behind every pass; GpuBlupEngine.log_likelihood_cov / estimate_h2_cov) on the GPU, against the dense float64
restatement of tests/score_cov_ref.py (itself within 1e-11 of a longdouble computation and equal to the
explicit-contrast likelihood: tests/test_score_cov_host.py).

Panels and covariates: tests/covar_ref.py's cases (331 x 600 with its four splits, c = 1, 5, 16; the deeper
700 x 800 panel) and the 1200 x 1100 panel of tests/score_cov_ref.py; h2 in {0.05, 0.4, 0.9}.

  A  against the restatement: auto branch (ragged batch: kernel form; alone: SNP form where k <= n_T), forced
     gblup with the column of ones, forced snp at n_T < k, the deeper panel in both forms, a (G, B) matrix of h2
  B  the 1200 x 1100 panel: systems of 1024 rows in both forms and of 1152 rows, c = 16
  C  the same bits: TBLUP_SCORE_LDS=0 with and without TBLUP_WORKSPACE_MB=1, the same call twice, a model alone
     against inside a batch; cov_effects and fitness at every h2 those of fit(covariates=) and evaluate()
  D  four traits against the restatement
  E  estimate_h2_cov against the same search on the restatement, on phenotypes with a strong covariate
     effect (the estimate without Q lies elsewhere: tests/test_score_cov_host.py)
  F  collinear covariates, a column constant over the train rows under snp (its plane has no log|Q~'Q~|), a
     monomorphic panel, c >= N - r: NaN; n_cov 0 / 17, NaN in cov, h2 = 1, a context without a panel
  G  BlupParallelEvaluator.log_likelihood / estimate_h2 (covariates=)

Tolerance: |got - ref| <= 1e-9 max(1, |ref|), tests/loglik_ref.py::TOL.  Each group prints the largest error it
saw (pytest -s); no printed figure is a threshold.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import loglik_ref as LL
from tests import model_ref as R
from tests import score_cov_ref as A
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

TOL = A.LL_TOL
N, P = R.N_ANIMALS, R.N_SNPS
HS = np.array(A.H2S)
I64, F64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = LL.close(got, ref)
        self.v = max(self.v, err)
        print("  %-44s %.3e" % (name, err))
        assert err <= TOL, (name, err)

    def show(self):
        print("\nLOGLIK-COV %s: worst error / max(1, |ref|) %.3e" % (self.label, self.v))


def _cov(c, ones=False):
    return C.make_cov(N, c, ones=ones)


def _ref(name):
    """(loglik (G,), sigma2_g (G,)) of a case over HS."""
    out = [A.case_loglik(name, float(h)) for h in HS]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


@pytest.fixture(scope="module")
def eng(gpu):
    pn = A.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    pn = A.panel()
    genomes = [pn["genomes"][k] for k in C.AUTO_KEYS]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.SPLIT_COV[s])
        ll, s2 = eng.log_likelihood_cov(genomes, T, V, HS, return_sigma2=True, covariates=q)
        assert ll.shape == s2.shape == (len(HS), len(genomes))
        for i, k in enumerate(C.AUTO_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            rl, rs = _ref(name)
            w.close(ll[:, i], rl, name + " l (batch)")
            w.close(s2[:, i], rs, name + " s2 (batch)")
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                l1, s1 = eng.log_likelihood_cov([genomes[i]], T, V, HS, return_sigma2=True, covariates=q)
                w.close(l1[:, 0], rl, name + " l (alone)")
                w.close(s1[:, 0], rs, name + " s2 (alone)")
    w.show()


def test_a_forced_branches(eng):
    pn = A.panel()
    w = _Worst("A forced")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.GBLUP_COV[s], ones=True)
        ll, s2 = eng.log_likelihood_cov([pn["genomes"][k] for k in R.GBLUP_KS], T, V, HS, branch="gblup",
                                    return_sigma2=True, covariates=q)
        for i, k in enumerate(R.GBLUP_KS):
            rl, rs = _ref("gblup-%d-%d-%s" % (s + (k,)))
            w.close(ll[:, i], rl, "gblup %s %s l" % (s, k))
            w.close(s2[:, i], rs, "gblup %s %s s2" % (s, k))
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in (200, 332, 400) if k > s[0]]
        ll, s2 = eng.log_likelihood_cov([pn["genomes"][k] for k in ks], T, V, HS, branch="snp", return_sigma2=True,
                                    covariates=_cov(C.SPLIT_COV[s]))
        for i, k in enumerate(ks):
            rl, rs = _ref("snp-%d-%d-%s" % (s + (k,)))
            w.close(ll[:, i], rl, "snp %s %s l" % (s, k))
            w.close(s2[:, i], rs, "snp %s %s s2" % (s, k))
    w.show()


def test_a_deeper_panel(gpu):
    dp = A.deep_panel()
    q = C.make_cov(len(dp["pheno"]), C.DEEP_COV)
    rl, rs = _ref("deep")
    w = _Worst("A deep")
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            ll, s2 = e.log_likelihood_cov([dp["genome"]], dp["train"], dp["valid"], HS, return_sigma2=True, covariates=q)
            w.close(ll[:, 0], rl, "form %s l" % form)
            w.close(s2[:, 0], rs, "form %s s2" % form)
    w.show()


def test_a_matrix_of_h2(eng):
    """Every model its own h2 in every row: row g, model b is the scalar call's value, bit for bit."""
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(16)
    genomes = [pn["genomes"][k] for k in (63, 64, 127)]
    H = np.array([[0.05, 0.4, 0.9], [0.9, 0.05, 0.4]])
    ll = eng.log_likelihood_cov(genomes, T, V, H, covariates=q)
    for g in range(2):
        for b in range(3):
            one = eng.log_likelihood_cov([genomes[b]], T, V, float(H[g, b]), covariates=q)
            assert one[0] == ll[g, b]


# ---------------------------------------------------------------------------------------------
# B. LDS at its limit and the workspace path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in A.big_cases()])
def test_b_systems_of_1024_rows_and_above(gpu, name):
    bp = A.big_panel()
    _, g, t, v, qk, br, rows, lds = next(x for x in A.big_cases() if x[0] == name)
    ref = A.big_ref(name)
    w = _Worst("B " + name)
    got = {}
    for knob in ("1", "0"):
        with _engine(bp["geno"], bp["pheno"], {"TBLUP_SCORE_LDS": knob}) as e:
            got[knob] = e.log_likelihood_cov([bp[g]], bp[t], bp[v], A.H2, branch=br, return_sigma2=True, covariates=bp[qk])
    w.close(got["1"][0], ref["loglik"], name + " l")
    w.close(got["1"][1], ref["sigma2_g"], name + " s2")
    np.testing.assert_array_equal(got["0"][0], got["1"][0])
    np.testing.assert_array_equal(got["0"][1], got["1"][1])
    w.show()


# ---------------------------------------------------------------------------------------------
# C. the same bits, and the other outputs of the same pass
# ---------------------------------------------------------------------------------------------
def _raw(e, genomes, T, V, H, q, branch=0):
    """the entry with every output: (fitness (G, B), loglik, sigma2_g (G, B, 1), cov_effects (G, B, 1, c))"""
    from tblup_amd.engine import concat_genomes
    idx, off = concat_genomes(genomes)
    B, G, c = len(genomes), H.shape[0], q.shape[1]
    Hm = np.ascontiguousarray(np.broadcast_to(H.reshape(G, -1), (G, B)))
    fit, ll, s2, be = np.empty((G, B)), np.empty((G, B, 1)), np.empty((G, B, 1)), np.empty((G, B, 1, c))
    rc = e._lib.tblup_loglik_cov_batch(e._ctx, e.split_id(T, V), q.ctypes.data_as(F64), c, idx.ctypes.data_as(I64),
                                       off.ctypes.data_as(I64), B, Hm.ctypes.data_as(F64), G, branch,
                                       fit.ctypes.data_as(F64), ll.ctypes.data_as(F64), s2.ctypes.data_as(F64),
                                       be.ctypes.data_as(F64))
    assert rc == 0, e._lib.tblup_last_error()
    return fit, ll, s2, be


def test_c_same_bits_and_the_other_outputs(eng):
    pn = A.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(5)
    snp = [pn["genomes"][k] for k in (1, 65, 129, 200, "dup")]              # SNP form (every k <= n_T)
    mixed = snp + [pn["genomes"][400]]                                      # kernel form
    ref = [_raw(eng, g, T, V, HS, q) for g in (snp, mixed)]
    for i, g in enumerate((snp, mixed)):
        for a, b in zip(_raw(eng, g, T, V, HS, q), ref[i]):
            np.testing.assert_array_equal(a, b, err_msg="twice")
        ll, s2 = eng.log_likelihood_cov(g, T, V, HS, return_sigma2=True, covariates=q)
        np.testing.assert_array_equal(ll, ref[i][1][:, :, 0])
        np.testing.assert_array_equal(s2, ref[i][2][:, :, 0])
        # cov_effects and fitness at every h2: fit(covariates=)'s and evaluate()'s
        for gi, h in enumerate(HS):
            models = eng.fit(g, T, V, float(h), covariates=q)
            np.testing.assert_array_equal(ref[i][3][gi], np.stack([m.cov_effects for m in models]))
            np.testing.assert_array_equal(ref[i][0][gi], eng.evaluate(g, T, V, float(h)))
    for env in ({"TBLUP_SCORE_LDS": "0"}, {"TBLUP_SCORE_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}, {"TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for i, g in enumerate((snp, mixed)):
                for a, b in zip(_raw(e, g, T, V, HS, q), ref[i]):
                    np.testing.assert_array_equal(a, b, err_msg=str(env))
    for b in (0, 3):      # a model alone against inside a batch of the same form
        for x, y in zip(_raw(eng, [snp[b]], T, V, HS, q), ref[0]):
            np.testing.assert_array_equal(x[:, 0], y[:, b], err_msg="alone")


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_four_traits(gpu):
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(5)
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    none = np.zeros(0, dtype=np.int64)
    w = _Worst("D traits")
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :4])) as e:
        for i, b in enumerate(batches):
            ll, s2 = e.log_likelihood_cov(b, T, V, A.H2, return_sigma2=True, covariates=q)
            assert ll.shape == s2.shape == (len(b), 4)
            for m, g in enumerate(b):
                ref = A.adj_ref(g, T, pn["geno"], pn["Y"][:, :4], q, A.H2, snps=none)
                w.close(ll[m], ref["loglik"], "l %d %d" % (i, m))
                w.close(s2[m], ref["sigma2_g"], "s2 %d %d" % (i, m))
    w.show()


# ---------------------------------------------------------------------------------------------
# E. estimate_h2
# ---------------------------------------------------------------------------------------------
def test_e_estimate_h2_with_covariates(gpu):
    x = A.est_inputs()
    ref = A.estimate_ref(x["genome"], x["T"], x["geno"], x["pheno"], x["cov"])
    plain = A.estimate_ref(x["genome"], x["T"], x["geno"], x["pheno"], None)
    assert abs(ref["h2"] - plain["h2"]) > 10 * max(ref["step"], plain["step"])      # the case is what it claims to be
    with _engine(x["geno"], x["pheno"]) as e:
        est = e.estimate_h2_cov([x["genome"], x["genome"][:120]], x["T"], x["V"], covariates=x["cov"])
        assert set(est) == {"h2", "loglik", "sigma2_g", "sigma2_e", "at_bound", "step"} and est["h2"].shape == (2,)
        refs = [ref, A.estimate_ref(x["genome"][:120], x["T"], x["geno"], x["pheno"], x["cov"])]
        for b, r in enumerate(refs):
            step = max(est["step"][b], r["step"])
            assert 0.0 < est["step"][b] < 1.0
            assert abs(est["h2"][b] - r["h2"]) <= step * (1 + 1e-9), (b, est["h2"][b], r["h2"], step)
            assert est["loglik"][b] >= r["loglik"] - TOL * max(1.0, abs(r["loglik"])), (b, est["loglik"][b], r["loglik"])
            assert bool(est["at_bound"][b]) == r["at_bound"]
            again = e.log_likelihood_cov([[x["genome"], x["genome"][:120]][b]], x["T"], x["V"], float(est["h2"][b]),
                                     covariates=x["cov"])
            assert LL.close(again[0], est["loglik"][b]) <= TOL
        without = e.estimate_h2([x["genome"]], x["T"], x["V"])
        assert abs(without["h2"][0] - est["h2"][0]) > 10 * est["step"][0]
    print("\nestimate_h2 with covariates:", np.round(est["h2"], 4), "without:", np.round(without["h2"], 4))


# ---------------------------------------------------------------------------------------------
# F. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_f_degenerate_inputs_give_nan(gpu):
    pn = A.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    q = _cov(3)
    with _engine(geno, pn["pheno"]) as e:
        two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 2]], axis=1))
        for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][200]]):     # SNP form, kernel form
            ll, s2 = e.log_likelihood_cov(genomes, T, V, HS, return_sigma2=True, covariates=two)
            assert np.all(np.isnan(ll)) and np.all(np.isnan(s2))
        # a column constant over the train rows: the snp plane has no log|Q~'Q~|, the gblup plane has
        const = q.copy()
        const[T, 1] = 1.0
        ll = e.log_likelihood_cov([pn["genomes"][200], pn["genomes"][400]], T, V, A.H2, covariates=const)
        assert np.isnan(ll[0])
        ref = A.adj_ref(pn["genomes"][400], T, geno, pn["pheno"], const, A.H2, snps=np.zeros(0, dtype=np.int64))
        _Worst("F beside a NaN model").close(ll[1], ref["loglik"][0], "gblup model")
        # a monomorphic model panel
        ll = e.log_likelihood_cov([np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]], T, V, A.H2, covariates=q)
        assert np.all(np.isnan(ll[:2])) and np.isfinite(ll[2])
        # c >= N - r: 17 train animals, the intercept and 16 covariates
        ll, s2 = e.log_likelihood_cov([pn["genomes"][64][:5]], T[:17], V, A.H2, branch="snp", return_sigma2=True,
                                  covariates=_cov(16))
        assert np.all(np.isnan(ll)) and np.all(np.isnan(s2))
        est = e.estimate_h2_cov([pn["genomes"][64]], T, V, refine=1, covariates=two)
        assert np.isnan(est["h2"][0]) and not est["at_bound"][0]


def test_f_errors(eng):
    from tblup_amd import _native
    from tblup_amd._native import TblupError, TblupIndexError
    from tblup_amd.engine import concat_genomes
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    q = _cov(5)
    for h in (1.0, 0.0, [0.3, 1.0]):
        with pytest.raises(TblupError):
            eng.log_likelihood_cov(g, T, V, h, covariates=q)
    with pytest.raises(TblupIndexError):
        eng.log_likelihood_cov(g + [np.array([3, P, 5])], T, V, 0.4, covariates=q)
    for bad in (np.zeros((N, 0)), np.zeros((N, 17)), np.full((N, 2), np.nan)):
        with pytest.raises(ValueError):
            eng.log_likelihood_cov(g, T, V, 0.4, covariates=bad)
    assert eng.log_likelihood_cov([], T, V, HS, covariates=q).shape == (len(HS), 0)
    idx, off = concat_genomes(g)
    h, ll = np.array([0.4]), np.empty(1)
    sid = eng.split_id(T, V)

    def call(ctx, cov, nc):
        return eng._lib.tblup_loglik_cov_batch(ctx, sid, None if cov is None else cov.ctypes.data_as(F64), nc,
                                               idx.ctypes.data_as(I64), off.ctypes.data_as(I64), 1, h.ctypes.data_as(F64),
                                               1, 0, None, ll.ctypes.data_as(F64), None, None)
    wide = np.zeros((N, 17))
    assert call(eng._ctx, wide, 0) != 0 and b"n_cov" in eng._lib.tblup_last_error()
    assert call(eng._ctx, wide, 17) != 0 and b"n_cov" in eng._lib.tblup_last_error()
    assert call(eng._ctx, None, 2) != 0
    nanq = q.copy()
    nanq[7, 3] = np.inf
    assert call(eng._ctx, nanq, 5) != 0 and b"finite" in eng._lib.tblup_last_error()
    assert call(eng._ctx, q, 5) == 0 and np.isfinite(ll[0])
    ctx = ctypes.c_void_p()
    assert eng._lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        assert call(ctx, q, 5) == _native.ERR_STATE and b"panel" in eng._lib.tblup_last_error()
    finally:
        eng._lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# G. evaluator level
# ---------------------------------------------------------------------------------------------
def test_g_evaluator(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = A.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(11)
    q = _cov(5)
    none = np.zeros(0, dtype=np.int64)
    w = _Worst("G")
    with E.BlupParallelEvaluator(gp, pp, A.H2) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 129)]
        genomes = [i.genome for i in pop]
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        ll = ev.log_likelihood(pop, 0.4, covariates=q)
        np.testing.assert_array_equal(ll, ev.engine.log_likelihood_cov(genomes, train, ev.testing_indices, 0.4, covariates=q))
        for b, g in enumerate(genomes):
            w.close(ll[b], A.adj_ref(g, train, pn["geno"], pn["pheno"], q, 0.4, snps=none)["loglik"][0], "model %d" % b)
        est = ev.estimate_h2(pop, refine=1, points=5, covariates=q)
        direct = ev.engine.estimate_h2_cov(genomes, train, ev.testing_indices, refine=1, points=5, covariates=q)
        for k in est:
            np.testing.assert_array_equal(est[k], direct[k])
    w.show()
