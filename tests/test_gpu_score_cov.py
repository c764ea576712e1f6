"""Score statistics of SNPs against fitted panels with fixed-effect covariates (tblup_snp_score_cov_batch:
k_covar in keep mode, k_snpscore's covariate-adjusted instances) on the GPU, against the dense float64
restatement of tests/score_cov_ref.py (itself within 1e-11 of a longdouble computation and checked by two
independent routes: tests/test_score_cov_host.py).

Panels: tests/covar_ref.py's cases -- 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64),
(257, 70), covariate counts 1, 5, 16 going round with the split; the deeper 700 x 800 panel; and a 1200 x 1100
synthetic panel whose systems have exactly 1024 rows (the largest whose right-hand sides live in LDS) and 1152.

  A  against the restatement over all columns: auto branch (ragged batch: kernel form; one genome alone: SNP
     form where k <= n_T), forced gblup with the column of ones, forced snp at n_T < k, the deeper panel and one
     model in both forms
  B  the 1200 x 1100 panel: 1024 rows in both forms (the plan keeps the right-hand sides in LDS: the workspace
     is smaller than with TBLUP_SCORE_LDS=0) and 1152 rows (workspace either way), c = 16, 33 listed SNPs
  C  candidate lists of length 1, 15, 16, 17, 33, 65: every (model, SNP) value the all-SNP call's
  D  the same bits: TBLUP_SCORE_LDS=0 with and without TBLUP_WORKSPACE_MB=1, the same call twice, a model
     alone against inside a batch
  E  four traits: info trait-independent, score / q / cov_effects per trait
  F  against the other entries: cov_effects bit-identical to fit(covariates=Q)'s, effect() of SNP j the last
     cov_effects of fit(covariates=[Q, x_j]), fitness bit-identical to evaluate's, q / dof the sigma2_g of
     log_likelihood_cov
  G  collinear covariates (NaN), a listed SNP equal to a covariate column or monomorphic (exact zeros), a
     monomorphic model panel (NaN), c >= N - r (NaN); n_cov 0 / 17, NaN in cov, h2 = 1, a context without a panel
  H  BlupParallelEvaluator.snp_scores(covariates=)

Tolerance: |got - ref| <= 1e-9 max(1, max |ref|) over the model's candidates (per trait for the score),
tests/score_ref.py::TOL.  Each group prints the largest error it saw (pytest -s); no printed figure is a threshold.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tests import score_cov_ref as A
from tests import score_ref as S
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = A.H2
TOL = A.TOL
N, P = R.N_ANIMALS, R.N_SNPS
I64, F64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = S.close(got, ref)
        self.v = max(self.v, err)
        print("  %-44s %.3e" % (name, err))
        assert err <= TOL, (name, err)

    def check(self, sc, b, ref, name, cols=None):
        """model b of a SnpScores against an adj_ref dictionary (cols: the listed columns of an all-column ref)."""
        u, v = (ref["u"], ref["v"]) if cols is None else (ref["u"][:, cols], ref["v"][cols])
        for t in range(u.shape[0]):
            self.close(sc.score[b, t], u[t], name + " u[%d]" % t)
            self.close(sc.q[b, t], ref["q"][t], name + " q[%d]" % t)
        self.close(sc.info[b], v, name + " v")
        self.close(sc.cov_effects[b], ref["b"], name + " b")
        assert sc.dof[b] == ref["dof"], name

    def show(self):
        print("\nSCORE-COV %s: worst error / max(1, max |ref|) %.3e" % (self.label, self.v))


def _same(a, b, msg=""):
    for f in ("score", "info", "q", "dof", "snps", "cov_effects"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f + " " + msg)


def _cov(c, ones=False):
    return C.make_cov(N, c, ones=ones)


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
        batch = eng.snp_scores(genomes, T, V, H2, covariates=q)
        assert batch.score.shape == (len(genomes), 1, P) and batch.cov_effects.shape == (len(genomes), 1, q.shape[1])
        for i, k in enumerate(C.AUTO_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            w.check(batch, i, A.case_ref(name), name + " (batch)")
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                w.check(eng.snp_scores([genomes[i]], T, V, H2, covariates=q), 0, A.case_ref(name), name + " (alone)")
    w.show()


def test_a_forced_gblup_with_ones(eng):
    pn = A.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.GBLUP_COV[s], ones=True)
        got = eng.snp_scores([pn["genomes"][k] for k in R.GBLUP_KS], T, V, H2, branch="gblup", covariates=q)
        assert np.all(got.dof == len(T) - q.shape[1])
        for i, k in enumerate(R.GBLUP_KS):
            name = "gblup-%d-%d-%s" % (s + (k,))
            w.check(got, i, A.case_ref(name), name)
    w.show()


def test_a_forced_snp_dual(eng):
    pn = A.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in (200, 332, 400) if k > s[0]]
        got = eng.snp_scores([pn["genomes"][k] for k in ks], T, V, H2, branch="snp", covariates=_cov(C.SPLIT_COV[s]))
        assert np.all(got.dof == len(T) - 1 - C.SPLIT_COV[s])
        for i, k in enumerate(ks):
            name = "snp-%d-%d-%s" % (s + (k,))
            w.check(got, i, A.case_ref(name), name)
    w.show()


def test_a_deeper_panel_and_forms_agree(gpu):
    """n_T = 520, k = 513, c = 16: five tile columns, one model forced through the SNP form (TBLUP_FORM=2) and
    the kernel form (TBLUP_FORM=1)."""
    dp = A.deep_panel()
    q = C.make_cov(len(dp["pheno"]), C.DEEP_COV)
    w = _Worst("A deep / forms")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.snp_scores([dp["genome"]], dp["train"], dp["valid"], H2, covariates=q)
            w.check(got[form], 0, A.case_ref("deep"), "form " + form)
    for f in ("score", "info", "q", "cov_effects"):
        w.close(getattr(got["1"], f)[0], getattr(got["2"], f)[0], "form 1 vs 2 " + f)
    w.show()


def test_a_forms_agree_on_the_small_panel(gpu):
    pn = A.panel()
    w = _Worst("A forms, 331 x 600")
    keys = [1, 64, 65, 127, "dup", "neg"]
    genomes = [pn["genomes"][k] for k in keys]
    s = (129, 64)
    T, V = pn["splits"][s]
    q = _cov(C.SPLIT_COV[s])
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.snp_scores(genomes, T, V, H2, covariates=q)
    for i, k in enumerate(keys):
        name = "auto-%d-%d-%s" % (s + (k,))
        for form in ("1", "2"):
            w.check(got[form], i, A.case_ref(name), name + " form " + form)
        for f in ("score", "info", "q"):
            w.close(getattr(got["1"], f)[i], getattr(got["2"], f)[i], name + " form 1 vs 2 " + f)
    w.show()


# ---------------------------------------------------------------------------------------------
# B. LDS at its limit and the workspace path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in A.big_cases()])
def test_b_systems_of_1024_rows_and_above(gpu, name):
    bp = A.big_panel()
    _, g, t, v, qk, br, rows, lds = next(x for x in A.big_cases() if x[0] == name)
    ref = A.big_ref(name)
    assert np.linalg.cond(ref["G"]) <= C.COND_MAX and np.all(ref["v"] >= A.SPAN_MIN * ref["v_plain"]) and ref["dof"] > 0
    w = _Worst("B " + name)
    got, mem = {}, {}
    for knob in ("1", "0"):
        with _engine(bp["geno"], bp["pheno"], {"TBLUP_SCORE_LDS": knob}) as e:
            got[knob] = e.snp_scores([bp[g]], bp[t], bp[v], H2, bp["snps"], branch=br, covariates=bp[qk])
            mem[knob] = e.mem_in_use()
    w.check(got["1"], 0, ref, name)
    _same(got["0"], got["1"], "TBLUP_SCORE_LDS=0")
    # the plan chose LDS exactly where 16 right-hand sides of the system fit 128 KB: without it the workspace
    # also holds the slices
    assert (mem["1"] < mem["0"]) == lds, (name, rows, mem)
    w.show()


# ---------------------------------------------------------------------------------------------
# C. candidate lists
# ---------------------------------------------------------------------------------------------
def test_c_candidate_lists(eng):
    pn = A.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(5)
    genomes = [pn["genomes"][k] for k in (2, 65, 200, 400, "dup")]       # kernel form (k = 400: gblup)
    snp_form = [genomes[1], genomes[4]]
    full = {0: eng.snp_scores(genomes, T, V, H2, covariates=q), 1: eng.snp_scores(snp_form, T, V, H2, covariates=q)}
    for m in A.LIST_LENGTHS:
        lst = A.cand_list(genomes[1], P, m)
        cols = S.wrap(lst, P)
        for which, batch in ((0, genomes), (1, snp_form)):
            got = eng.snp_scores(batch, T, V, H2, lst, covariates=q)
            assert got.score.shape == (len(batch), 1, m) and got.info.shape == (len(batch), m)
            np.testing.assert_array_equal(got.snps, cols)
            np.testing.assert_array_equal(got.score, full[which].score[:, :, cols], err_msg=str(m))
            np.testing.assert_array_equal(got.info, full[which].info[:, cols], err_msg=str(m))
            np.testing.assert_array_equal(got.q, full[which].q, err_msg=str(m))
            np.testing.assert_array_equal(got.cov_effects, full[which].cov_effects, err_msg=str(m))
            if m >= 3:      # the list's last entry repeats its first
                np.testing.assert_array_equal(got.score[:, :, -1], got.score[:, :, 0])
                np.testing.assert_array_equal(got.info[:, -1], got.info[:, 0])


# ---------------------------------------------------------------------------------------------
# D. the same bits
# ---------------------------------------------------------------------------------------------
def test_d_same_bits(eng):
    pn = A.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(16)
    snp = [pn["genomes"][k] for k in (1, 65, 129, 200, "dup")]              # SNP form (every k <= n_T)
    mixed = snp + [pn["genomes"][400]]                                      # kernel form
    lst = A.cand_list(pn["genomes"][65], P, 65)
    ref = {(i, j): eng.snp_scores(g, T, V, H2, c, covariates=q)
           for i, g in enumerate((snp, mixed)) for j, c in enumerate((None, lst))}
    _same(eng.snp_scores(snp, T, V, H2, lst, covariates=q), ref[0, 1], "twice")
    _same(eng.snp_scores(mixed, T, V, H2, lst, covariates=q), ref[1, 1], "twice")
    for env in ({"TBLUP_SCORE_LDS": "0"}, {"TBLUP_SCORE_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}, {"TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for i, g in enumerate((snp, mixed)):
                for j, c in enumerate((None, lst)):
                    _same(e.snp_scores(g, T, V, H2, c, covariates=q), ref[i, j], str(env))
    # a model alone against inside a batch of the same form
    for b in (0, 3):
        one = eng.snp_scores([snp[b]], T, V, H2, lst, covariates=q)
        for f in ("score", "info", "q", "cov_effects"):
            np.testing.assert_array_equal(getattr(one, f)[0], getattr(ref[0, 1], f)[b], err_msg="alone " + f)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": "1"}) as e:
        one = e.snp_scores([mixed[2]], T, V, H2, lst, covariates=q)
        for f in ("score", "info", "q", "cov_effects"):
            np.testing.assert_array_equal(getattr(one, f)[0], getattr(ref[1, 1], f)[2], err_msg="alone, kernel form " + f)


# ---------------------------------------------------------------------------------------------
# E. traits
# ---------------------------------------------------------------------------------------------
def test_e_four_traits(gpu):
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(5)
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    lst = A.cand_list(pn["genomes"][65], P, 33)
    w = _Worst("E traits")
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, 0])) as e:
        single = [e.snp_scores(b, T, V, H2, lst, covariates=q) for b in batches]
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :4])) as e:
        for i, b in enumerate(batches):
            got = e.snp_scores(b, T, V, H2, lst, covariates=q)
            assert got.score.shape == (len(b), 4, len(lst)) and got.q.shape == (len(b), 4)
            assert got.cov_effects.shape == (len(b), 4, 5)
            np.testing.assert_array_equal(got.info, single[i].info)          # info does not see the phenotypes
            for m, g in enumerate(b):
                w.check(got, m, A.adj_ref(g, T, pn["geno"], pn["Y"][:, :4], q, H2, snps=lst), "4 traits %d %d" % (i, m))
                w.close(got.score[m, 0], single[i].score[m, 0], "trait 0 against the single-trait run")
    w.show()


# ---------------------------------------------------------------------------------------------
# F. against the other entries
# ---------------------------------------------------------------------------------------------
def test_f_cov_effects_and_fitness_are_the_other_entries(eng):
    from tblup_amd.engine import concat_genomes
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(16)
    lst = A.cand_list(pn["genomes"][65], P, 33)
    for genomes in ([pn["genomes"][k] for k in (63, 64, 127)], [pn["genomes"][k] for k in C.AUTO_KEYS]):
        sc = eng.snp_scores(genomes, T, V, H2, lst, covariates=q)
        models = eng.fit(genomes, T, V, H2, covariates=q)
        np.testing.assert_array_equal(sc.cov_effects, np.stack([m.cov_effects for m in models]))
        fit = eng.evaluate(genomes, T, V, H2)
        idx, off = concat_genomes(genomes)
        B = len(genomes)
        f2, u2, v2 = np.empty(B), np.empty((B, 1, len(lst))), np.empty((B, len(lst)))
        rc = eng._lib.tblup_snp_score_cov_batch(
            eng._ctx, eng.split_id(T, V), q.ctypes.data_as(F64), q.shape[1], lst.ctypes.data_as(I64), len(lst),
            idx.ctypes.data_as(I64), off.ctypes.data_as(I64), B, H2, 0, f2.ctypes.data_as(F64), u2.ctypes.data_as(F64),
            v2.ctypes.data_as(F64), None, None)
        assert rc == 0
        np.testing.assert_array_equal(f2, fit)
        np.testing.assert_array_equal(u2, sc.score)
        np.testing.assert_array_equal(v2, sc.info)


def test_f_effect_is_the_gls_effect_of_the_appended_snp(eng):
    """u_P / v_P of SNP j = the last covariate effect of fit(covariates=[Q, x_j]), in both forms (snp models: the
    fit centres the appended column over the train rows itself)."""
    pn = A.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(5)
    w = _Worst("F effect against fit(covariates=[Q, x_j])")
    cols = S.wrap(A.cand_list(pn["genomes"][65], P, 4), P)
    for genomes in ([pn["genomes"][k] for k in (65, 200)], [pn["genomes"][k] for k in (65, 200, S.K300)]):
        br = "auto" if len(genomes) == 2 else "snp"      # SNP form; kernel form (k = 300 > n_T under snp)
        eff = eng.snp_scores(genomes, T, V, H2, cols, branch=br, covariates=q).effect()
        for j, col in enumerate(cols):
            q1 = np.ascontiguousarray(np.hstack([q, pn["geno"][:, [col]].astype(np.float64)]))
            models = eng.fit(genomes, T, V, H2, branch=br, covariates=q1)
            last = np.array([m.cov_effects[0, -1] for m in models])
            w.close(eff[:, 0, j], last, "SNP %d" % col)
    w.show()


def test_f_q_over_dof_is_the_likelihoods_sigma2(eng):
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(16)
    w = _Worst("F sigma2_g")
    for genomes in ([pn["genomes"][k] for k in (1, 63, 64, 127, "dup", "neg")], [pn["genomes"][k] for k in C.AUTO_KEYS]):
        sc = eng.snp_scores(genomes, T, V, H2, [0, 1], covariates=q)
        _, s2 = eng.log_likelihood_cov(genomes, T, V, H2, return_sigma2=True, covariates=q)
        w.close(sc.q[:, 0] / sc.dof, s2, "q / dof")
    w.show()


# ---------------------------------------------------------------------------------------------
# G. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_g_collinear_covariates_give_nan(eng):
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(3)
    two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 2]], axis=1))
    for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][200]]):     # SNP form, kernel form
        sc = eng.snp_scores(genomes, T, V, H2, [3, 4, 5], covariates=two)
        for f in ("score", "info", "q", "cov_effects"):
            assert np.all(np.isnan(getattr(sc, f))), f
    # the model beside it in the batch is unharmed: a column constant over the train rows is collinear only under snp
    const = q.copy()
    const[T, 1] = 1.0
    sc = eng.snp_scores([pn["genomes"][200], pn["genomes"][400]], T, V, H2, [3, 4, 5], covariates=const)
    assert np.all(np.isnan(sc.score[0])) and np.all(np.isnan(sc.info[0])) and np.all(np.isnan(sc.q[0]))
    ref = A.adj_ref(pn["genomes"][400], T, pn["geno"], pn["pheno"], const, H2, snps=[3, 4, 5])
    _Worst("G beside a NaN model").check(sc, 1, ref, "gblup model")


def test_g_snp_in_the_span_and_monomorphic_snp_give_exact_zeros(gpu):
    pn = A.panel()
    geno = pn["geno"].copy()
    T, V = pn["splits"][129, 64]
    geno[T, 9] = 0                                   # constant over the train rows
    q = _cov(5)
    q[:, 2] = geno[:, 11]                            # covariate 2 is SNP 11
    with _engine(geno, pn["pheno"]) as e:
        for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][200]]):     # SNP form, kernel form
            sc = e.snp_scores(genomes, T, V, H2, [5, 11, 9, 11 - P], covariates=q)
            for j in (1, 2, 3):
                assert np.all(sc.score[:, :, j] == 0) and np.all(sc.info[:, j] == 0), j
            assert np.all(sc.info[:, 0] > 0) and np.all(np.isfinite(sc.q))
            chi = sc.chi2()
            assert np.all(np.isnan(chi[:, :, 1:])) and np.all(np.isfinite(chi[:, :, 0]))
            ref = A.adj_ref(genomes[0], T, geno, pn["pheno"], q, H2, snps=[5, 11, 9, 11 - P])
            _Worst("G zeros").check(sc, 0, ref, "beside the zeros")


def test_g_monomorphic_model_panel_and_no_degrees_of_freedom_give_nan(gpu):
    pn = A.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            q = _cov(5, ones=(br == "gblup"))
            sc = e.snp_scores(genomes, T, V, H2, [3, 4], branch=br, covariates=q)
            assert np.all(np.isnan(sc.score[:2])) and np.all(np.isnan(sc.info[:2])) and np.all(np.isnan(sc.q[:2]))
            _Worst("G").check(sc, 2, A.adj_ref(genomes[2], T, geno, pn["pheno"], q, H2, br, snps=[3, 4]), br)
        # c >= N - r: 17 train animals, the intercept and 16 covariates
        few = T[:17]
        sc = e.snp_scores([pn["genomes"][64][:5]], few, V, H2, [3, 4], branch="snp", covariates=_cov(16))
        assert sc.dof[0] == 0
        assert np.all(np.isnan(sc.score)) and np.all(np.isnan(sc.info)) and np.all(np.isnan(sc.q))


def test_g_errors(eng):
    from tblup_amd import _native
    from tblup_amd._native import TblupError, TblupIndexError
    pn = A.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    q = _cov(5)
    with pytest.raises(TblupError):
        eng.snp_scores(g, T, V, 1.0, covariates=q)
    with pytest.raises(TblupIndexError):
        eng.snp_scores(g, T, V, H2, [0, P], covariates=q)
    for bad in (np.zeros((N, 0)), np.zeros((N, 17)), np.full((N, 2), np.nan)):
        with pytest.raises(ValueError):
            eng.snp_scores(g, T, V, H2, covariates=bad)
    empty = eng.snp_scores(g * 3, T, V, H2, [], covariates=q)
    assert empty.score.shape == (3, 1, 0) and empty.cov_effects.shape == (3, 1, 5) and np.all(np.isnan(empty.q))
    # the entry's own argument checks
    from tblup_amd.engine import concat_genomes
    idx, off = concat_genomes(g)
    lst = np.array([1, 2], dtype=np.int64)
    u, v = np.empty((1, 1, 2)), np.empty((1, 2))
    sid = eng.split_id(T, V)

    def call(ctx, cov, nc, h2=H2):
        return eng._lib.tblup_snp_score_cov_batch(
            ctx, sid, None if cov is None else cov.ctypes.data_as(F64), nc, lst.ctypes.data_as(I64), 2,
            idx.ctypes.data_as(I64), off.ctypes.data_as(I64), 1, h2, 0, None, u.ctypes.data_as(F64), v.ctypes.data_as(F64),
            None, None)
    wide = np.zeros((N, 17))
    assert call(eng._ctx, wide, 0) != 0 and b"n_cov" in eng._lib.tblup_last_error()
    assert call(eng._ctx, wide, 17) != 0 and b"n_cov" in eng._lib.tblup_last_error()
    assert call(eng._ctx, None, 2) != 0
    nanq = q.copy()
    nanq[7, 3] = np.nan
    assert call(eng._ctx, nanq, 5) != 0 and b"finite" in eng._lib.tblup_last_error()
    assert call(eng._ctx, q, 5, 1.0) != 0
    assert call(eng._ctx, q, 5) == 0
    ctx = ctypes.c_void_p()
    assert eng._lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        assert call(ctx, q, 5) == _native.ERR_STATE and b"panel" in eng._lib.tblup_last_error()
    finally:
        eng._lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# H. evaluator level
# ---------------------------------------------------------------------------------------------
def test_h_evaluator_snp_scores(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = A.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, H2, False)
    rem.removed = np.array((5, 17, 301, 599), dtype=np.float64)
    q = _cov(5)
    w = _Worst("H")
    with E.BlupParallelEvaluator(gp, pp, H2, snp_remover=rem) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        lst = A.cand_list(pop[1].genome, P, 33)
        sc = ev.snp_scores(pop, lst, covariates=q)
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        _same(sc, ev.engine.snp_scores(genomes, train, ev.testing_indices, H2, lst, covariates=q))
        for i, g in enumerate(genomes):
            w.check(sc, i, A.adj_ref(g, train, pn["geno"], pn["pheno"], q, H2, snps=lst), "model %d" % i)
        plain = ev.snp_scores(pop, lst)
        assert plain.cov_effects is None and np.all(plain.dof == sc.dof + 5)
    w.show()
