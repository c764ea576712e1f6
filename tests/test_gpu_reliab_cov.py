"""Reliabilities, the error variance of predicted values and the covariates' sampling covariance under the model
with fixed-effect covariates (tblup_reliability_cov_batch: k_covar in keep mode, k_reliab's covariate-adjusted
instances, k_cov_cov) on the GPU, against the dense float64 restatement of tests/reliab_cov_ref.py (the mixed-model
equations in SNP space, itself within 1e-11 of the header's V-form in longdouble: tests/test_reliab_cov_host.py).

Panels: tests/covar_ref.py's cases -- 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64),
(257, 70), covariate counts 1, 5, 16 going round with the split; the deeper 700 x 800 panel; and the 1200 x 1100
synthetic panel whose systems have exactly 1024 rows (the largest whose right-hand sides live in LDS) and 1152.

  A  against the restatement, all animals as the list: auto branch (ragged batch: kernel form; one genome alone:
     SNP form where k <= n_T), forced gblup with the column of ones, forced snp at n_T < k, the deeper panel in
     both forms
  B  the 1200 x 1100 panel: 1024 rows in both forms (the plan keeps the right-hand sides in LDS: the workspace
     is smaller than with TBLUP_RELIAB_LDS=0) and 1152 rows (workspace either way), c = 16
  C  animal lists of length 1, 15, 16, 17, 33, 65 with repeats and animals outside the split: every value the
     all-animal call's, bit for bit
  D  the same bits: TBLUP_RELIAB_LDS=0 / TBLUP_SCORE_LDS=0 with and without TBLUP_WORKSPACE_MB=1, the same call
     twice, a model alone against inside a batch, plain reliability() before and after a covariate call
  E  four traits: one reliability per (model, animal), models per trait
  F  against the other entries: models bit-identical to fit(covariates=Q)'s, cov_cov[-1, -1] of [Q, x_j] against
     1 / snp_scores(covariates=Q).info[j], rel_cov <= reliability() + TOL
  G  collinear covariates (NaN model), a monomorphic panel (NaN), an animal with K_aa = 0 (NaN for it alone);
     n_cov 0 / 17, NaN in cov, an animal id out of range (TBLUP_ERR_ARG), a context without a panel
     (TBLUP_ERR_STATE), empty lists
  H  BlupParallelEvaluator.reliability_cov(covariates=)

Tolerance: |got - ref| <= 1e-9 max(1, max |ref|) over the model's animals (over the matrix for cov_cov),
tests/score_ref.py::TOL as tests/test_gpu_score_cov.py applies it.  Each group prints the largest error it saw
(pytest -s); no printed figure is a threshold.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tests import reliab_cov_ref as Q
from tests import score_ref as S
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = Q.H2
TOL = Q.TOL
N, P = R.N_ANIMALS, R.N_SNPS
HERD = np.arange(N)
I64, F64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
ALL = dict(return_pev=True, return_cov_cov=True)


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = S.close(got, ref)
        self.v = max(self.v, err)
        print("  %-48s %.3e" % (name, err))
        assert err <= TOL, (name, err)

    def check(self, got, b, ref, name, an=None):
        """model b of a CovReliability against a mme_ref dictionary (an: the listed animals of an all-animal ref)."""
        rel, pev = (ref["rel"], ref["pev"]) if an is None else (ref["rel"][an], ref["pev"][an])
        self.close(got.reliability[b], rel, name + " rel")
        self.close(got.pev_total[b], pev, name + " pev")
        self.close(got.cov_cov[b], ref["cov_cov"], name + " cov_cov")
        np.testing.assert_array_equal(got.cov_cov[b], got.cov_cov[b].T, err_msg=name)

    def show(self):
        print("\nRELIAB-COV %s: worst error / max(1, max |ref|) %.3e" % (self.label, self.v))


def _same(a, b, msg=""):
    for f in ("reliability", "pev_total", "cov_cov"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f + " " + msg)


def _cov(c, ones=False):
    return C.make_cov(N, c, ones=ones)


@pytest.fixture(scope="module")
def eng(gpu):
    pn = Q.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    pn = Q.panel()
    genomes = [pn["genomes"][k] for k in C.AUTO_KEYS]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.SPLIT_COV[s])
        batch = eng.reliability_cov(genomes, T, V, H2, HERD, covariates=q, **ALL)
        c = q.shape[1]
        assert batch.reliability.shape == (len(genomes), N) and batch.cov_cov.shape == (len(genomes), c, c)
        assert batch.models is None
        for i, k in enumerate(C.AUTO_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            w.check(batch, i, Q.case_ref(name), name + " (batch)")
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                w.check(eng.reliability_cov([genomes[i]], T, V, H2, HERD, covariates=q, **ALL), 0, Q.case_ref(name),
                        name + " (alone)")
    w.show()


def test_a_forced_gblup_with_ones(eng):
    pn = Q.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.GBLUP_COV[s], ones=True)
        got = eng.reliability_cov([pn["genomes"][k] for k in R.GBLUP_KS], T, V, H2, HERD, branch="gblup", covariates=q,
                                  **ALL)
        for i, k in enumerate(R.GBLUP_KS):
            name = "gblup-%d-%d-%s" % (s + (k,))
            w.check(got, i, Q.case_ref(name), name)
    w.show()


def test_a_forced_snp_dual(eng):
    pn = Q.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in (200, 332, 400) if k > s[0]]
        got = eng.reliability_cov([pn["genomes"][k] for k in ks], T, V, H2, HERD, branch="snp",
                                  covariates=_cov(C.SPLIT_COV[s]), **ALL)
        for i, k in enumerate(ks):
            name = "snp-%d-%d-%s" % (s + (k,))
            w.check(got, i, Q.case_ref(name), name)
    w.show()


def test_a_deeper_panel_in_both_forms(gpu):
    """n_T = 520, k = 513, c = 16: five tile columns, one model forced through the SNP form (TBLUP_FORM=2) and
    the kernel form (TBLUP_FORM=1)."""
    dp = Q.deep_panel()
    n = len(dp["pheno"])
    q = C.make_cov(n, C.DEEP_COV)
    w = _Worst("A deep / forms")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.reliability_cov([dp["genome"]], dp["train"], dp["valid"], H2, np.arange(n), covariates=q, **ALL)
            w.check(got[form], 0, Q.case_ref("deep"), "form " + form)
    for f in ("reliability", "pev_total", "cov_cov"):
        w.close(getattr(got["1"], f)[0], getattr(got["2"], f)[0], "form 1 vs 2 " + f)
    w.show()


# ---------------------------------------------------------------------------------------------
# B. LDS at its limit and the workspace path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in Q.big_cases()])
def test_b_systems_of_1024_rows_and_above(gpu, name):
    bp = Q.big_panel()
    _, g, t, v, qk, br, rows, lds = next(x for x in Q.big_cases() if x[0] == name)
    ref = Q.big_ref(name)                                   # asserts cond(G) <= COND_MAX and K_aa > 0
    herd = np.arange(Q.A.BIG_N)
    w = _Worst("B " + name)
    got, mem = {}, {}
    for knob in ("1", "0"):
        with _engine(bp["geno"], bp["pheno"], {"TBLUP_RELIAB_LDS": knob}) as e:
            got[knob] = e.reliability_cov([bp[g]], bp[t], bp[v], H2, herd, branch=br, covariates=bp[qk], **ALL)
            mem[knob] = e.mem_in_use()
    w.check(got["1"], 0, ref, name)
    _same(got["0"], got["1"], "TBLUP_RELIAB_LDS=0")
    # the plan chose LDS exactly where 16 right-hand sides of the system fit 128 KB: without it the workspace
    # also holds the slices
    assert (mem["1"] < mem["0"]) == lds, (name, rows, mem)
    w.show()


# ---------------------------------------------------------------------------------------------
# C. animal lists
# ---------------------------------------------------------------------------------------------
def test_c_animal_lists(eng):
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(5)
    genomes = [pn["genomes"][k] for k in (2, 65, 200, 400, "dup")]       # kernel form (k = 400: gblup)
    snp_form = [genomes[1], genomes[4]]
    full = {0: eng.reliability_cov(genomes, T, V, H2, HERD, covariates=q, **ALL),
            1: eng.reliability_cov(snp_form, T, V, H2, HERD, covariates=q, **ALL)}
    outside = np.setdiff1d(HERD, np.concatenate([T, V]))
    assert len(outside) > 0
    for m in Q.LIST_LENGTHS:
        lst = Q.animal_list(N, T, m)
        if m >= 2:
            lst[1] = outside[m % len(outside)]            # in no split role at all
        for which, batch in ((0, genomes), (1, snp_form)):
            got = eng.reliability_cov(batch, T, V, H2, lst, covariates=q, **ALL)
            assert got.reliability.shape == (len(batch), m) and got.pev_total.shape == (len(batch), m)
            np.testing.assert_array_equal(got.reliability, full[which].reliability[:, lst], err_msg=str(m))
            np.testing.assert_array_equal(got.pev_total, full[which].pev_total[:, lst], err_msg=str(m))
            np.testing.assert_array_equal(got.cov_cov, full[which].cov_cov, err_msg=str(m))
            if m >= 3:      # the list's last entry repeats its first
                np.testing.assert_array_equal(got.reliability[:, -1], got.reliability[:, 0])


# ---------------------------------------------------------------------------------------------
# D. the same bits
# ---------------------------------------------------------------------------------------------
def test_d_same_bits(eng):
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(16)
    snp = [pn["genomes"][k] for k in (1, 65, 129, 200, "dup")]              # SNP form (every k <= n_T)
    mixed = snp + [pn["genomes"][400]]                                      # kernel form
    lst = Q.animal_list(N, T, 65)
    plain_before = [eng.reliability(g, T, V, H2, HERD) for g in (snp, mixed)]
    ref = {(i, j): eng.reliability_cov(g, T, V, H2, a, covariates=q, **ALL)
           for i, g in enumerate((snp, mixed)) for j, a in enumerate((HERD, lst))}
    _same(eng.reliability_cov(snp, T, V, H2, lst, covariates=q, **ALL), ref[0, 1], "twice")
    _same(eng.reliability_cov(mixed, T, V, H2, lst, covariates=q, **ALL), ref[1, 1], "twice")
    # plain reliability() on the same engine is what it was before the covariate calls
    for g, before in zip((snp, mixed), plain_before):
        np.testing.assert_array_equal(eng.reliability(g, T, V, H2, HERD), before)
    off = {"TBLUP_RELIAB_LDS": "0", "TBLUP_SCORE_LDS": "0"}
    for env in (off, dict(off, TBLUP_WORKSPACE_MB="1"), {"TBLUP_WORKSPACE_MB": "1"}, {"TBLUP_RELIAB_LDS": "0"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for i, g in enumerate((snp, mixed)):
                for j, a in enumerate((HERD, lst)):
                    _same(e.reliability_cov(g, T, V, H2, a, covariates=q, **ALL), ref[i, j], str(env))
            np.testing.assert_array_equal(e.reliability(mixed, T, V, H2, HERD), plain_before[1], err_msg=str(env))
    # a model alone against inside a batch of the same form
    for b in (0, 3):
        one = eng.reliability_cov([snp[b]], T, V, H2, lst, covariates=q, **ALL)
        for f in ("reliability", "pev_total", "cov_cov"):
            np.testing.assert_array_equal(getattr(one, f)[0], getattr(ref[0, 1], f)[b], err_msg="alone " + f)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": "1"}) as e:
        one = e.reliability_cov([mixed[2]], T, V, H2, lst, covariates=q, **ALL)
        for f in ("reliability", "pev_total", "cov_cov"):
            np.testing.assert_array_equal(getattr(one, f)[0], getattr(ref[1, 1], f)[2], err_msg="alone, kernel form " + f)
    # the optional outputs change nothing in the ones that are asked for
    bare = eng.reliability_cov(mixed, T, V, H2, lst, covariates=q)
    assert bare.pev_total is None and bare.cov_cov is None and bare.models is None
    np.testing.assert_array_equal(bare.reliability, ref[1, 1].reliability)
    with_models = eng.reliability_cov(mixed, T, V, H2, lst, covariates=q, return_models=True, **ALL)
    _same(with_models, ref[1, 1], "with the models")


# ---------------------------------------------------------------------------------------------
# E. traits
# ---------------------------------------------------------------------------------------------
def test_e_four_traits(gpu):
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(5)
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    lst = Q.animal_list(N, T, 33)
    w = _Worst("E traits")
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, 0])) as e:
        single = [e.reliability_cov(b, T, V, H2, lst, covariates=q, **ALL) for b in batches]
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :4])) as e:
        for i, b in enumerate(batches):
            got = e.reliability_cov(b, T, V, H2, lst, covariates=q, return_models=True, **ALL)
            assert got.reliability.shape == (len(b), len(lst)) and got.cov_cov.shape == (len(b), 5, 5)
            _same(got, single[i], "no phenotype enters")
            fitted = e.fit(b, T, V, H2, covariates=q)
            _, s2 = e.log_likelihood_cov(b, T, V, H2, covariates=q, return_sigma2=True)
            se = got.cov_stderr(s2)
            assert se.shape == (len(b), 4, 5) and np.all(se > 0)
            for m, g in enumerate(b):
                assert got.models[m].effects.shape == (4, len(g)) and got.models[m].cov_effects.shape == (4, 5)
                np.testing.assert_array_equal(got.models[m].cov_effects, fitted[m].cov_effects)
                np.testing.assert_array_equal(got.models[m].effects, fitted[m].effects)
                w.check(got, m, Q.mme_ref(g, T, pn["geno"], q, H2, animals=lst), "4 traits %d %d" % (i, m))
    w.show()


# ---------------------------------------------------------------------------------------------
# F. against the other entries
# ---------------------------------------------------------------------------------------------
def test_f_models_are_fit_covariates_models(eng):
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(16)
    lst = Q.animal_list(N, T, 33)
    for genomes in ([pn["genomes"][k] for k in (63, 64, 127)], [pn["genomes"][k] for k in C.AUTO_KEYS]):
        got = eng.reliability_cov(genomes, T, V, H2, lst, covariates=q, return_models=True)
        fitted = eng.fit(genomes, T, V, H2, covariates=q)
        assert len(got.models) == len(fitted)
        for a, b in zip(got.models, fitted):
            for f in ("indices", "effects", "intercept", "center", "cov_effects", "cov_center"):
                np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
            assert a.fitness == b.fitness and a.branch == b.branch


def test_f_cov_cov_of_the_appended_snp_is_the_score_tests_information(eng):
    """(G^-1)[-1, -1] of [Q, x_j] = 1 / v_P(j), in both forms (snp models: the entry centres the appended column
    over the train rows itself)."""
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    q = _cov(5)
    w = _Worst("F cov_cov against 1 / info")
    cols = S.wrap(S.cand_list(pn["genomes"][65], P, 4), P)
    none = np.zeros(0, dtype=np.int64)
    for genomes in ([pn["genomes"][k] for k in (65, 200)], [pn["genomes"][k] for k in (65, 200, S.K300)]):
        br = "auto" if len(genomes) == 2 else "snp"      # SNP form; kernel form (k = 300 > n_T under snp)
        info = eng.snp_scores(genomes, T, V, H2, cols, branch=br, covariates=q).info
        for j, col in enumerate(cols):
            q1 = np.ascontiguousarray(np.hstack([q, pn["geno"][:, [col]].astype(np.float64)]))
            cc = eng.reliability_cov(genomes, T, V, H2, none, branch=br, covariates=q1, return_cov_cov=True).cov_cov
            assert cc.shape == (len(genomes), 6, 6)
            w.close(cc[:, -1, -1], 1.0 / info[:, j], "SNP %d" % col)
    w.show()


def test_f_never_above_the_plain_reliability(eng):
    pn = Q.panel()
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        q = _cov(C.SPLIT_COV[s])
        for genomes in ([pn["genomes"][k] for k in (1, 64, 65)], [pn["genomes"][k] for k in C.AUTO_KEYS]):
            plain = eng.reliability(genomes, T, V, H2, HERD)
            got = eng.reliability_cov(genomes, T, V, H2, HERD, covariates=q, return_pev=True)
            assert np.all(got.reliability <= plain + TOL), float(np.max(got.reliability - plain))
            assert np.all(got.pev_total > 0)


# ---------------------------------------------------------------------------------------------
# G. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_g_collinear_covariates_give_nan(eng):
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    q = _cov(3)
    two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 2]], axis=1))
    for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][200]]):     # SNP form, kernel form
        got = eng.reliability_cov(genomes, T, V, H2, [3, 4, 5], covariates=two, return_models=True, **ALL)
        for f in ("reliability", "pev_total", "cov_cov"):
            assert np.all(np.isnan(getattr(got, f))), f
        assert all(np.all(np.isnan(m.cov_effects)) and np.all(np.isnan(m.effects)) for m in got.models)
    # the model beside it in the batch is unharmed: a column constant over the train rows is collinear only under snp
    const = q.copy()
    const[T, 1] = 1.0
    got = eng.reliability_cov([pn["genomes"][200], pn["genomes"][400]], T, V, H2, [3, 4, 5], covariates=const, **ALL)
    assert np.all(np.isnan(got.reliability[0])) and np.all(np.isnan(got.pev_total[0])) and np.all(np.isnan(got.cov_cov[0]))
    ref = Q.mme_ref(pn["genomes"][400], T, pn["geno"], const, H2, animals=[3, 4, 5])
    _Worst("G beside a NaN model").check(got, 1, ref, "gblup model")


def test_g_monomorphic_panel_and_an_animal_with_zero_k_aa(gpu):
    pn = Q.panel()
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
    q = _cov(5)
    lst = np.array([int(T[0]), a0, int(V[0]), a0], dtype=np.int64)
    for form in ("2", "1"):
        with _engine(geno, pn["pheno"], {"TBLUP_FORM": form}) as e:
            genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64], np.array([2])]
            got = e.reliability_cov(genomes, T, V, H2, lst, branch="snp", covariates=q, **ALL)
            for f in ("reliability", "pev_total", "cov_cov"):
                assert np.all(np.isnan(getattr(got, f)[:2])), (form, f)
            ref = Q.mme_ref(genomes[2], T, geno, q, H2, "snp", animals=lst)
            _Worst("G beside the NaN models").check(got, 2, ref, "form " + form)
            # K_aa = 0: NaN for that animal alone
            assert np.all(np.isnan(got.reliability[3, [1, 3]])) and np.all(np.isnan(got.pev_total[3, [1, 3]])), form
            assert np.all(np.isfinite(got.reliability[3, [0, 2]])) and np.all(np.isfinite(got.cov_cov[3])), form
            one = Q.mme_ref(genomes[3], T, geno, q, H2, "snp", animals=lst[[0, 2]])
            w = _Worst("G beside the K_aa = 0 animal")
            w.close(got.reliability[3, [0, 2]], one["rel"], "rel form " + form)
            w.close(got.pev_total[3, [0, 2]], one["pev"], "pev form " + form)


def test_g_errors_and_empty_lists(eng):
    from tblup_amd import _native
    from tblup_amd._native import TblupError, TblupIndexError
    from tblup_amd.engine import concat_genomes
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    q = _cov(5)
    with pytest.raises(TblupIndexError):
        eng.reliability_cov([np.array([0, P])], T, V, H2, [1], covariates=q)
    with pytest.raises(TblupError):
        eng.reliability_cov(g, T, V, H2, [0, N], covariates=q)
    for bad in (np.zeros((N, 0)), np.zeros((N, 17)), np.full((N, 2), np.nan)):
        with pytest.raises(ValueError):
            eng.reliability_cov(g, T, V, H2, [1], covariates=bad)
    # empty lists: no animals -- cov_cov and the models are still filled; no models -- empty arrays
    empty = eng.reliability_cov(g * 3, T, V, H2, [], covariates=q, return_models=True, **ALL)
    assert empty.reliability.shape == (3, 0) and empty.pev_total.shape == (3, 0)
    full = eng.reliability_cov(g * 3, T, V, H2, [1, 2], covariates=q, return_models=True, **ALL)
    np.testing.assert_array_equal(empty.cov_cov, full.cov_cov)
    assert np.all(np.isfinite(empty.cov_cov))
    np.testing.assert_array_equal(empty.models[2].cov_effects, full.models[2].cov_effects)
    none = eng.reliability_cov([], T, V, H2, [1, 2], covariates=q, return_models=True, **ALL)
    assert none.reliability.shape == (0, 2) and none.cov_cov.shape == (0, 5, 5) and none.models == []
    # the entry's own argument checks
    idx, off = concat_genomes(g)
    lst = np.array([1, 2], dtype=np.int64)
    rel = np.empty((1, 2))
    sid = eng.split_id(T, V)

    def call(ctx, cov, nc, animals=lst, rel_out=rel, **out):
        ptr = {k: v.ctypes.data_as(F64) for k, v in out.items()}
        return eng._lib.tblup_reliability_cov_batch(
            ctx, sid, None if cov is None else cov.ctypes.data_as(F64), nc, animals.ctypes.data_as(I64), len(animals),
            idx.ctypes.data_as(I64), off.ctypes.data_as(I64), 1, H2, 0, None, ptr.get("cov_effects"),
            ptr.get("cov_center"), ptr.get("intercept"), ptr.get("center"), ptr.get("effects"),
            None if rel_out is None else rel_out.ctypes.data_as(F64), None, None)
    wide = np.zeros((N, 17))
    assert call(eng._ctx, wide, 0) == _native.ERR_ARG and b"n_cov" in eng._lib.tblup_last_error()
    assert call(eng._ctx, wide, 17) == _native.ERR_ARG and b"n_cov" in eng._lib.tblup_last_error()
    assert call(eng._ctx, None, 2) == _native.ERR_ARG
    nanq = q.copy()
    nanq[7, 3] = np.nan
    assert call(eng._ctx, nanq, 5) == _native.ERR_ARG and b"finite" in eng._lib.tblup_last_error()
    for bad in (np.array([1, N], dtype=np.int64), np.array([-1, 2], dtype=np.int64)):
        assert call(eng._ctx, q, 5, animals=bad) == _native.ERR_ARG and b"animal" in eng._lib.tblup_last_error()
    assert call(eng._ctx, q, 5, rel_out=None) == _native.ERR_ARG
    assert call(eng._ctx, q, 5, cov_effects=np.empty((1, 1, 5))) == _native.ERR_ARG      # the group, or none of it
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
def test_h_evaluator_reliability(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = Q.panel()
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
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        lst = Q.animal_list(N, train, 33)
        got = ev.reliability_cov(pop, lst, covariates=q, **ALL)
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        _same(got, ev.engine.reliability_cov(genomes, train, ev.testing_indices, H2, lst, covariates=q, **ALL))
        for i, g in enumerate(genomes):
            w.check(got, i, Q.mme_ref(g, train, pn["geno"], q, H2, animals=lst), "model %d" % i)
        plain = ev.reliability(pop, lst)
        assert isinstance(plain, np.ndarray) and np.all(got.reliability <= plain + TOL)
    w.show()
