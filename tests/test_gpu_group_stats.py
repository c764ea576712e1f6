"""Score statistics and the restricted likelihood of h2 under a class fixed effect (tblup_snp_score_group_batch,
tblup_loglik_group_batch: k_fixed_gls in keep mode, k_snpscore's wide-design instances, k_loglik with a column count
per plane) on the GPU, against tests/group_stats_ref.py: score_cov_ref's dense float64 restatement on the expanded
design [Q, Z] (within 1e-14 of its longdouble form: tests/test_group_stats_host.py).

Panels and designs are tests/group_ref.py's: 331 animals x 600 SNPs with 18 levels (17 / 18 columns: one column in
the second slab), 40 levels + 3 covariates (the last slab partial) and 113 levels + 15 covariates (127 / 128 columns,
the limit); the deeper 700 x 800 panel with 40 levels; and score_cov_ref's 1200 x 1100 panel with 24 levels + 3
covariates, whose systems have exactly 1024 rows (right-hand sides in LDS) and 1152 (workspace).

  A  against the restatement over all columns: u_P, v_P, q_P, dof, the effects; loglik and sigma2_g at H2S as a shared
     grid and as a (G, B) matrix -- auto branch (a ragged batch: kernel form, gblup and snp models of different C_m; a
     genome alone: SNP form), forced gblup, forced snp at k > n_T, the deeper panel and one model in both forms
  B  the 1200 x 1100 panel: 1024 rows in both forms and 1152 rows, 33 listed SNPs, with and without TBLUP_SCORE_LDS
  C  candidate lists of length 1, 15, 16, 17, 33, 65: every (model, SNP) value the all-SNP call's, bit for bit
  D  the same bits: TBLUP_SCORE_LDS=0 with and without TBLUP_WORKSPACE_MB=1, the same call twice, a model alone
     against inside a batch
  E  four traits: info trait-independent, score / q / loglik per trait
  F  against the other entries: the effects bit-identical to fit(groups=)'s; a design of <= 16 columns bit-identical
     to snp_scores(covariates=[Q, Z]) and log_likelihood_cov; q_P / dof the likelihood's sigma2_g; effect() of SNP j
     the last covariate effect of fit(covariates=[Q, x_j], groups=); string labels; another reference level
  G  collinear designs (NaN), 113 levels + 15 covariates on 127 train animals (NaN, no error), a listed SNP equal to a
     covariate or monomorphic (exact zeros), a monomorphic model panel (NaN); 129 columns, wrong label shapes, float
     labels; the entries' own argument errors; an empty batch and an empty list
  H  estimate_h2_group against the restatement's search; BlupParallelEvaluator's three methods

Tolerance: score_ref.TOL / loglik_ref.TOL, |got - ref| <= 1e-9 max(1, max |ref|).  Each group prints the largest
error it saw (pytest -s); no printed figure is a threshold.
"""
import ctypes

import numpy as np
import pytest

from tests import covar_ref as C
from tests import group_ref as G
from tests import group_stats_ref as GS
from tests import loglik_ref as LR
from tests import model_ref as R
from tests import score_cov_ref as A
from tests import score_ref as S
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2, H2S, TOL = GS.H2, GS.H2S, GS.TOL
N, P = R.N_ANIMALS, R.N_SNPS
I64, F64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
FIELDS = ("score", "info", "q", "dof", "snps", "group_effects", "group_levels")


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name, measure=S.close):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), name
        err = measure(got, ref)
        self.v = max(self.v, err)
        assert err <= TOL, (name, err)

    def check(self, sc, b, ref, name, cols=None):
        """model b of a SnpScores against a group_stats_ref dictionary (cols: the listed columns of an all-column ref)."""
        u, v = (ref["u"], ref["v"]) if cols is None else (ref["u"][:, cols], ref["v"][cols])
        for t in range(u.shape[0]):
            self.close(sc.score[b, t], u[t], name + " u[%d]" % t)
            self.close(sc.q[b, t], ref["q"][t], name + " q[%d]" % t)
        self.close(sc.info[b], v, name + " v")
        assert sc.dof[b] == ref["dof"], (name, sc.dof[b], ref["dof"])
        # the expanded design's effects: the covariates', then the levels' (0 at the reference level under snp)
        L = len(sc.group_levels)
        nc = ref["b"].shape[1] - L + (ref["branch"] == "snp")
        ge = np.zeros((ref["b"].shape[0], L))
        ge[:, L - (ref["b"].shape[1] - nc):] = ref["b"][:, nc:]
        self.close(sc.group_effects[b], ge, name + " group_effects")
        if nc:
            self.close(sc.cov_effects[b], ref["b"][:, :nc], name + " cov_effects")
        else:
            assert sc.cov_effects is None

    def loglik(self, got_ll, got_s2, ref, name):
        self.close(got_ll, ref["loglik"], name + " loglik", LR.close)
        self.close(got_s2, ref["sigma2_g"], name + " sigma2_g", LR.close)

    def show(self):
        print("\nGROUP-STATS %s: worst error / max(1, max |ref|) %.3e" % (self.label, self.v))


def _same(a, b, msg=""):
    for f in FIELDS + (("cov_effects",) if a.cov_effects is not None else ()):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f + " " + msg)


@pytest.fixture(scope="module")
def eng(gpu):
    pn = GS.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


def _likelihoods(e, w, genomes, T, V, q, g, branch, refs, name):
    """log_likelihood_group at H2S as a shared grid and as a (G, B) matrix that gives every model its own order of
    them; refs(i, h2): the model's restatement at h2."""
    B = len(genomes)
    ll, s2 = e.log_likelihood_group(genomes, T, V, np.array(H2S), g, covariates=q, branch=branch, return_sigma2=True)
    assert ll.shape == (len(H2S), B) and s2.shape == ll.shape
    hm = np.array([[H2S[(gi + b) % len(H2S)] for b in range(B)] for gi in range(len(H2S))])
    lm, sm = e.log_likelihood_group(genomes, T, V, hm, g, covariates=q, branch=branch, return_sigma2=True)
    for i in range(B):
        for gi, h2 in enumerate(H2S):
            w.loglik(ll[gi, i], s2[gi, i], {k: refs(i, h2)[k][0] for k in ("loglik", "sigma2_g")}, "%s %d grid %g" % (name, i, h2))
            np.testing.assert_array_equal(lm[gi, i], ll[(gi + i) % len(H2S), i], err_msg="matrix against grid")
            np.testing.assert_array_equal(sm[gi, i], s2[(gi + i) % len(H2S), i], err_msg="matrix against grid")


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", list(GS.DESIGNS))
def test_a_auto_branch(eng, design):
    pn = GS.panel()
    genomes = [pn["genomes"][k] for k in GS.AUTO_KEYS]
    L, c = GS.DESIGNS[design]
    w = _Worst("A auto " + design)
    for s in GS.DESIGN_SPLITS[design]:
        T, V = pn["splits"][s]
        q, g = GS.design_inputs(design, s)
        batch = eng.snp_scores_group(genomes, T, V, H2, g, covariates=q)
        assert batch.score.shape == (len(genomes), 1, P) and batch.group_effects.shape == (len(genomes), 1, L)
        assert set(batch.dof) == {len(T) - 1 - (c + L - 1), len(T) - (c + L)}     # snp and gblup models: C_m differs
        for i, k in enumerate(GS.AUTO_KEYS):
            ref = GS.case_ref(design, s, k, "auto")
            w.check(batch, i, ref, "%s %s %s (batch)" % (design, s, k))
            if len(genomes[i]) <= s[0]:                   # alone: the SNP form
                w.check(eng.snp_scores_group([genomes[i]], T, V, H2, g, covariates=q), 0, ref, "%s %s %s (alone)" % (design, s, k))
        _likelihoods(eng, w, genomes, T, V, q, g, "auto",
                     lambda i, h2: GS.case_ref(design, s, GS.AUTO_KEYS[i], "auto", h2, False), "%s %s" % (design, s))
        one = [genomes[0]]                                # alone: the SNP form
        _likelihoods(eng, w, one, T, V, q, g, "auto",
                     lambda i, h2: GS.case_ref(design, s, GS.AUTO_KEYS[0], "auto", h2, False), "%s %s alone" % (design, s))
    w.show()


@pytest.mark.parametrize("design", list(GS.DESIGNS))
def test_a_forced_branches(eng, design):
    pn = GS.panel()
    w = _Worst("A forced " + design)
    for s in GS.DESIGN_SPLITS[design]:
        T, V = pn["splits"][s]
        q, g = GS.design_inputs(design, s)
        for branch, keys in (("gblup", GS.GBLUP_KEYS), ("snp", GS.snp_keys(s[0]))):
            genomes = [pn["genomes"][k] for k in keys]
            sc = eng.snp_scores_group(genomes, T, V, H2, g, branch=branch, covariates=q)
            for i, k in enumerate(keys):
                if branch == "snp":
                    assert np.all(sc.group_effects[i, :, 0] == 0.0)
                w.check(sc, i, GS.case_ref(design, s, k, branch), "%s %s %s %s" % (design, branch, s, k))
            _likelihoods(eng, w, genomes, T, V, q, g, branch,
                         lambda i, h2: GS.case_ref(design, s, keys[i], branch, h2, False), "%s %s %s" % (design, branch, s))
    w.show()


def test_a_deeper_panel_and_forms_agree(gpu):
    """n_T = 520, k = 513, 40 levels: five tile columns, one model forced through the SNP form (TBLUP_FORM=2) and the
    kernel form (TBLUP_FORM=1)."""
    dp = GS.deep_panel()
    q, g = GS.deep_inputs()
    w = _Worst("A deep / forms")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.snp_scores_group([dp["genome"]], dp["train"], dp["valid"], H2, g, covariates=q)
            w.check(got[form], 0, GS.deep_ref(), "form " + form)
            ll, s2 = e.log_likelihood_group([dp["genome"]], dp["train"], dp["valid"], H2, g, covariates=q, return_sigma2=True)
            w.loglik(ll, s2, GS.deep_ref(H2, False), "form " + form)
    for f in ("score", "info", "q", "group_effects"):
        w.close(getattr(got["1"], f)[0], getattr(got["2"], f)[0], "form 1 vs 2 " + f)
    w.show()


# ---------------------------------------------------------------------------------------------
# B. LDS at its limit and the workspace path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in A.big_cases()])
def test_b_systems_of_1024_rows_and_above(gpu, name):
    bp = GS.big_panel()
    _, gk, t, v, _, br, rows, lds = next(x for x in A.big_cases() if x[0] == name)
    q, g = GS.big_inputs(t)
    ref = GS.big_ref(name)
    assert ref["b"].shape[1] > 16 and ref["dof"] > 0
    assert np.linalg.cond(ref["G"]) <= GS.COND_MAX and np.all(ref["v"] >= GS.SPAN_MIN * ref["v_plain"])
    w = _Worst("B " + name)
    got = {}
    for knob in ("1", "0"):
        with _engine(bp["geno"], bp["pheno"], {"TBLUP_SCORE_LDS": knob}) as e:
            got[knob] = e.snp_scores_group([bp[gk]], bp[t], bp[v], H2, g, bp["snps"], branch=br, covariates=q)
            if knob == "1":
                ll, s2 = e.log_likelihood_group([bp[gk]], bp[t], bp[v], H2, g, covariates=q, branch=br, return_sigma2=True)
    w.check(got["1"], 0, ref, name)
    w.loglik(ll, s2, ref, name)
    _same(got["0"], got["1"], "TBLUP_SCORE_LDS=0")
    w.show()


# ---------------------------------------------------------------------------------------------
# C. candidate lists
# ---------------------------------------------------------------------------------------------
def test_c_candidate_lists(eng):
    pn = GS.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L40c3", s)
    genomes = [pn["genomes"][k] for k in (65, 200, 400, "dup")]       # kernel form (k = 400: gblup)
    snp_form = [genomes[0], genomes[3]]
    full = {0: eng.snp_scores_group(genomes, T, V, H2, g, covariates=q),
            1: eng.snp_scores_group(snp_form, T, V, H2, g, covariates=q)}
    for m in GS.LIST_LENGTHS:
        lst = GS.cand_list(genomes[0], P, m)
        cols = S.wrap(lst, P)
        for which, batch in ((0, genomes), (1, snp_form)):
            got = eng.snp_scores_group(batch, T, V, H2, g, lst, covariates=q)
            assert got.score.shape == (len(batch), 1, m) and got.info.shape == (len(batch), m)
            np.testing.assert_array_equal(got.snps, cols)
            np.testing.assert_array_equal(got.score, full[which].score[:, :, cols], err_msg=str(m))
            np.testing.assert_array_equal(got.info, full[which].info[:, cols], err_msg=str(m))
            for f in ("q", "dof", "cov_effects", "group_effects"):
                np.testing.assert_array_equal(getattr(got, f), getattr(full[which], f), err_msg="%s %d" % (f, m))


# ---------------------------------------------------------------------------------------------
# D. the same bits
# ---------------------------------------------------------------------------------------------
def test_d_same_bits(eng):
    pn = GS.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L113c15", s)
    snp = [pn["genomes"][k] for k in (65, 129, 200)]                      # SNP form (every k <= n_T)
    mixed = snp + [pn["genomes"][400]]                                      # kernel form, 127 and 128 columns
    lst = GS.cand_list(pn["genomes"][65], P, 65)
    hs = np.array(H2S)

    def run(e, genomes, cand):
        return (e.snp_scores_group(genomes, T, V, H2, g, cand, covariates=q),
                e.log_likelihood_group(genomes, T, V, hs, g, covariates=q, return_sigma2=True))

    def same(a, b, msg):
        _same(a[0], b[0], msg)
        np.testing.assert_array_equal(a[1][0], b[1][0], err_msg="loglik " + msg)
        np.testing.assert_array_equal(a[1][1], b[1][1], err_msg="sigma2_g " + msg)

    ref = {(i, j): run(eng, b, c) for i, b in enumerate((snp, mixed)) for j, c in enumerate((None, lst))}
    for i, b in enumerate((snp, mixed)):
        same(run(eng, b, lst), ref[i, 1], "twice")
    for env in ({"TBLUP_SCORE_LDS": "0"}, {"TBLUP_SCORE_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}, {"TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for i, b in enumerate((snp, mixed)):
                for j, c in enumerate((None, lst)):
                    same(run(e, b, c), ref[i, j], str(env))
    # a model alone against inside a batch of the same form
    one = run(eng, [snp[1]], lst)
    for f in ("score", "info", "q", "cov_effects", "group_effects"):
        np.testing.assert_array_equal(getattr(one[0], f)[0], getattr(ref[0, 1][0], f)[1], err_msg="alone " + f)
    np.testing.assert_array_equal(one[1][0][:, 0], ref[0, 1][1][0][:, 1])
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": "1"}) as e:
        one = run(e, [mixed[2]], lst)
        for f in ("score", "info", "q", "cov_effects", "group_effects"):
            np.testing.assert_array_equal(getattr(one[0], f)[0], getattr(ref[1, 1][0], f)[2], err_msg="alone, kernel form " + f)
        np.testing.assert_array_equal(one[1][0][:, 0], ref[1, 1][1][0][:, 2])


# ---------------------------------------------------------------------------------------------
# E. traits
# ---------------------------------------------------------------------------------------------
def test_e_four_traits(gpu):
    pn = GS.panel()
    s = (129, 64)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L18", s)
    batches = [[pn["genomes"][k] for k in (64, 127)],                # SNP form
               [pn["genomes"][k] for k in (200, 400)]]               # kernel form (k = 400: gblup)
    lst = GS.cand_list(pn["genomes"][64], P, 33)
    w = _Worst("E traits")
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, 0])) as e:
        single = [e.snp_scores_group(b, T, V, H2, g, lst, covariates=q) for b in batches]
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :4])) as e:
        for i, b in enumerate(batches):
            got = e.snp_scores_group(b, T, V, H2, g, lst, covariates=q)
            assert got.score.shape == (len(b), 4, len(lst)) and got.q.shape == (len(b), 4)
            assert got.group_effects.shape == (len(b), 4, 18) and got.cov_effects is None
            np.testing.assert_array_equal(got.info, single[i].info)          # info does not see the phenotypes
            ll, s2 = e.log_likelihood_group(b, T, V, H2, g, covariates=q, return_sigma2=True)
            assert ll.shape == (len(b), 4)
            for m, genome in enumerate(b):
                ref = GS.adj_ref(genome, T, pn["geno"], pn["Y"][:, :4], q, g, H2, snps=lst)
                w.check(got, m, ref, "4 traits %d %d" % (i, m))
                w.loglik(ll[m], s2[m], ref, "4 traits %d %d" % (i, m))
                w.close(got.score[m, 0], single[i].score[m, 0], "trait 0 against the single-trait run")
    w.show()


# ---------------------------------------------------------------------------------------------
# F. against the other entries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["L18", "L113c15"])
def test_f_effects_are_fit_groups_bit_for_bit(eng, design):
    pn = GS.panel()
    s = GS.DESIGN_SPLITS[design][-1]
    T, V = pn["splits"][s]
    q, g = GS.design_inputs(design, s)
    for genomes in ([pn["genomes"][k] for k in (64, 127)], [pn["genomes"][k] for k in GS.AUTO_KEYS]):
        sc = eng.snp_scores_group(genomes, T, V, H2, g, [1, 2, 3], covariates=q)
        models = eng.fit(genomes, T, V, H2, covariates=q, groups=g)
        np.testing.assert_array_equal(sc.group_effects, np.stack([m.group_effects for m in models]))
        np.testing.assert_array_equal(sc.group_levels, models[0].group_levels)
        if q is not None:
            np.testing.assert_array_equal(sc.cov_effects, np.stack([m.cov_effects for m in models]))


@pytest.mark.parametrize("branch", ["snp", "gblup", "auto"])
def test_f_narrow_design_is_the_covariate_entries_bit_for_bit(eng, branch):
    """5 levels + 3 covariates: 7 columns under snp, 8 under gblup -- the covariate entries' own kernels on [Q, Z];
    auto: a ragged batch whose models go both ways."""
    pn = GS.panel()
    T, V = pn["splits"][129, 64]
    q, g = C.make_cov(N, 3), GS.make_groups(N, 5, T)
    genomes = [pn["genomes"][k] for k in (64, 127, 200, 400)]
    lst = GS.cand_list(genomes[0], P, 33)
    sc = eng.snp_scores_group(genomes, T, V, H2, g, lst, branch=branch, covariates=q)
    ll, s2 = eng.log_likelihood_group(genomes, T, V, np.array(H2S), g, covariates=q, branch=branch, return_sigma2=True)
    # the models of a branch run as one batch of the covariate entry (a batch has one form)
    for br in ("snp", "gblup"):
        at = [i for i, genome in enumerate(genomes) if GS.fitted_branch(genome, pn["geno"], branch) == br]
        if not at:
            continue
        sub = [genomes[i] for i in at]
        X, _ = G.expand(q, g, T, br)
        sx = eng.snp_scores(sub, T, V, H2, lst, branch=br, covariates=X)
        for f in ("score", "info", "q", "dof"):
            np.testing.assert_array_equal(getattr(sc, f)[at], getattr(sx, f), err_msg=f)
        lo = 1 if br == "snp" else 0
        np.testing.assert_array_equal(sc.cov_effects[at], sx.cov_effects[:, :, :3])
        np.testing.assert_array_equal(sc.group_effects[at][:, :, lo:], sx.cov_effects[:, :, 3:])
        if lo:
            assert np.all(sc.group_effects[at][:, :, 0] == 0.0)
        lx, s2x = eng.log_likelihood_cov(sub, T, V, np.array(H2S), X, branch=br, return_sigma2=True)
        np.testing.assert_array_equal(ll[:, at], lx)
        np.testing.assert_array_equal(s2[:, at], s2x)


def test_f_q_over_dof_is_the_likelihoods_sigma2(eng):
    pn = GS.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L40c3", s)
    w = _Worst("F sigma2_g")
    for genomes in ([pn["genomes"][k] for k in (64, 127, 200)], [pn["genomes"][k] for k in GS.AUTO_KEYS]):
        sc = eng.snp_scores_group(genomes, T, V, H2, g, [0, 1], covariates=q)
        _, s2 = eng.log_likelihood_group(genomes, T, V, H2, g, covariates=q, return_sigma2=True)
        w.close(sc.q[:, 0] / sc.dof, s2, "q / dof", LR.close)
    w.show()


def test_f_effect_is_the_gls_effect_of_the_appended_snp(eng):
    """u_P / v_P of SNP j = the last covariate effect of fit(covariates=[Q, x_j], groups=), in both forms and both
    branches (the levels span the mean, so the appended column's centre is immaterial under gblup too)."""
    pn = GS.panel()
    s = (257, 70)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L40c3", s)
    w = _Worst("F effect against fit(covariates=[Q, x_j], groups=)")
    cols = S.wrap(GS.cand_list(pn["genomes"][65], P, 3), P)
    for genomes in ([pn["genomes"][k] for k in (65, 200)], [pn["genomes"][k] for k in (65, 400)]):   # SNP / kernel form
        eff = eng.snp_scores_group(genomes, T, V, H2, g, cols, covariates=q).effect()
        for j, col in enumerate(cols):
            q1 = np.ascontiguousarray(np.hstack([q, pn["geno"][:, [col]].astype(np.float64)]))
            models = eng.fit(genomes, T, V, H2, covariates=q1, groups=g)
            w.close(eff[:, 0, j], np.array([m.cov_effects[0, -1] for m in models]), "SNP %d" % col)
    w.show()


def test_f_string_labels_and_another_reference_level(eng):
    pn = GS.panel()
    s = (129, 64)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L18", s)
    genomes = [pn["genomes"][k] for k in (64, 200, 400)]
    lst = GS.cand_list(genomes[0], P, 17)
    hs = np.array(H2S)
    a = eng.snp_scores_group(genomes, T, V, H2, g, lst)
    la = eng.log_likelihood_group(genomes, T, V, hs, g)
    named = np.array(["herd%03d" % x for x in g])
    b = eng.snp_scores_group(genomes, T, V, H2, named, lst)
    for f in ("score", "info", "q", "dof", "group_effects"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert b.group_levels.dtype.kind == "U" and b.group_levels[3] == "herd003"
    np.testing.assert_array_equal(la, eng.log_likelihood_group(genomes, T, V, hs, named))
    # permuted codes: another level is the lowest, so the reference under snp
    w = _Worst("F reference level")
    perm = (7 * np.arange(18) + 5) % 18
    c = eng.snp_scores_group(genomes, T, V, H2, perm[g], lst)
    for f in ("score", "info", "q"):
        w.close(getattr(c, f), getattr(a, f), f)
    w.close(eng.log_likelihood_group(genomes, T, V, hs, perm[g]), la, "loglik", LR.close)
    w.show()


# ---------------------------------------------------------------------------------------------
# G. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def _all_nan(sc, ll, b):
    return (np.all(np.isnan(sc.score[b])) and np.all(np.isnan(sc.info[b])) and np.all(np.isnan(sc.q[b]))
            and np.all(np.isnan(ll[..., b])))


def test_g_collinear_designs_give_nan(eng):
    pn = GS.panel()
    s = (129, 64)
    T, V = pn["splits"][s]
    _, g = GS.design_inputs("L18", s)
    genomes = [pn["genomes"][k] for k in (64, 200, 400)]             # snp, snp, gblup: kernel form
    # a covariate equal to a level's indicator: collinear under both branches
    ind = np.ascontiguousarray(np.stack([C.make_cov(N, 1)[:, 0], (g == 3).astype(np.float64)], axis=1))
    for batch in (genomes, genomes[:1]):                             # kernel form, SNP form
        sc = eng.snp_scores_group(batch, T, V, H2, g, [3, 4, 5], covariates=ind)
        ll = eng.log_likelihood_group(batch, T, V, np.array(H2S), g, covariates=ind)
        for b in range(len(batch)):
            assert _all_nan(sc, ll, b) and np.all(np.isnan(sc.group_effects[b])) and np.all(np.isnan(sc.cov_effects[b]))
    # a column of ones beside the levels: collinear under gblup, vanishing (so collinear) under snp as well; beside
    # it a plain covariate harms nobody
    ones = np.ascontiguousarray(np.stack([C.make_cov(N, 1)[:, 0], np.ones(N)], axis=1))
    sc = eng.snp_scores_group(genomes, T, V, H2, g, [3, 4, 5], covariates=ones)
    ll = eng.log_likelihood_group(genomes, T, V, np.array(H2S), g, covariates=ones)
    assert all(_all_nan(sc, ll, b) for b in range(3))
    ok = eng.snp_scores_group(genomes, T, V, H2, g, [3, 4, 5], covariates=ones[:, :1])
    assert np.all(np.isfinite(ok.score)) and np.all(np.isfinite(ok.group_effects))


def test_g_no_degrees_of_freedom_is_nan_not_an_error(eng):
    """113 levels + 15 covariates on 127 train animals: dof = -1 under snp, G singular under gblup."""
    pn = GS.panel()
    s = (127, 5)
    T, V = pn["splits"][s]
    q, g = C.make_cov(N, 15), GS.make_groups(N, 113, T)
    genomes = [pn["genomes"][k] for k in (64, 200, 400)]
    for batch, branch in ((genomes, "auto"), (genomes[:1], "auto"), (genomes[:2], "gblup")):
        sc = eng.snp_scores_group(batch, T, V, H2, g, [3, 4, 5], branch=branch, covariates=q)
        ll, s2 = eng.log_likelihood_group(batch, T, V, np.array(H2S), g, covariates=q, branch=branch, return_sigma2=True)
        assert all(_all_nan(sc, ll, b) for b in range(len(batch))) and np.all(np.isnan(s2))
        assert np.all(sc.dof <= 0)


def test_g_snp_in_the_span_and_monomorphic_snp_give_exact_zeros(gpu):
    pn = GS.panel()
    geno = pn["geno"].copy()
    s = (257, 70)
    T, V = pn["splits"][s]
    geno[T, 9] = 0                                   # constant over the train rows
    q, g = GS.design_inputs("L40c3", s)
    q = q.copy()
    q[:, 2] = geno[:, 11]                            # covariate 2 is SNP 11
    with _engine(geno, pn["pheno"]) as e:
        for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][400]]):     # SNP form, kernel form
            sc = e.snp_scores_group(genomes, T, V, H2, g, [5, 11, 9, 11 - P], covariates=q)
            for j in (1, 2, 3):
                assert np.all(sc.score[:, :, j] == 0) and np.all(sc.info[:, j] == 0), j
            assert np.all(sc.info[:, 0] > 0) and np.all(np.isfinite(sc.q))
            chi = sc.chi2()
            assert np.all(np.isnan(chi[:, :, 1:])) and np.all(np.isfinite(chi[:, :, 0]))
            ref = GS.adj_ref(genomes[0], T, geno, pn["pheno"], q, g, H2, snps=[5, 11, 9, 11 - P])
            _Worst("G zeros").check(sc, 0, ref, "beside the zeros")


def test_g_monomorphic_model_panel_gives_nan(gpu):
    pn = GS.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    s = (129, 64)
    T, V = pn["splits"][s]
    q, g = GS.design_inputs("L18", s)
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            sc = e.snp_scores_group(genomes, T, V, H2, g, [3, 4], branch=br, covariates=q)
            ll = e.log_likelihood_group(genomes, T, V, np.array(H2S), g, covariates=q, branch=br)
            assert _all_nan(sc, ll, 0) and _all_nan(sc, ll, 1)
            _Worst("G").check(sc, 2, GS.adj_ref(genomes[2], T, geno, pn["pheno"], q, g, H2, br, snps=[3, 4]), br)


def test_g_errors_and_empty_calls(eng):
    from tblup_amd._native import TblupError, TblupIndexError
    from tblup_amd.engine import concat_genomes
    pn = GS.panel()
    T, V = pn["splits"][129, 64]
    gen = [pn["genomes"][64]]
    g = GS.make_groups(N, 18, T)
    calls = (lambda **kw: eng.snp_scores_group(gen, T, V, H2, snps=[1, 2], **kw),
             lambda **kw: eng.log_likelihood_group(gen, T, V, H2, **kw),
             lambda **kw: eng.estimate_h2_group(gen, T, V, refine=0, **kw))
    for call in calls:
        for wrong in (g[:-1], g.astype(np.float64), np.stack([g, g], axis=1)):
            with pytest.raises(ValueError):
                call(groups=wrong)
        unseen = g.copy()
        unseen[V[3]] = 99
        with pytest.raises(ValueError, match="99"):
            call(groups=unseen)
    # 129 columns: 113 levels + 16 covariates under gblup (128 under snp run)
    T2, V2 = pn["splits"][257, 70]
    g113, q16 = GS.make_groups(N, 113, T2), C.make_cov(N, 16)
    with pytest.raises(ValueError, match="129"):
        eng.snp_scores_group(gen, T2, V2, H2, g113, [1], branch="gblup", covariates=q16)
    with pytest.raises(ValueError, match="129"):
        eng.log_likelihood_group(gen, T2, V2, H2, g113, covariates=q16, branch="gblup")
    assert np.all(np.isfinite(eng.snp_scores_group(gen, T2, V2, H2, g113, [1], branch="snp", covariates=q16).score))
    with pytest.raises(TblupError):
        eng.snp_scores_group(gen, T, V, 1.0, g)
    with pytest.raises(TblupError):
        eng.log_likelihood_group(gen, T, V, [0.3, 1.0], g)
    with pytest.raises(TblupIndexError):
        eng.snp_scores_group(gen, T, V, H2, g, [0, P])
    # the existing entries keep refusing, and name the new method
    with pytest.raises(ValueError, match="snp_scores_group"):
        eng.snp_scores(gen, T, V, H2, [1], groups=g)
    with pytest.raises(ValueError, match="groups"):
        eng.reliability_cov(gen, T, V, H2, [1], C.make_cov(N, 2), groups=g)
    # an empty batch and an empty list run nothing
    empty = eng.snp_scores_group(gen * 3, T, V, H2, g, [])
    assert empty.score.shape == (3, 1, 0) and empty.group_effects.shape == (3, 1, 18) and np.all(np.isnan(empty.q))
    none = eng.snp_scores_group([], T, V, H2, g, [1, 2])
    assert none.score.shape == (0, 1, 2) and none.dof.shape == (0,)
    assert eng.log_likelihood_group([], T, V, np.array(H2S), g).shape == (len(H2S), 0)
    # the entries' own argument checks
    lib, sid = eng._lib, eng.split_id(T, V)
    idx, off = concat_genomes(gen)
    lst = np.array([1, 2], dtype=np.int64)
    u, v, ll = np.empty((1, 1, 2)), np.empty((1, 2)), np.empty((1, 1, 1))
    h = np.array([H2])

    def score(codes, L, cov=None, nc=0):
        return lib.tblup_snp_score_group_batch(
            eng._ctx, sid, None if cov is None else cov.ctypes.data_as(F64), nc, codes.ctypes.data_as(I64), L,
            lst.ctypes.data_as(I64), 2, idx.ctypes.data_as(I64), off.ctypes.data_as(I64), 1, H2, 0, None,
            u.ctypes.data_as(F64), v.ctypes.data_as(F64), None, None, None)

    def loglik(codes, L, cov=None, nc=0):
        return lib.tblup_loglik_group_batch(
            eng._ctx, sid, None if cov is None else cov.ctypes.data_as(F64), nc, codes.ctypes.data_as(I64), L,
            idx.ctypes.data_as(I64), off.ctypes.data_as(I64), 1, h.ctypes.data_as(F64), 1, 0, None,
            ll.ctypes.data_as(F64), None, None, None)
    codes = np.ascontiguousarray(g, dtype=np.int64)
    off_split = np.setdiff1d(np.arange(N), np.concatenate([T, V]))
    for call in (score, loglik):
        assert call(codes, 18) == 0
        assert call(codes, 17) != 0 and b"level code" in lib.tblup_last_error()            # a code >= n_levels
        bad = codes.copy()
        bad[T[5]] = -1
        assert call(bad, 18) != 0 and b"no level" in lib.tblup_last_error()                # -1 on a train row
        bad = codes.copy()
        bad[off_split[:3]] = -1                                                              # -1 outside the split: fine
        assert call(bad, 18) == 0
        assert call(codes, 19) != 0 and b"no train row" in lib.tblup_last_error()          # a level without a train row
        assert call(codes, 18, np.zeros((N, 17)), 17) != 0 and b"n_cov" in lib.tblup_last_error()
        nanq = C.make_cov(N, 2)
        nanq[7, 1] = np.nan
        assert call(codes, 18, nanq, 2) != 0 and b"finite" in lib.tblup_last_error()
        assert call(codes, 0) != 0


# ---------------------------------------------------------------------------------------------
# H. estimate_h2_group and the evaluator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["snp", "gblup"])
def test_h_estimate_h2_group(gpu, branch):
    e = GS.est_inputs()
    ref = GS.estimate_ref(e["genome"], e["T"], e["geno"], e["pheno"], e["cov"], e["groups"], branch)
    with _engine(e["geno"], e["pheno"]) as en:
        got = en.estimate_h2_group([e["genome"]], e["T"], e["V"], e["groups"], covariates=e["cov"], branch=branch)
    print("\nGROUP-STATS H %s: h2 %.6f (ref %.6f), loglik error %.3e" % (
        branch, got["h2"][0], ref["h2"], abs(got["loglik"][0] - ref["loglik"]) / max(1.0, abs(ref["loglik"]))))
    assert got["h2"][0] == ref["h2"] and got["step"][0] == ref["step"] and bool(got["at_bound"][0]) == ref["at_bound"]
    assert abs(got["loglik"][0] - ref["loglik"]) <= TOL * max(1.0, abs(ref["loglik"]))
    assert abs(got["sigma2_g"][0] - ref["sigma2_g"]) <= TOL * max(1.0, abs(ref["sigma2_g"]))


@pytest.fixture
def global_rngs_kept():
    """The evaluator draws its split from python's and numpy's global generators; tests that run later in the same
    process (tests/test_gpu_loglik_cov.py::test_g_evaluator compares bits across two orders of a genome on such a
    split) must find them as they would without this file."""
    import random
    py, npy = random.getstate(), np.random.get_state()
    yield
    random.setstate(py)
    np.random.set_state(npy)


def test_h_evaluator_methods(gpu, tmp_path, global_rngs_kept):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = GS.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, H2, False)
    rem.removed = np.array((5, 17, 301, 599), dtype=np.float64)
    q = C.make_cov(N, 3)
    w = _Worst("H")
    with E.BlupParallelEvaluator(gp, pp, H2, snp_remover=rem) as ev:
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        g = GS.make_groups(N, 30, train)
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 129, 200)]
        lst = GS.cand_list(pop[1].genome, P, 33)
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        sc = ev.snp_scores_group(pop, g, lst, covariates=q)
        _same(sc, ev.engine.snp_scores_group(genomes, train, ev.testing_indices, H2, g, lst, covariates=q))
        for i, genome in enumerate(genomes):
            w.check(sc, i, GS.adj_ref(genome, train, pn["geno"], pn["pheno"], q, g, H2, snps=lst), "model %d" % i)
        hs = np.array(H2S)
        np.testing.assert_array_equal(ev.log_likelihood_group(pop, hs, g, covariates=q),
                                      ev.engine.log_likelihood_group(genomes, train, ev.testing_indices, hs, g, covariates=q))
        a = ev.estimate_h2_group(pop, g, covariates=q, refine=1, points=5)
        b = ev.engine.estimate_h2_group(genomes, train, ev.testing_indices, g, covariates=q, refine=1, points=5)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        # the entries that do not take the class factor still say so
        for call in (lambda: ev.snp_scores(pop, lst, groups=g), lambda: ev.log_likelihood(pop, H2, groups=g),
                     lambda: ev.estimate_h2(pop, groups=g)):
            with pytest.raises(ValueError, match="groups"):
                call()
    w.show()
