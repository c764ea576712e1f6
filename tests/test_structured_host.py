"""The structured panel of tests/structured_ref.py is what it says, its systems are as ill-conditioned as the GPU
tests need, and the bar of tests/test_gpu_structured.py is fair: on every case and quantity that the GPU tests check,
the float64 restatement (LAPACK, or the restatements' own column Cholesky) is within
max(TOL / 8, 2 kappa 2^-53) of the longdouble truth, an eighth of what the GPU path is allowed.  The worst
err / (kappa 2^-53) of each quantity is printed (pytest -s).

The same for the fixed-effect designs of tests/test_gpu_structured_fixed.py: the input conditions (level counts, no
unseen label, cond(G) <= STRUCT_COND_MAX, v_P >= SPAN_MIN v, bar / gap <= LOO_GAP_MAX), one restatement test per
truth (adjusted statistics, adjusted uncertainty, fit(groups=), leave-one-out in both forms -- pred, eloo, PRESS and
the fitness held to host_bar / gap, the LOO rule of tests/structured_ref.py), and the two further left-out inputs: (d)
under gblup with the class factor, and LOO pred / eloo without the 1 / gap factor.
"""
import numpy as np

from oracle import blup_oracle as O
from tests import covar_ref as CV
from tests import group_ref as GR
from tests import group_stats_ref as GS
from tests import loglik_ref as LL
from tests import loo_ref as LO
from tests import model_ref as R
from tests import reliab_cov_ref as RC
from tests import reliab_group_ref as RG
from tests import reliability_ref as Q
from tests import score_cov_ref as SC
from tests import score_ref as S
from tests import structured_ref as SR

LD = np.longdouble


# ---------------------------------------------------------------------------------------------
# The panel
# ---------------------------------------------------------------------------------------------
def test_panel_shape_and_splits():
    pn = SR.panel()
    g = pn["geno"]
    assert g.shape == (301, 640) and g.dtype == np.int8 and g.min() == 0 and g.max() == 2 and g.shape[0] % 2 == 1
    special = set(sum(pn["clones"].values(), ())) | set(pn["carriers"])
    for s in SR.SPLITS:
        T, V = pn["splits"][s]
        assert (len(T), len(V)) == s and len(set(T)) == len(T) and len(set(V)) == len(V) and not set(T) & set(V)
        assert special <= set(T)
    T200, T257 = pn["splits"][200, 60][0], pn["splits"][257, 40][0]
    np.testing.assert_array_equal(T257[:200], T200)
    Tcf = pn["splits"]["cf"][0]
    assert len(Tcf) == 196 and len(np.unique(g[Tcf], axis=0)) == 196


def test_ld_blocks():
    pn = SR.panel()
    g = pn["geno"].astype(np.float64)
    edited = set(pn["rare"]) | set(pn["dup"]) | set(pn["comp"])
    r = [abs(np.corrcoef(g[:, j], g[:, j + 1])[0, 1]) for j in range(SR.N_SNPS - 1)
         if (j + 1) % SR.BLOCK and j not in edited and j + 1 not in edited]
    across = [abs(np.corrcoef(g[:, j], g[:, j + 1])[0, 1]) for j in range(SR.BLOCK - 1, SR.N_SNPS - 1, SR.BLOCK)]
    print("median |r| of adjacent SNPs: %.3f within blocks, %.3f across block boundaries" % (np.median(r), np.median(across)))
    assert np.median(r) >= 0.5
    assert np.median(across) < 0.5


def test_families_inherit_whole_blocks():
    """Within a family a block has at most 4 parental haplotype pairs (plus rare new flips): the 10 sibs show few
    distinct block genotypes, unrelated animals many."""
    pn = SR.panel()
    g = pn["geno"]
    cols = np.setdiff1d(np.arange(SR.N_SNPS), np.concatenate([pn["rare"], pn["dup"], pn["comp"]]))
    blocks = [b for b in range(SR.N_SNPS // SR.BLOCK) if set(range(b * 16, b * 16 + 16)) <= set(cols)]
    assert len(blocks) >= 25

    def distinct(rows):
        return np.mean([len(np.unique(g[np.ix_(rows, np.arange(b * 16, b * 16 + 16))], axis=0)) for b in blocks])

    fam = [distinct(np.flatnonzero(pn["family"] == f)) for f in range(SR.N_FAM)]
    rnd = distinct(np.arange(0, 290, 29))                       # ten animals of ten families
    print("distinct block genotypes among 10 animals: sibs %.2f, across families %.2f" % (np.mean(fam), rnd))
    assert all(np.bincount(pn["family"][pn["family"] >= 0]) == SR.FAM)
    assert max(fam) <= 6.0 and rnd >= 7.0


def test_clones_sit_where_the_factor_is_sensitive():
    pn = SR.panel()
    g = pn["geno"]
    for s in SR.SPLITS:
        T = pn["splits"][s][0]
        i, j = SR.PAIR_ROWS
        assert i // 16 == j // 16 and j == i + 1 and np.array_equal(g[T[i]], g[T[j]])
        i, j = SR.STRADDLE_ROWS
        assert i // 128 != j // 128 and np.array_equal(g[T[i]], g[T[j]])
        a, b, c = SR.TRIPLE_ROWS
        assert np.array_equal(g[T[a]], g[T[b]]) and np.array_equal(g[T[a]], g[T[c]])
        assert len(np.unique(g[T], axis=0)) == len(T) - 4       # no other repeated row
    assert tuple(pn["splits"][200, 60][0][list(SR.PAIR_ROWS)]) == pn["clones"]["pair"]
    # the clones have sibs among the validation animals, and there are unrelated validation animals
    V = pn["splits"][257, 40][1]
    assert set(pn["sibs"]) <= set(V) and len(set(pn["unrelated"]) & set(V)) >= 3
    assert set(pn["family"][pn["sibs"]]) == {0, 1, 2}


def test_rare_and_repeated_columns():
    pn = SR.panel()
    g = pn["geno"]
    assert len(pn["rare"]) == 20 and len(set(pn["carriers"])) == 20
    for c, a in zip(pn["rare"], pn["carriers"]):
        assert g[:, c].sum() == 1 and g[a, c] == 1
    np.testing.assert_array_equal(g[:, pn["dup"][1]], g[:, pn["dup"][0]])
    np.testing.assert_array_equal(g[:, pn["comp"][1]], 2 - g[:, pn["comp"][0]])
    assert g[:, pn["dup"][0]].std() > 0 and g[:, pn["comp"][0]].std() > 0
    g160 = pn["genomes"]["snp160"]
    assert set(pn["rare"]) | set(pn["dup"]) | set(pn["comp"]) <= set(g160)
    assert tuple(g160[[4, 5]]) == pn["dup"] and tuple(g160[[127, 128]]) == pn["comp"]
    whole = [b for b in range(40) if set(range(16 * b, 16 * b + 16)) <= set(g160)]
    assert len(whole) == 9
    # candidates of the score test: the duplicate of a model SNP, a rare column, an outside SNP of a model LD block
    cand = S.wrap(SR.cand_snps(), SR.N_SNPS)
    assert pn["dup"][1] in cand and set(cand) & set(pn["rare"])
    out = [c for c in cand if c not in g160 and set(range(c // 16 * 16, c // 16 * 16 + 16)) & set(g160)]
    assert len(out) >= 2
    # nothing but the two pairs is repeated or complemented in the SNP-form genome on the train rows
    x = g[np.ix_(pn["splits"][200, 60][0], pn["genomes"]["snp158"])]
    both = np.concatenate([x, 2 - x], axis=1)
    assert len(np.unique(both, axis=1).T) == 2 * 158


def test_genomes_and_phenotypes():
    pn = SR.panel()
    k = {key: len(v) for key, v in pn["genomes"].items()}
    assert k == {"snp160": 160, "snp158": 158, "dual260": 260, "g400": 400, "g130": 130}
    assert all(len(set(v)) == len(v) for v in pn["genomes"].values())
    assert all(200 < k["dual260"] <= SR.N_ANIMALS and s[0] < k["dual260"] for s in SR.SPLITS) and k["g400"] > SR.N_ANIMALS
    assert set(pn["genomes"]["snp160"]) <= set(pn["genomes"]["dual260"])
    Y = pn["Y"]
    i, j = pn["clones"]["pair"]
    e = np.zeros(SR.N_ANIMALS)
    e[i], e[j] = 1.0, -1.0
    np.testing.assert_array_equal(Y[:, 1], e)
    np.testing.assert_array_equal(Y[:, 3], Y[:, 0] + 1e6)
    np.testing.assert_array_equal(Y[:, 4], Y[:, 0] + Y[:, 1])
    assert abs(Y[:, 0].std() - 1) < 0.15
    r2 = np.corrcoef(Y[:, 2], pn["bv"])[0, 1] ** 2                 # (c): a breeding value and as much noise
    assert 0.35 < r2 < 0.65 and abs(pn["bv"].std() - 1) < 1e-12


# ---------------------------------------------------------------------------------------------
# Conditioning
# ---------------------------------------------------------------------------------------------
def test_condition_numbers():
    """kappa at h2 = 0.999999 is >= 1e7 in every solve path (SNP form, gblup, snp-dual) of both splits, about 20 at
    h2 = 0.4; the 16 x 16 diagonal block of the in-block clone pair, which the explicit inverse of the diagonal
    blocks sees, is >= 1e5."""
    for s in SR.SPLITS:
        for g, br, form in (("snp160", "snp", "snp"), ("snp160", "snp", "kernel"), ("g400", "gblup", "kernel"),
                            ("dual260", "snp", "kernel"), ("g130", "gblup", "kernel")):
            ks = [SR.kappa(s, g, br, h, form) for h in SR.H2S]
            print("kappa %s %-8s %-5s %-6s: %s" % (s, g, br, form, " ".join("%.2e" % k for k in ks)))
            assert ks[0] < 100 and ks[-1] >= 1e7 and all(a < b for a, b in zip(ks, ks[1:]))
        for g, br in (("g400", "gblup"), ("snp160", "snp")):
            kb = SR.block_kappa(s, g, br, 0.999999, 0, 16)
            print("kappa of the diagonal block [0:16) %s %s: %.2e" % (s, g, kb))
            assert kb >= 1e5
            assert SR.block_kappa(s, g, br, 0.999999, 16, 32) < kb / 100       # it is the clones' doing


def test_kappa_is_the_condition_of_the_solved_matrix():
    A = SR._system((200, 60), "g400", "gblup", 0.9999, "kernel")
    assert abs(np.linalg.cond(A) / SR.kappa((200, 60), "g400", "gblup", 0.9999, "kernel") - 1) < 1e-6
    A = SR._system((200, 60), "snp160", "snp", 0.99, "snp")
    assert abs(np.linalg.cond(A) / SR.kappa((200, 60), "snp160", "snp", 0.99, "snp") - 1) < 1e-6
    assert SR.form_of(["snp160"], (200, 60), "auto") == "snp" and SR.form_of(SR.GENOMES, (200, 60), "auto") == "kernel"
    assert SR.form_of(["dual260"], (200, 60), "auto") == "kernel" and SR.form_of(["dual260"], (257, 40), "auto") == "snp"
    assert SR.form_of(["g130"], (200, 60), "gblup") == "kernel"


# ---------------------------------------------------------------------------------------------
# The float64 restatements against the longdouble truth
# ---------------------------------------------------------------------------------------------
class _Ratios:
    """Every error is asserted against host_bar; the worst err / (kappa u) per quantity is kept twice: over every
    comparison (at small kappa the flat TOL / 8 rules and the ratio means little) and over those with kappa >= 3e3."""
    ILL = 3e3

    def __init__(self):
        self.worst, self.ill, self.n = {}, {}, 0

    def check(self, quantity, err, kappa, name, tol=SR.TOL):
        self.n += 1
        ratio = err / (kappa * SR.U)
        for tab in (self.worst,) + ((self.ill,) if kappa >= self.ILL else ()):
            if ratio >= tab.get(quantity, (0.0,))[0]:
                tab[quantity] = (ratio, err, kappa, name)
        assert err <= SR.host_bar(kappa, tol), (quantity, name, err, kappa, ratio)

    def show(self, label):
        print("\nSTRUCTURED host %s, %d comparisons; worst err / (kappa u), all | kappa >= %g:" % (label, self.n, self.ILL))
        for q, (ratio, err, kappa, name) in sorted(self.worst.items()):
            ill = self.ill.get(q)
            print("  %-12s %7.3f (err %.2e, kappa %.2e, %s) | %s" % (
                q, ratio, err, kappa, name, "-" if ill is None else "%.3f (err %.2e, kappa %.2e, %s)" % ill))
            assert ill is None or ill[0] <= 2.0, (q, ill)


def _fit_host(w, split, gkey, br, h2, form=None):
    pn = SR.panel()
    idx, (T, V) = pn["genomes"][gkey], pn["splits"][split]
    g64 = pn["geno"].astype(np.float64)
    truth = SR.fit_truth(split, gkey, br, h2)
    assert truth is not None
    kap = SR.kappa(split, gkey, br, h2, form or SR.own_form(split, gkey, br))
    fn = O.gblup if br == "gblup" else O.snp_blup
    for t in SR.fit_cols(br, gkey):
        name = "%s %s %s h2=%s (%s)" % (split, gkey, br, h2, SR.COLS[t])
        y = np.ascontiguousarray(pn["Y"][:, t])
        m = R.fit_ref(idx, T, pn["geno"], y, h2, br)
        w.check("effects", SR.relerr(m["effects"], truth["effects"][t]), kap, name)
        if br == "snp":
            w.check("intercept", SR.relerr([m["intercept"]], [truth["intercept"][t]]), kap, name)
        ebv_all = (g64[:, idx] - m["center"]) @ m["effects"] + m["intercept"]
        w.check("ebv (model)", SR.relerr(ebv_all, truth["ebv"][t]), kap, name)
        f, e = fn(idx, T, V, g64, y, h2, return_ebv=True)
        w.check("ebv (oracle)", SR.relerr(e, truth["ebv"][t][V]), kap, name)
        if t in SR.FITNESS_COLS:
            w.check("fitness", abs(f - truth["fitness"][t]), kap, name)


def test_fit_and_evaluate_restatements():
    w = _Ratios()
    for case in SR.FIT_CASES:
        _fit_host(w, *case)
    w.show("fit / evaluate")


def test_truth_is_blup_wide_too():
    """fit_truth's EBVs (from model_ref.fit_wide's effects) are test_edge_cases_cpu.blup_wide's."""
    pn = SR.panel()
    for split, gkey, br, h2 in (((200, 60), "snp160", "snp", 0.999999), ((257, 40), "g400", "gblup", 0.999999),
                                ((200, 60), "dual260", "snp", 0.4)):
        T, V = pn["splits"][split]
        truth = SR.fit_truth(split, gkey, br, h2)
        for t in SR.fit_cols(br):
            f, e, _ = SR.blup_wide(pn["genomes"][gkey], T, V, pn["geno"], pn["Y"][:, t], h2, br)
            assert SR.relerr(e, truth["ebv"][t][V]) < 1e-18 * SR.kappa(split, gkey, br, h2, "kernel")
            assert abs(f - truth["fitness"][t]) < 1e-12


def test_factor_restatement():
    pn = SR.panel()
    w = _Ratios()
    for split in SR.SPLITS:                      # the K block of the oracle against the exact counts: nothing solved
        for gkey, br in SR.FACTOR_MODELS:
            T, V = pn["splits"][split]
            K = O.grm_block(pn["genomes"][gkey], T, V, pn["geno"], br)
            assert SR.relerr(K, SR.k_truth(split, gkey, br)) <= 1e-12 / 8
    for split, gkey, br, h2 in SR.FACTOR_CASES:
        L, z = SR.factor_truth(split, gkey, br, h2)
        kap = SR.kappa(split, gkey, br, h2, "kernel")
        A = SR._system(split, gkey, br, h2, "kernel")
        L64 = np.linalg.cholesky(A)
        name = "%s %s %s h2=%s" % (split, gkey, br, h2)
        w.check("L", SR.relerr(L64, L), kap, name, SR.CHOL_TOL)
        y = pn["Y"][pn["splits"][split][0]]
        y = y - (y.mean(axis=0) if br == "snp" else 0.0)
        z64 = np.linalg.solve(L64, y)
        for t in SR.z_cols(br):
            w.check("z", SR.relerr(z64[:, t], z[:, t]), kap, name + " (%s)" % SR.COLS[t], SR.CHOL_TOL)
    w.show("factor")


def test_reliability_restatement():
    pn = SR.panel()
    an = SR.rel_animals()
    w = _Ratios()
    for split, gkey, br, h2 in SR.AUX_CASES:
        form = "snp" if len(pn["genomes"][gkey]) <= len(pn["splits"][split][0]) else "kernel"     # rel_ref's own
        r = Q.rel_ref(pn["genomes"][gkey], pn["splits"][split][0], pn["geno"], h2, br)
        truth = SR.rel_truth(split, gkey, br, h2)
        assert np.all(truth > -1e-15) and np.all(truth < 1 + 1e-15)
        err = float(np.max(np.abs(r.astype(LD) - truth)[an]))
        w.check("reliability", err, SR.kappa(split, gkey, br, h2, form), "%s %s %s h2=%s" % (split, gkey, br, h2))
    w.show("reliability")


def test_reliability_of_a_clone_is_nearly_one():
    """At h2 = 0.999999 the clone of a train animal is all but known; its sibs and unrelated animals are not."""
    pn = SR.panel()
    r = SR.rel_truth((200, 60), "g400", "gblup", 0.999999)
    clones = list(sum(pn["clones"].values(), ()))
    assert np.all(r[clones] > 0.999999) and np.all(r[pn["sibs"]] < 0.99)
    assert np.all(r[pn["splits"][200, 60][1][6:9]] < r[pn["sibs"]].max())


def test_loglik_restatement():
    pn = SR.panel()
    w = _Ratios()
    for split, gkey, br, h2 in SR.LL_CASES:
        ll, s2 = LL.loglik_ref(pn["genomes"][gkey], pn["splits"][split][0], pn["geno"], pn["Y"], h2, br)
        tl, ts = SR.loglik_truth(split, gkey, br, h2)
        kap = SR.kappa(split, gkey, br, h2, "kernel")
        for t in range(5):
            name = "%s %s %s h2=%s (%s)" % (split, gkey, br, h2, SR.COLS[t])
            w.check("loglik", float(abs(LD(ll[t]) - tl[t]) / max(LD(1), abs(tl[t]))), kap, name)
            w.check("sigma2_g", float(abs(LD(s2[t]) - ts[t]) / max(LD(1), abs(ts[t]))), kap, name)
    w.show("log-likelihood")


def test_score_restatement():
    pn = SR.panel()
    cand = SR.cand_snps()
    w = _Ratios()
    for split, gkey, br, h2 in SR.AUX_CASES:
        u, v, q = S.score_ref(pn["genomes"][gkey], pn["splits"][split][0], pn["geno"], pn["Y"], h2, br, cand)
        tu, tv, tq = SR.score_truth(split, gkey, br, h2)
        kap = SR.kappa(split, gkey, br, h2, SR.own_form(split, gkey, br))
        name = "%s %s %s h2=%s" % (split, gkey, br, h2)
        w.check("info v", SR.relerr(v, tv), kap, name)
        for t in range(5):
            w.check("q", SR.relerr([q[t]], [tq[t]]), kap, name + " (%s)" % SR.COLS[t])
        for t in SR.fit_cols(br):
            w.check("score u", SR.relerr(u[t], tu[t]), kap, name + " (%s)" % SR.COLS[t])
    w.show("SNP scores")


def test_covariate_restatement():
    pn = SR.panel()
    Qm = SR.covariates()
    assert Qm.shape == (SR.N_ANIMALS, 3) and set(np.flatnonzero(Qm[:, 0])) == set(np.flatnonzero(pn["family"] == 0))
    w = _Ratios()
    for split, gkey, br, h2 in SR.AUX_CASES:
        T = pn["splits"][split][0]
        g = CV.gls_ref(pn["genomes"][gkey], T, pn["geno"], pn["Y"], Qm, h2, br)
        truth = SR.gls_truth(split, gkey, br, h2)
        name = "%s %s %s h2=%s" % (split, gkey, br, h2)
        print("cond(G) %s: %.2e" % (name, truth["cond"]))
        assert truth["cond"] < CV.COND_MAX, name
        kap = SR.kappa(split, gkey, br, h2, "kernel")
        for t in SR.fit_cols(br):
            w.check("cov effects", SR.relerr(g["b"][t], truth["b"][t]), kap, name + " (%s)" % SR.COLS[t])
            m = R.fit_ref(pn["genomes"][gkey], T, pn["geno"], np.ascontiguousarray(g["ystar"][:, t]), h2, br)
            w.check("effects", SR.relerr(m["effects"], truth["effects"][t]), kap, name + " (%s)" % SR.COLS[t])
            V = pn["splits"][split][1]
            ebv = (pn["geno"][np.ix_(V, pn["genomes"][gkey])] - m["center"]) @ m["effects"] + m["intercept"]
            w.check("ebv valid", SR.relerr(ebv, truth["ebv"][t][V]), kap, name + " (%s)" % SR.COLS[t])
    w.show("covariates")


# ---------------------------------------------------------------------------------------------
# Fixed effects: the designs' conditions and the float64 restatements of the adjusted entries
# ---------------------------------------------------------------------------------------------
def test_fixed_design_input_conditions():
    """The class factor has 30 levels, each with 5-10 train rows in (200, 60) and 6-10 in (257, 40), and no validation
    animal carries a label the train rows lack; cond(G) <= STRUCT_COND_MAX in every case (fam+n passes
    covar_ref.COND_MAX in two: the family directions, where V^-1 is about 1 / eig(K), beside the normal column, where it
    is about 1 / lambda); v_P >= SPAN_MIN v for every candidate; bar / gap <= LOO_GAP_MAX for every LOO case."""
    pn = SR.panel()
    grp = SR.groups()
    assert len(np.unique(grp)) == 30
    for s, lo in (((200, 60), 5), ((257, 40), 6)):
        T, V = pn["splits"][s]
        lev, n = np.unique(grp[T], return_counts=True)
        print("levels %s: %d, train rows per level %d-%d" % (s, len(lev), n.min(), n.max()))
        assert len(lev) == 30 and n.min() == lo and n.max() == 10
        assert set(grp[V]) <= set(lev) and set(grp[SR.rel_animals()]) <= set(lev)
    Qm = SR.covariates()
    np.testing.assert_array_equal(Qm[:, 0], (grp == 0).astype(np.float64))      # why fam+n leaves it out
    worst_cond, span = {}, (np.inf, None)
    over = []
    for name in SR.DESIGNS:
        for split, gkey, br, h2 in sorted(set(SR.AUX_CASES + SR.LL_CASES), key=str):
            tr = SR.adj_truth(name, split, gkey, br, h2)
            F, _ = SR.design_matrix(name, split, gkey, br)
            assert F.shape[1] == {"cov3": 3, "fam": 30, "fam+n": 31}[name] - (name != "cov3" and br == "snp")
            label = "%s %s %s %s h2=%s" % (name, split, gkey, br, h2)
            print("cond(G) %s: %.2e" % (label, tr["cond"]))
            assert tr["cond"] <= SR.STRUCT_COND_MAX, label
            if tr["cond"] > CV.COND_MAX:
                over.append(label)
            worst_cond[name] = max(worst_cond.get(name, 0.0), tr["cond"])
            ratio = float(np.min(tr["v"] / tr["v_plain"]))
            span = min(span, (ratio, label))
            assert np.all(tr["v"] >= SR.SC.SPAN_MIN * tr["v_plain"]), label
    print("worst cond(G): %s; over covar_ref.COND_MAX: %s" % (
        ", ".join("%s %.2e" % kv for kv in worst_cond.items()), over))
    print("smallest v_P / v: %.2e (%s)" % span)
    assert all(o.startswith("fam+n") for o in over)
    worst = (0.0, None)
    for split, gkey, br, form, h2 in SR.LOO_CASES:
        tr = SR.loo_truth(split, gkey, br, h2, form)
        kap = SR.kappa(split, gkey, br, h2, form)
        r = SR.loo_bar(kap, tr["gap"])
        label = "%s %s %s %s h2=%s" % (split, gkey, br, form, h2)
        print("LOO gap %s: %.2e, bar / gap %.2e" % (label, tr["gap"], r))
        assert 0 < tr["gap"] <= 1 and r <= SR.LOO_GAP_MAX, label
        worst = max(worst, (r, label))
    print("largest bar / gap: %.2e (%s)" % worst)


def _rel1(got, truth):
    return float(abs(LD(got) - truth) / max(LD(1), abs(truth)))


def test_adjusted_statistics_restatement():
    """score_cov_ref.adj_ref / group_stats_ref.adj_ref (the same routine on the expanded design) against adj_wide:
    u_P, v_P, q_P, b, log-likelihood and sigma2_g of every design."""
    pn = SR.panel()
    cand = SR.cand_snps()
    for name in SR.DESIGNS:
        w = _Ratios()
        cov, grp = SR.design(name)
        for split, gkey, br, h2 in sorted(set(SR.AUX_CASES + SR.LL_CASES), key=str):
            idx, T = pn["genomes"][gkey], pn["splits"][split][0]
            if grp is None:
                r = SC.adj_ref(idx, T, pn["geno"], pn["Y"], cov, h2, br, cand)
            else:
                r = GS.adj_ref(idx, T, pn["geno"], pn["Y"], cov, grp, h2, br, cand)
            tr = SR.adj_truth(name, split, gkey, br, h2)
            kap = SR.kappa(split, gkey, br, h2, "kernel")
            label = "%s %s %s h2=%s" % (split, gkey, br, h2)
            for t in SR.stat_cols(name, br):
                c = label + " (%s)" % SR.COLS[t]
                w.check("q", SR.relerr([r["q"][t]], [tr["q"][t]]), kap, c)
                w.check("loglik", _rel1(r["loglik"][t], tr["loglik"][t]), kap, c)
                w.check("sigma2_g", _rel1(r["sigma2_g"][t], tr["sigma2_g"][t]), kap, c)
            if (split, gkey, br, h2) not in SR.AUX_CASES:
                continue
            w.check("info v", SR.relerr(r["v"], tr["v"]), kap, label)
            for t in SR.fit_cols(br):
                c = label + " (%s)" % SR.COLS[t]
                w.check("b", SR.relerr(r["b"][t], tr["b"][t]), kap, c)
                if t in SR.stat_cols(name, br):
                    w.check("score u", SR.relerr(r["u"][t], tr["u"][t]), kap, c)
        w.show("adjusted statistics, " + name)


def test_adjusted_uncertainty_restatement():
    """reliab_cov_ref.vform_ref / reliab_group_ref.vform_ref against vform_wide on rel_animals(): reliability
    (absolute, inside [0, 1] and never above the plain one), pev_total, cov_cov / fixed_cov."""
    pn = SR.panel()
    an = SR.rel_animals()
    for name in SR.DESIGNS:
        w = _Ratios()
        cov, grp = SR.design(name)
        for split, gkey, br, h2 in SR.AUX_CASES:
            idx, T = pn["genomes"][gkey], pn["splits"][split][0]
            if grp is None:
                r = RC.vform_ref(idx, T, pn["geno"], cov, h2, br, an)
                key = "cov_cov"
            else:
                r = RG.vform_ref(idx, T, pn["geno"], cov, grp, h2, br, an)
                key = "fixed_cov"
                assert not np.any(r["unseen"])
                if br == "snp":
                    nc = 0 if cov is None else cov.shape[1]
                    assert not np.any(r[key][nc]) and not np.any(r[key][:, nc])
            tr = SR.relfix_truth(name, split, gkey, br, h2)
            kap = SR.kappa(split, gkey, br, h2, "kernel")
            hb = SR.host_bar(kap)
            label = "%s %s %s h2=%s" % (split, gkey, br, h2)
            plain = SR.rel_truth(split, gkey, br, h2)[an]
            assert np.all(tr["rel"][an] <= plain + 1e-15) and np.all(tr["rel"][an] > -1e-15), label
            assert np.all(r["rel"] >= -hb) and np.all(r["rel"] <= plain + hb), label
            w.check("reliability", float(np.max(np.abs(r["rel"].astype(LD) - tr["rel"][an]))), kap, label)
            w.check("pev_total", SR.relerr(r["pev"], tr["pev"][an]), kap, label)
            w.check(key, SR.relerr(r[key], tr[key]), kap, label)
        w.show("adjusted uncertainty, " + name)


def test_group_fit_restatement():
    """group_ref.group_ref (the GLS of the expanded design, then the oracle's blup and fit_ref of y*) against
    fixfit_truth under the class factor: level and covariate effects, SNP effects, validation EBVs, fitness."""
    pn = SR.panel()
    for name in ("fam", "fam+n"):
        w = _Ratios()
        cov, grp = SR.design(name)
        for split, gkey, br, h2 in SR.AUX_CASES:
            idx, (T, V) = pn["genomes"][gkey], pn["splits"][split]
            tr = SR.fixfit_truth(name, split, gkey, br, h2)
            assert tr["cond"] <= SR.STRUCT_COND_MAX
            kap = SR.kappa(split, gkey, br, h2, "kernel")
            for t in SR.fit_cols(br, gkey):
                c = "%s %s %s h2=%s (%s)" % (split, gkey, br, h2, SR.COLS[t])
                r = GR.group_ref(idx, T, V, pn["geno"], np.ascontiguousarray(pn["Y"][:, t]), cov, grp, h2, br)
                np.testing.assert_allclose(r["group_center"], tr["group_center"].astype(np.float64), rtol=1e-14, atol=0)
                # b is one output vector, covariates then levels: its error is relative to its largest entry
                got = np.concatenate(([] if cov is None else [r["cov_effects"][0]]) + [r["group_effects"][0]])
                w.check("b", SR.relerr(got, np.concatenate([tr["cov_effects"][t], tr["group_effects"][t]])), kap, c)
                if t not in SR.fixfit_cols(name, br, gkey):
                    continue
                w.check("effects", SR.relerr(r["effects"][0], tr["effects"][t]), kap, c)
                w.check("ebv valid", SR.relerr(r["ebv"][0], tr["ebv"][t][V]), kap, c)
                w.check("fitness", abs(r["fitness"] - tr["fitness"][t]), kap, c)
        w.show("fit(groups=), " + name)


def _loo_host(w, split, gkey, br, form, h2):
    pn = SR.panel()
    idx, T = pn["genomes"][gkey], pn["splits"][split][0]
    tr = SR.loo_truth(split, gkey, br, h2, form)
    kap = SR.kappa(split, gkey, br, h2, form)
    scale = 1.0 / tr["gap"]
    for t in SR.fit_cols(br, gkey):
        c = "%s %s %s %s h2=%s (%s)" % (split, gkey, br, form, h2, SR.COLS[t])
        r = LO.loo_ref(idx, T, pn["geno"], pn["Y"][:, t], h2, br, form)
        if t == 0:
            w.check("leverage", float(np.max(np.abs(r["leverage"].astype(LD) - tr["leverage"]))), kap, c)
            assert abs(r["gap"] - tr["gap"]) <= SR.host_bar(kap), c
        w.check("pred", SR.relerr(r["pred"], tr["pred"][t]) / scale, kap, c)
        if t in SR.z_cols(br):          # (d) under snp: y - mean(y_T) is rounded at 1e-10 before anything is solved
            w.check("eloo", SR.relerr(r["eloo"], tr["eloo"][t]) / scale, kap, c)
        w.check("press", SR.relerr([r["press"]], [tr["press"][t]]) / scale, kap, c)
        w.check("fitness", abs(r["fitness"] - tr["fitness"][t]) / scale, kap, c)


def test_loo_restatement():
    """loo_ref.loo_ref in both forms against loo_wide: the leverages to host_bar, pred / eloo / PRESS / fitness to
    host_bar / gap (err * gap is what is checked and printed)."""
    w = _Ratios()
    for split, gkey, br, form, h2 in SR.LOO_CASES:
        _loo_host(w, split, gkey, br, form, h2)
    w.show("leave-one-out (pred, eloo, press, fitness: err * gap)")


def test_inputs_left_out_do_miss_the_host_bar():
    """The inputs of the issue that tests/structured_ref.py leaves out (fit_cols, z_cols, the absolute fitness), each with the float64 restatement's own error on it: over host_bar, so no factor could be held to the
    bar there.  The figures are printed; each is asserted to miss, so a change that makes one of them pass shows up
    here and the input can come back."""
    pn = SR.panel()
    g64 = pn["geno"].astype(np.float64)

    def oracle(split, gkey, br, h2, t):
        T, V = pn["splits"][split]
        fn = O.gblup if br == "gblup" else O.snp_blup
        f, e = fn(pn["genomes"][gkey], T, V, g64, np.ascontiguousarray(pn["Y"][:, t]), h2, return_ebv=True)
        truth = SR.fit_truth(split, gkey, br, h2)
        kap = SR.kappa(split, gkey, br, h2, SR.own_form(split, gkey, br))
        return abs(f - truth["fitness"][t]), SR.relerr(e, truth["ebv"][t][V]), truth["fitness"][t], kap

    # (b) alone: the EBVs and effects of the clone contrast are zero (rounding of the longdouble solve), beside 4.3 for (a)
    truth = SR.fit_truth((200, 60), "g400", "gblup", 0.999999)
    print("(b): max |EBV| %.1e, max |effect| %.1e; (a): max |EBV| %.2f" % (
        np.max(np.abs(truth["ebv"][1])), np.max(np.abs(truth["effects"][1])), np.max(np.abs(truth["ebv"][0]))))
    assert np.max(np.abs(truth["ebv"][1])) < 1e-12 and np.max(np.abs(truth["effects"][1])) < 1e-12
    # (d) under snp: z with a float64 mean
    split, gkey, br, h2 = (200, 60), "snp160", "snp", 0.4
    L, z = SR.factor_truth(split, gkey, br, h2)
    y = pn["Y"][pn["splits"][split][0], 3]
    z64 = np.linalg.solve(np.linalg.cholesky(SR._system(split, gkey, br, h2, "kernel")), y - y.mean())
    kap = SR.kappa(split, gkey, br, h2, "kernel")
    ez = SR.relerr(z64, z[:, 3])
    print("(d) under snp: z err %.2e (host bar %.2e)" % (ez, SR.host_bar(kap, SR.CHOL_TOL)))
    assert ez > SR.host_bar(kap, SR.CHOL_TOL)
    # (d) for snp160 under forced gblup: the oracle's K_VT alpha
    for h2 in (0.9999, 0.999999):
        _, de, _, kap = oracle((257, 40), "snp160", "gblup", h2, 3)
        print("(d) snp160 gblup (257, 40) h2=%s: oracle EBV err %.2e = %.2f kappa u (host bar %.2e)" % (
            h2, de, de / (kap * SR.U), SR.host_bar(kap)))
        assert de > SR.host_bar(kap)
    # the fitness relative to |truth|
    df, _, tf, kap = oracle((257, 40), "snp160", "gblup", 0.9999, 2)
    print("fitness relative to |truth|: truth %.4f, err %.2e absolute, %.2e relative (host bar %.2e)" % (
        tf, df, df / tf, SR.host_bar(kap)))
    assert df <= SR.host_bar(kap) < df / tf
    # (d) under gblup with the class factor: the level means absorb the offset, q_P = q - |C^-1 h|^2 cancels twelve digits
    split, gkey, br, h2 = (200, 60), "g400", "gblup", 0.4
    T, V = pn["splits"][split]
    kap = SR.kappa(split, gkey, br, h2, "kernel")
    for name in ("fam", "fam+n"):
        cov, grp = SR.design(name)
        r = GS.adj_ref(pn["genomes"][gkey], T, pn["geno"], pn["Y"], cov, grp, h2, br, SR.cand_snps())
        tr = SR.adj_truth(name, split, gkey, br, h2)
        eq, el = SR.relerr([r["q"][3]], [tr["q"][3]]), _rel1(r["loglik"][3], tr["loglik"][3])
        eu, eb = SR.relerr(r["u"][3], tr["u"][3]), SR.relerr(r["b"][3], tr["b"][3])
        print("(d) g400 gblup %s h2=0.4: q_P %.3e, err %.2e = %.2e host bars, loglik %.2e, u_P %.2e = %.1f host bars; "
              "b %.2e" % (name, float(tr["q"][3]), eq, eq / SR.host_bar(kap), el, eu, eu / SR.host_bar(kap), eb))
        assert eq > SR.host_bar(kap) and el > SR.host_bar(kap) and eu > SR.host_bar(kap) and eb <= SR.host_bar(kap)
        g = GR.group_ref(pn["genomes"][gkey], T, V, pn["geno"], np.ascontiguousarray(pn["Y"][:, 3]), cov, grp, h2, br)
        ft = SR.fixfit_truth(name, split, gkey, br, h2)
        ee, ev = SR.relerr(g["effects"][0], ft["effects"][3]), SR.relerr(g["ebv"][0], ft["ebv"][3][V])
        print("  its fit(groups=) model: effects err %.2e = %.1f host bars, validation EBVs %.2e = %.1f" % (
            ee, ee / SR.host_bar(kap), ev, ev / SR.host_bar(kap)))
        assert ee > SR.host_bar(kap)
    # LOO pred / eloo without the 1 / gap factor at h2 = 0.999999
    split, gkey, br, form, h2 = (200, 60), "dual260", "snp", "kernel", 0.999999
    tr = SR.loo_truth(split, gkey, br, h2, form)
    r = LO.loo_ref(pn["genomes"][gkey], pn["splits"][split][0], pn["geno"], pn["Y"][:, 0], h2, br, form)
    kap = SR.kappa(split, gkey, br, h2, form)
    ee, eh = SR.relerr(r["eloo"], tr["eloo"][0]), float(np.max(np.abs(r["leverage"].astype(LD) - tr["leverage"])))
    print("LOO (200, 60) dual260 snp h2=0.999999 (a): gap %.2e; eloo err %.2e = %.0f host bars, %.3f with the 1 / gap "
          "factor; leverage %.2e = %.3f host bars" % (tr["gap"], ee, ee / SR.host_bar(kap),
                                                      ee * tr["gap"] / SR.host_bar(kap), eh, eh / SR.host_bar(kap)))
    assert ee > SR.host_bar(kap) >= ee * tr["gap"] and eh <= SR.host_bar(kap)


# ---------------------------------------------------------------------------------------------
# h2 = 1
# ---------------------------------------------------------------------------------------------
def test_h2_one_positive_definite_cases():
    """lambda = 0 on systems that are positive definite on their own: treated as any other case."""
    w = _Ratios()
    for split, gkey, br, form in SR.PD_CASES:
        kap = SR.kappa(split, gkey, br, 1.0, form)
        print("h2 = 1 %s %s %s: kappa %.2e" % (split, gkey, br, kap))
        assert SR.own_form(split, gkey, br) == form and kap < 1e6
        _fit_host(w, split, gkey, br, 1.0, form)
    w.show("h2 = 1")


def test_h2_one_singular_cases():
    """The longdouble Cholesky finds no positive pivot (and the float64 spectrum has no positive end): there is no
    truth, and the GPU tests only ask for a clean return and untouched batch-mates -- which are positive definite."""
    pd = {(c[0], c[1], c[2]) for c in SR.PD_CASES}
    singular = [(split, batch[pos], br, form) for _, split, br, form, batch, pos in SR.SINGULAR_CASES]
    singular += [c[1:] for c in SR.SINGULAR_ALONE]
    for split, gkey, br, form in singular:
        lo, hi = SR._spectrum(split, gkey, SR.fitted_branch(gkey, br), form)
        print("h2 = 1 singular %s %s %s: smallest eigenvalue / largest %.1e" % (split, gkey, br, lo / hi))
        assert SR.fit_truth(split, gkey, br, 1.0) is None          # every one of them: the Cholesky finds no pivot
        assert lo < 1e-13 * hi
    for _, split, br, form, batch, pos in SR.SINGULAR_CASES:
        assert 0 < pos < len(batch) - 1
        assert SR.form_of(batch, split, br) == form
        for i, gkey in enumerate(batch):
            assert i == pos or (split, gkey, br) in pd
