"""Everything that reads the factor, on the structured panel of tests/structured_ref.py -- LD blocks, full sibs,
clones inside a pivot block and across a tile boundary, rare alleles, a repeated and a complemented column -- at
h2 = 0.4, 0.99, 0.9999, 0.999999 and 1, against the longdouble truth under

    bar = max(TOL, 16 kappa 2^-53)

kappa the 2-norm condition number of the system the library solves in the form it takes (tests/structured_ref.py:
kappa, form_of), TOL the flat tolerance of the existing GPU tests (1e-9; 1e-10 for the factor readback).  The
error is relative to the largest |truth| of the output vector, absolute for reliabilities and -- a departure from
the issue, which makes only reliabilities absolute; tests/structured_ref.py says why -- for the fitness, relative to
max(1, |truth|) for log-likelihood terms.  tests/test_structured_host.py holds LAPACK to an eighth of this bar
on every case here.  kappa runs from 15 to 3e7; from about 6e5 on the bar is kappa's.

  A  K_TT + lambda I and K_VT (debug_grm stage 1), the factor L and z = L^-1 (y_T - mu) (stage 2), every phenotype
     column; the tile-by-tile residual, pivot and substitution figures that localise a miss are printed
  B  evaluate / fit / predict: EBVs of all animals, effects, intercept, fitness; the ragged batch of four genomes and
     each alone; auto, gblup and snp; one, three and four traits; h2 = 1 on positive-definite systems
  C  TBLUP_FORM 1 / 2 and TBLUP_PAD_FIRST under the bar; TBLUP_SOLVE_CHAIN / TBLUP_SOLVE_PULL and TBLUP_DIAG_WAVES
     bit-identical
  D  reliability, log_likelihood, estimate_h2, snp_scores, fit(covariates)
  E  h2 = 1 on singular systems: a clean return, no infinity, bit-identical batch-mates
  F  the one model and column over the bar (forced gblup at k < n_T with the 1e6 offset): strict expected failures
  G to K  (tests/test_gpu_structured_fixed.py) the entries that adjust for covariates and a class factor confounded
     with relationship -- adjusted scores and likelihood, adjusted reliabilities, the wide GLS fit -- and leave-one-out
     under the rule bar / min (1 - h_tt); two more inputs are left out there ((d) under gblup with the class factor;
     LOO pred without the 1 / gap factor), each with its figure in tests/test_structured_host.py

Each test prints its worst err / bar per quantity (pytest -s); PERFLOG.md holds the figures of the last run.
"""
import numpy as np
import pytest

from tests import covar_ref as CV
from tests import loglik_ref as LL
from tests import structured_ref as SR
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

LD = np.longdouble
ALL = np.arange(SR.N_ANIMALS)
ENGINES = {"a": (0,), "b": (1,), "c": (2,), "d": (3,), "ab": (4,), "mt3": (0, 4, 2), "mt4": SR.MT_COLS}


class _Worst:
    """Worst err / bar per quantity.  Every error is held against bar(kappa); the misses are collected, so that one
    run names them all, and show() fails on any."""

    def __init__(self, label):
        self.label, self.v, self.missed = label, {}, []

    def check(self, quantity, err, kappa, name, tol=SR.TOL):
        assert np.isfinite(err), (quantity, name)
        b = SR.bar(kappa, tol)
        if err / b >= self.v.get(quantity, (-1.0,))[0]:
            self.v[quantity] = (err / b, err, kappa, name)
        if not err <= b:
            self.missed.append("MISS %s %s: err %.3e > bar %.3e (kappa %.2e): err / bar %.2f" % (quantity, name, err, b, kappa, err / b))

    def show(self):
        print("\nSTRUCTURED %s: worst err / bar" % self.label)
        for q, (r, err, kappa, name) in sorted(self.v.items()):
            print("  %-14s %.4f  (err %.2e, kappa %.2e, %s)" % (q, r, err, kappa, name))
        print("\n".join(self.missed))
        assert not self.missed, "%d over the bar:\n%s" % (len(self.missed), "\n".join(self.missed))


@pytest.fixture(scope="module")
def engines(gpu):
    """One context per phenotype layout, created on first use and closed with the module."""
    import contextlib
    pn = SR.panel()
    with contextlib.ExitStack() as stack:
        made = {}

        def get(key):
            if key not in made:
                made[key] = stack.enter_context(_engine(pn["geno"], SR.pheno(ENGINES[key])))
            return made[key]
        yield get


def _name(split, gkey, br, h2, extra=""):
    return "%s %s %s h2=%s%s" % (split, gkey, br, h2, extra)


# ---------------------------------------------------------------------------------------------
# A. the factor
# ---------------------------------------------------------------------------------------------
def _tiles(E, scale):
    """max |E| / scale over each 128 x 128 tile of the lower triangle: how section A localises a miss."""
    nt = -(-E.shape[0] // 128)
    return " ".join("[%d,%d] %.1e" % (i, j, float(np.max(np.abs(E[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128])) / scale))
                    for i in range(nt) for j in range(i + 1))


def _where(F, L):
    """The entry with the largest error of a factor, and the error of every tile relative to max |L|."""
    e = np.abs(F.astype(LD) - L)
    i, j = np.unravel_index(int(np.argmax(e)), e.shape)
    return "largest at L[%d, %d] (16-row block (%d, %d): %s); per tile %s" % (
        i, j, i // 16, j // 16, "diagonal block" if i // 16 == j // 16 else "off-diagonal panel",
        _tiles(F.astype(LD) - L, float(np.max(np.abs(L)))))


K_RTOL = 1e-12          # the K block read back (tests/test_gpu_edges.py): nothing is solved, so no kappa term


@pytest.mark.parametrize("split", SR.SPLITS, ids=str)
def test_a_factor_and_forward_solve(engines, split):
    """debug_grm of the kernel-form system: stage 1's K_TT + lambda I (lower triangle) and K_VT against the exact
    counts, stage 2's L and z against the longdouble factor.  Printed beside them, to tell where an error enters:
    the residual F F^T - A of every tile (the factor's backward error; numpy's Cholesky of the same matrix beside
    it), the largest relative error of a pivot, and z once more by numpy's substitution on the GPU's own F -- if
    that z is good and the library's is not, the forward solve (the multiplication by X = L_JJ^-1) loses it, not
    the factor.  (The validation rows K_VT L^-T are not part of the stage-2 readback.)"""
    import scipy.linalg
    pn = SR.panel()
    T, V = pn["splits"][split]
    nT = len(T)
    w = _Worst("A factor %s" % (split,))
    for s, gkey, br, h2 in SR.FACTOR_CASES:
        if s != split:
            continue
        L, z = SR.factor_truth(split, gkey, br, h2)
        kap = SR.kappa(split, gkey, br, h2, "kernel")
        name = _name(split, gkey, br, h2)
        A = SR.k_truth(split, gkey, br)[:nT].copy()
        A[np.diag_indices(nT)] += (LD(1) - LD(h2)) / LD(h2)
        scale = float(np.max(np.abs(A)))
        K, _ = engines("a").debug_grm(pn["genomes"][gkey], T, V, h2, branch=br, stage=1)
        w.check("K_TT", float(np.max(np.abs(np.tril(K[:nT].astype(LD) - A)))) / scale, 1.0, name, K_RTOL)
        w.check("K_VT", float(np.max(np.abs(K[nT:].astype(LD) - SR.k_truth(split, gkey, br)[nT:]))) / scale, 1.0, name, K_RTOL)
        for t in SR.z_cols(br):
            F, zz = engines(SR.COLS[t]).debug_grm(pn["genomes"][gkey], T, V, h2, branch=br, stage=2)
            F = np.tril(F[:nT])
            if t == 0:
                err = SR.relerr(F, L)
                L64 = np.linalg.cholesky(A.astype(np.float64))
                Fl = F.astype(LD)
                piv = float(np.max(np.abs(np.diag(Fl) ** 2 - np.diag(L) ** 2) / np.diag(L) ** 2))
                piv64 = float(np.max(np.abs(np.diag(L64).astype(LD) ** 2 - np.diag(L) ** 2) / np.diag(L) ** 2))
                print("factor %s: kappa %.2e, L err %.2e (numpy %.2e), %s" % (name, kap, err, SR.relerr(L64, L), _where(F, L)))
                print("  residual F F^T - A / max |A| per tile: %s\n  numpy's:                              %s" % (
                    _tiles(np.tril(Fl @ Fl.T - A), scale), _tiles(np.tril(L64.astype(LD) @ L64.T.astype(LD) - A), scale)))
                print("  largest relative error of a pivot: %.2e (numpy %.2e)" % (piv, piv64))
                w.check("L", err, kap, name, SR.CHOL_TOL)
            y = pn["Y"][T, t] - (pn["Y"][T, t].mean() if br == "snp" else 0.0)
            z_own = scipy.linalg.solve_triangular(F, y, lower=True)
            z_np = scipy.linalg.solve_triangular(L64, y, lower=True)
            ez = SR.relerr(zz, z[:, t])
            print("  z (%s): library %.2e, numpy's substitution on the library's F %.2e, numpy's on numpy's %.2e" % (
                SR.COLS[t], ez, SR.relerr(z_own, z[:, t]), SR.relerr(z_np, z[:, t])))
            w.check("z", ez, kap, name + " (%s)" % SR.COLS[t], SR.CHOL_TOL)
    w.show()


# ---------------------------------------------------------------------------------------------
# B. evaluate, fit, predict
# ---------------------------------------------------------------------------------------------
RDO = ("g130", "gblup", 3)      # the rank-deficient gblup model with the offset column: section F, an open finding


def _not_rdo(gkey, br, t):
    return (gkey, br, t) != RDO


def _check_fit(w, eng, cols, split, gkeys, branch, h2, form, tag, compared=_not_rdo):
    """evaluate(return_ebv), fit and predict of one batch on one engine against fit_truth, trait by trait."""
    pn = SR.panel()
    T, V = pn["splits"][split]
    genomes = [pn["genomes"][g] for g in gkeys]
    fit, ebv = eng.evaluate(genomes, T, V, h2, branch=branch, return_ebv=True)
    models = eng.fit(genomes, T, V, h2, branch=branch)
    herd = eng.predict(models, ALL)
    nt = len(cols)
    ebv, herd = ebv.reshape(len(gkeys), nt, len(V)), herd.reshape(len(gkeys), nt, SR.N_ANIMALS)
    assert not eng.index_error()
    for i, gkey in enumerate(gkeys):
        br = SR.fitted_branch(gkey, branch)
        truth = SR.fit_truth(split, gkey, br, h2)
        kap = SR.kappa(split, gkey, br, h2, form)
        m = models[i]
        assert m.branch == br and m.effects.shape == (nt, len(genomes[i]))
        assert m.fitness == fit[i]
        for j, t in enumerate(cols):
            if t not in SR.fit_cols(br, gkey) or not compared(gkey, br, t):
                continue
            name = _name(split, gkey, br, h2, " (%s) %s" % (SR.COLS[t], tag))
            w.check("effects", SR.relerr(m.effects[j], truth["effects"][t]), kap, name)
            w.check("ebv all", SR.relerr(herd[i, j], truth["ebv"][t]), kap, name)
            w.check("ebv valid", SR.relerr(ebv[i, j], truth["ebv"][t][V]), kap, name)
            if br == "gblup":
                assert m.intercept[j] == 0.0, name
            else:
                w.check("intercept", SR.relerr([m.intercept[j]], [truth["intercept"][t]]), kap, name)
        if set(cols) <= set(SR.FITNESS_COLS):
            want = float(np.mean([truth["fitness"][t] for t in cols]))
            w.check("fitness", abs(fit[i] - want), kap, _name(split, gkey, br, h2, " " + tag))


@pytest.mark.parametrize("branch", ["auto", "gblup", "snp"])
@pytest.mark.parametrize("split", SR.SPLITS, ids=str)
def test_b_evaluate_fit_predict(engines, split, branch):
    """The ragged batch of the four genomes (k = 400 beside k = 130: the kernel form under auto) and each genome
    alone (the SNP form where it gives no more tiles), single-trait on (ab), three traits and four."""
    w = _Worst("B %s %s" % (split, branch))
    for h2 in SR.H2S:
        for key in ("ab", "mt3", "mt4"):
            eng, cols = engines(key), ENGINES[key]
            _check_fit(w, eng, cols, split, SR.GENOMES, branch, h2, SR.form_of(SR.GENOMES, split, branch), key + " batch")
            if key != "mt3":
                for g in SR.GENOMES:
                    _check_fit(w, eng, cols, split, [g], branch, h2, SR.form_of([g], split, branch), key + " alone")
    w.show()


def test_b_h2_one_positive_definite(engines):
    """lambda = 0 where the system is positive definite on its own: under the bar like any other case."""
    w = _Worst("B h2 = 1")
    for split, gkey, br, form in SR.PD_CASES:
        assert SR.form_of([gkey], split, br) == form
        for key in ("ab", "mt3"):
            _check_fit(w, engines(key), ENGINES[key], split, [gkey], br, 1.0, form, key)
    w.show()


# ---------------------------------------------------------------------------------------------
# C. forms and kernels under stress
# ---------------------------------------------------------------------------------------------
SNP_GENOMES = ("snp160", "g130", "dual260")


@pytest.mark.parametrize("env,form", [({"TBLUP_FORM": "1"}, "kernel"), ({"TBLUP_FORM": "2"}, "snp"),
                                      ({"TBLUP_FORM": "2", "TBLUP_PAD_FIRST": "1"}, "snp"),
                                      ({"TBLUP_FORM": "2", "TBLUP_PAD_FIRST": "0"}, "snp")],
                         ids=["form1", "form2", "form2-pad-first", "form2-pad-last"])
def test_c_forms_under_the_bar(gpu, env, form):
    """The snp-branch genomes in the kernel form and in the SNP form (padding rows leading and trailing): each is
    under the bar against the truth; they need not agree with each other beyond that."""
    pn = SR.panel()
    w = _Worst("C %s" % env)
    with _engine(pn["geno"], SR.pheno(ENGINES["mt3"]), env) as eng:
        for split in SR.SPLITS:
            for h2 in (0.4, 0.999999):
                _check_fit(w, eng, ENGINES["mt3"], split, SNP_GENOMES, "auto", h2, form, "batch")
                _check_fit(w, eng, ENGINES["mt3"], split, ["snp160"], "auto", h2, form, "alone")
    w.show()


def _bits(eng, split, h2):
    """Every output of evaluate / fit / predict of the mixed batch (kernel form) and of the snp batch (SNP form)."""
    pn = SR.panel()
    T, V = pn["splits"][split]
    out = []
    for gkeys in (SR.GENOMES, ("snp160", "g130")):
        genomes = [pn["genomes"][g] for g in gkeys]
        fit, ebv = eng.evaluate(genomes, T, V, h2, return_ebv=True)
        models = eng.fit(genomes, T, V, h2)
        out += [fit, ebv, eng.predict(models, ALL)] + [a for m in models for a in (m.effects, m.intercept, np.asarray(m.fitness))]
    return out


def _same_bits(a, b, msg):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.all(np.isfinite(x)), (msg, i)
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (msg, i)


SOLVE_SETTINGS = [{"TBLUP_SOLVE_CHAIN": "0"}, {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "1"},
                  {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "0"}]
WAVE_SETTINGS = [{"TBLUP_DIAG_WAVES": "8"}, {"TBLUP_DIAG_WAVES": "16"}]


@pytest.mark.parametrize("settings", [SOLVE_SETTINGS, WAVE_SETTINGS], ids=["solve-kernels", "diag-waves"])
def test_c_kernel_variants_are_bit_identical(gpu, settings):
    """The solve kernels and the diagonal kernel's wave counts run the same chains on the same operands: the same
    bits at kappa = 3e7 as at kappa = 20 (tests/test_gpu_model.py, tests/test_gpu_diag_waves.py)."""
    pn = SR.panel()
    got = []
    for env in settings:
        with _engine(pn["geno"], SR.pheno(ENGINES["mt3"]), env) as eng:
            got.append([_bits(eng, split, h2) for split in SR.SPLITS for h2 in (0.999999, 0.9999)])
    for env, g in zip(settings[1:], got[1:]):
        for a, b in zip(g, got[0]):
            _same_bits(a, b, str(env))


# ---------------------------------------------------------------------------------------------
# D. everything else that reads the factor
# ---------------------------------------------------------------------------------------------
def _aux_groups(cases):
    """(split, h2) -> the calls that cover its cases: the auto-branch models as one batch (kernel form) and each
    alone, the forced gblup model alone."""
    out = {}
    for split, gkey, br, h2 in cases:
        out.setdefault((split, h2), []).append((gkey, br))
    calls = {}
    for key, models in out.items():
        auto = [g for g, br in models if SR.fitted_branch(g, "auto") == br]
        forced = [(g, br) for g, br in models if SR.fitted_branch(g, "auto") != br]
        calls[key] = ([(tuple(auto), "auto", "batch")] if len(auto) > 1 else []) + [((g,), "auto", "alone") for g in auto] \
            + [((g,), br, "alone") for g, br in forced]
    return calls


def test_d_reliability(engines):
    pn = SR.panel()
    an = SR.rel_animals()
    eng = engines("a")
    w = _Worst("D reliability")
    for (split, h2), calls in _aux_groups(SR.AUX_CASES).items():
        T, V = pn["splits"][split]
        for gkeys, branch, tag in calls:
            rel = eng.reliability([pn["genomes"][g] for g in gkeys], T, V, h2, an, branch=branch)
            form = SR.form_of(gkeys, split, branch)
            for i, g in enumerate(gkeys):
                br = SR.fitted_branch(g, branch)
                kap = SR.kappa(split, g, br, h2, form)
                truth = SR.rel_truth(split, g, br, h2)[an]
                name = _name(split, g, br, h2, " " + tag)
                w.check("reliability", float(np.max(np.abs(rel[i].astype(LD) - truth))), kap, name)
                b = SR.bar(kap)
                assert np.all(rel[i] >= -b) and np.all(rel[i] <= 1 + b), name
                n_cl = len(sum(pn["clones"].values(), ()))
                w.check("r2 of clones", float(np.max(np.abs(rel[i][:n_cl].astype(LD) - truth[:n_cl]))), kap, name)
    w.show()


def test_d_log_likelihood(engines):
    """Per-model h2 values (a (G, B) matrix: model b takes the values rotated by b), every phenotype column."""
    pn = SR.panel()
    w = _Worst("D log-likelihood")
    for (split, _), calls in _aux_groups([c for c in SR.LL_CASES if c[3] == 0.999999]).items():
        T, V = pn["splits"][split]
        hs = [h for s, g, br, h in SR.LL_CASES if s == split and (g, br) == SR.AUX_MODELS[0]]
        for key in ("mt4", "b"):
            eng, cols = engines(key), ENGINES[key]
            for gkeys, branch, tag in calls:
                B, G = len(gkeys), len(hs)
                hm = np.array([[hs[(r + b) % G] for b in range(B)] for r in range(G)])
                ll, s2 = eng.log_likelihood([pn["genomes"][g] for g in gkeys], T, V, hm, branch=branch, return_sigma2=True)
                ll, s2 = ll.reshape(G, B, len(cols)), s2.reshape(G, B, len(cols))
                for r in range(G):
                    for i, g in enumerate(gkeys):
                        br = SR.fitted_branch(g, branch)
                        tl, ts = SR.loglik_truth(split, g, br, hm[r, i])
                        kap = SR.kappa(split, g, br, hm[r, i], SR.form_of(gkeys, split, branch))
                        for j, t in enumerate(cols):
                            if not _not_rdo(g, br, t):
                                continue
                            name = _name(split, g, br, hm[r, i], " (%s) %s" % (SR.COLS[t], tag))
                            w.check("loglik", float(abs(LD(ll[r, i, j]) - tl[t]) / max(LD(1), abs(tl[t]))), kap, name)
                            w.check("sigma2_g", float(abs(LD(s2[r, i, j]) - ts[t]) / max(LD(1), abs(ts[t]))), kap, name)
    w.show()


def test_d_estimate_h2(engines):
    """On the breeding-value column the estimate lands within the last refinement step of the same procedure on
    the float64 restatement's own values."""
    pn = SR.panel()
    T, V = pn["splits"][200, 60]
    eng = engines("c")
    y = SR.pheno(ENGINES["c"])
    for gkeys, branch in ((("snp160", "dual260", "g400"), "auto"), (("g130", "g400"), "gblup")):
        genomes = [pn["genomes"][g] for g in gkeys]
        est = eng.estimate_h2(genomes, T, V, branch=branch)
        for i, g in enumerate(gkeys):
            ref = LL.estimate_ref(genomes[i], T, pn["geno"], y, branch)
            print("estimate_h2 %s %s: %.6f (restatement %.6f, step %.2e, loglik %.6f / %.6f)" % (
                g, branch, est["h2"][i], ref["h2"], ref["step"], est["loglik"][i], ref["loglik"]))
            assert 0.02 < ref["h2"] < 0.98 and not ref["at_bound"]
            assert abs(est["step"][i] - ref["step"]) <= 1e-12 and est["at_bound"][i] == ref["at_bound"]
            assert abs(est["h2"][i] - ref["h2"]) <= ref["step"], (g, branch)
            if est["h2"][i] == ref["h2"]:
                assert LL.close(est["loglik"][i], ref["loglik"]) <= LL.TOL


def test_d_snp_scores(engines):
    pn = SR.panel()
    cand = SR.cand_snps()
    w = _Worst("D SNP scores")
    for (split, h2), calls in _aux_groups(SR.AUX_CASES).items():
        T, V = pn["splits"][split]
        for key in ("mt4", "b"):
            eng, cols = engines(key), ENGINES[key]
            for gkeys, branch, tag in calls:
                sc = eng.snp_scores([pn["genomes"][g] for g in gkeys], T, V, h2, cand, branch=branch)
                form = SR.form_of(gkeys, split, branch)
                for i, g in enumerate(gkeys):
                    br = SR.fitted_branch(g, branch)
                    tu, tv, tq = SR.score_truth(split, g, br, h2)
                    kap = SR.kappa(split, g, br, h2, form)
                    name = _name(split, g, br, h2, " " + tag)
                    w.check("info v", SR.relerr(sc.info[i], tv), kap, name)
                    for j, t in enumerate(cols):
                        if not _not_rdo(g, br, t):
                            continue
                        w.check("q", SR.relerr([sc.q[i, j]], [tq[t]]), kap, name + " (%s)" % SR.COLS[t])
                        if t in SR.fit_cols(br, g):
                            w.check("score u", SR.relerr(sc.score[i, j], tu[t]), kap, name + " (%s)" % SR.COLS[t])
    w.show()


def test_d_covariates(engines):
    """Three covariates, the first the indicator of the in-block clone pair's family; cond(Q~^T V^-1 Q~) stays under
    covar_ref.COND_MAX, so the documented NaN threshold of a collinear Q is not what is tested."""
    pn = SR.panel()
    Qm = SR.covariates()
    eng, cols = engines("mt4"), ENGINES["mt4"]
    w = _Worst("D covariates")
    for (split, h2), calls in _aux_groups(SR.AUX_CASES).items():
        T, V = pn["splits"][split]
        for gkeys, branch, tag in calls:
            models, ebv = eng.fit([pn["genomes"][g] for g in gkeys], T, V, h2, branch=branch, covariates=Qm, return_ebv=True)
            form = SR.form_of(gkeys, split, branch)
            for i, g in enumerate(gkeys):
                br = SR.fitted_branch(g, branch)
                truth = SR.gls_truth(split, g, br, h2)
                assert truth["cond"] < CV.COND_MAX
                kap = SR.kappa(split, g, br, h2, form)
                np.testing.assert_allclose(models[i].cov_center, truth["m"].astype(np.float64), rtol=1e-14, atol=0)
                for j, t in enumerate(cols):
                    if t not in SR.fit_cols(br, g):
                        continue
                    name = _name(split, g, br, h2, " (%s) %s" % (SR.COLS[t], tag))
                    w.check("cov effects", SR.relerr(models[i].cov_effects[j], truth["b"][t]), kap, name)
                    w.check("effects", SR.relerr(models[i].effects[j], truth["effects"][t]), kap, name)
                    w.check("ebv valid", SR.relerr(ebv[i, j], truth["ebv"][t][V]), kap, name)
    w.show()


# ---------------------------------------------------------------------------------------------
# E. h2 = 1 on singular systems
# ---------------------------------------------------------------------------------------------
def _run_e(eng, split, gkeys, branch):
    pn = SR.panel()
    T, V = pn["splits"][split]
    genomes = [pn["genomes"][g] for g in gkeys]
    fit, ebv = eng.evaluate(genomes, T, V, 1.0, branch=branch, return_ebv=True)
    models = eng.fit(genomes, T, V, 1.0, branch=branch)
    assert not eng.index_error()
    return fit, ebv, models


@pytest.mark.parametrize("case", SR.SINGULAR_CASES, ids=[c[0] for c in SR.SINGULAR_CASES])
def test_e_singular_individual_leaves_its_batch_alone(engines, case):
    """lambda = 0 and a system with no inverse (a repeated column in the SNP form; fewer columns than train rows in
    the kernel form) between two positive-definite ones: the call returns, the singular individual's fitness is NaN
    or finite -- which of the two is not asserted, the reference's inverse is as undefined -- never infinite, no
    index error is raised, and its batch-mates have the bits they have without it."""
    _, split, branch, form, batch, pos = case
    mates = [g for i, g in enumerate(batch) if i != pos]
    for key in ("ab", "mt3"):
        eng = engines(key)
        fit, ebv, models = _run_e(eng, split, batch, branch)
        assert not np.isinf(fit[pos]) and not np.isinf(models[pos].fitness)
        fit0, ebv0, models0 = _run_e(eng, split, mates, branch)
        keep = [i for i in range(len(batch)) if i != pos]
        assert np.all(np.isfinite(fit0)) and np.all(np.isfinite(ebv0))
        assert fit[keep].tobytes() == fit0.tobytes()
        assert np.ascontiguousarray(ebv[keep]).tobytes() == ebv0.tobytes()
        for i, m0 in zip(keep, models0):
            assert models[i].effects.tobytes() == m0.effects.tobytes()
            assert models[i].intercept.tobytes() == m0.intercept.tobytes()
            assert models[i].fitness == m0.fitness


@pytest.mark.parametrize("case", SR.SINGULAR_ALONE, ids=[c[0] for c in SR.SINGULAR_ALONE])
def test_e_singular_train_rows(engines, case):
    """Clones among the train rows make every kernel-form system of the batch singular at lambda = 0, so there is no
    healthy batch-mate to compare: the call returns, nothing is infinite, no index error."""
    _, split, gkey, branch, _ = case
    fit, ebv, models = _run_e(engines("ab"), split, [gkey], branch)
    assert not np.isinf(fit[0]) and not np.isinf(models[0].fitness)


# ---------------------------------------------------------------------------------------------
# F. the offset in the null space of a rank-deficient gblup system: an open finding (PERFLOG.md)
# ---------------------------------------------------------------------------------------------
F_MISSES = {((200, 60), 0.999999): "ebv valid 1.21",
            ((257, 40), 0.9999): "ebv valid 2.23 (err 2.2e-9 against the flat 1e-9: 73 kappa u)",
            ((257, 40), 0.999999): "ebv valid 2.92, effects 1.29, ebv all 1.28, q 1.25, sigma2_g 1.25, score u 1.21"}


@pytest.mark.parametrize("split,h2", [
    pytest.param(s, h, id="%s-%s" % (s, h), marks=[pytest.mark.xfail(strict=True, reason="err / bar: " + F_MISSES[s, h])]
                 if (s, h) in F_MISSES else []) for s in SR.SPLITS for h in SR.H2S])
def test_f_offset_in_the_null_space(engines, split, h2):
    """g130 under forced gblup with column (d): k = 130 < n_T, so K_TT has a null space of n_T - 130 directions beside
    the clones', gblup fits no mean, and the offset 1e6 lies largely in that null space -- the solution is its
    component there over lambda, and every output is a small difference of it.  The only model and column of this
    file that miss the bar, from h2 = 0.9999 on: err / bar 1.2 to 2.9 (19 to 73 kappa u, where LAPACK stays under
    1.2 kappa u); the same model passes on the other columns, and the other models pass on (d).  Every comparison
    of sections B and D for this model and column is made here, one parametrisation per (split, h2); those that
    miss are strict expected failures with the measured ratios.  Section A has localised it (PERFLOG.md): K_TT and
    K_VT are exact to 4e-16, F F^T - A is LAPACK's, and plain substitution on the library's own F reproduces its z,
    so the forward solve is not the source -- the null-direction pivots of tile [1,1] are ten times further from the
    truth than LAPACK's.  The fix belongs in the diagonal chain of k_chol.hip."""
    pn = SR.panel()
    T, V = pn["splits"][split]
    gkey, br, t = RDO

    def only(g, b, c):
        return (g, b, c) == RDO
    w = _Worst("F %s h2=%s" % (split, h2))
    for key in ("d", "mt4"):
        eng, cols = engines(key), ENGINES[key]
        j = cols.index(t)
        _check_fit(w, eng, cols, split, [gkey], br, h2, "kernel", key + " alone", only)
        _check_fit(w, eng, cols, split, SR.GENOMES, br, h2, "kernel", key + " batch", only)
        kap = SR.kappa(split, gkey, br, h2, "kernel")
        name = _name(split, gkey, br, h2, " (d) " + key)
        if (split, gkey, br, h2) in SR.LL_CASES:
            ll, s2 = eng.log_likelihood([pn["genomes"][gkey]], T, V, h2, branch=br, return_sigma2=True)
            tl, ts = SR.loglik_truth(split, gkey, br, h2)
            w.check("loglik", float(abs(LD(ll.reshape(1, -1)[0, j]) - tl[t]) / max(LD(1), abs(tl[t]))), kap, name)
            w.check("sigma2_g", float(abs(LD(s2.reshape(1, -1)[0, j]) - ts[t]) / max(LD(1), abs(ts[t]))), kap, name)
        if (split, gkey, br, h2) in SR.AUX_CASES:
            sc = eng.snp_scores([pn["genomes"][gkey]], T, V, h2, SR.cand_snps(), branch=br)
            tu, tv, tq = SR.score_truth(split, gkey, br, h2)
            w.check("q", SR.relerr([sc.q[0, j]], [tq[t]]), kap, name)
            w.check("score u", SR.relerr(sc.score[0, j], tu[t]), kap, name)
    w.show()
