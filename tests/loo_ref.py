"""Float64 restatement of the leave-one-out closed forms (TEST INFRASTRUCTURE ONLY), the brute-force refit
they stand for, and the inputs shared by tests/test_loo_host.py (CPU) and tests/test_gpu_loo.py (GPU).

Per fitted model and trait, with T the training animals in `train` order, lambda = (1 - h2) / h2, w_t the
animal's centred row (tests/reliability_ref.py's notation), c = 0 and mu = 0 under gblup, c = 1 / n_T and
mu = mean(y_T) under snp:

  SNP form     L L^T = W_T^T W_T / d + lambda I:  h_tt = c + |L^-1 w_t|^2 / d,  e_t = y_t - mu - w_t . beta,
               e_loo,t = e_t / (1 - h_tt)
  kernel form  L L^T = V = K_TT + lambda I, alpha = V^-1 (y_T - mu):  (V^-1)_tt = |L^-1 e_t|^2,
               e_loo,t = lambda alpha_t / (lambda (V^-1)_tt - c),  h_tt = 1 + c - lambda (V^-1)_tt
  y^_loo,t = y_t - e_loo,t,  PRESS = sum_t e_loo,t^2,  fitness = |pearson(y^_loo, y_T)|

The brute force: under gblup oracle.gblup trained on T without t predicting t; under snp oracle's
_ridge_predict on the raw genotype columns of T without t with the fitted model's own penalty lambda d kept
(d from the full training set).  The latter is not the reference pipeline re-run with t removed, which would
also change p and d.
"""
import functools

import numpy as np

from oracle import blup_oracle as O
from tests import model_ref as R
from tests import reliability_ref as Q

LD = np.longdouble
H2 = Q.H2
K40, K300 = 40, Q.K300


def loo_ref(idx, train, geno, pheno, h2, branch="auto", form=None):
    """{pred, leverage, eloo (n_T,), press, fitness, gap = min(1 - h_tt)} of one phenotype vector in float64;
    form "snp" / "kernel" (None: the smaller system)."""
    T = np.asarray(train)
    nT = len(T)
    y = np.asarray(pheno, dtype=np.float64)[T]
    branch = R._branch(len(idx), np.asarray(geno).shape[0], branch)
    _, wt, d, lam = Q._setup(idx, T, geno, h2, branch, np.float64)
    nan = {"pred": np.full(nT, np.nan), "leverage": np.full(nT, np.nan), "eloo": np.full(nT, np.nan),
           "press": np.nan, "fitness": np.nan, "gap": np.nan}
    if not d > 0:
        return nan
    c = 0.0 if branch == "gblup" else 1.0 / nT
    r = y - (0.0 if branch == "gblup" else y.mean())
    if form is None:
        form = "snp" if wt.shape[1] <= nT else "kernel"
    with np.errstate(all="ignore"):
        if form == "snp":
            A = (wt.T @ wt) / d
            A[np.diag_indices_from(A)] += lam
            L = Q._chol(A)
            if L is None:
                return nan
            beta = R._chol_solve(A, (wt.T @ r) / d)
            s = Q._forward(L, np.ascontiguousarray(wt.T))
            h = c + np.sum(s * s, axis=0) / d
            eloo = (r - wt @ beta) / (1.0 - h)
        else:
            A = (wt @ wt.T) / d
            A[np.diag_indices_from(A)] += lam
            L = Q._chol(A)
            if L is None:
                return nan
            alpha = R._chol_solve(A, r)
            s = Q._forward(L, np.eye(nT))
            vtt = np.sum(s * s, axis=0)
            eloo = lam * alpha / (lam * vtt - c)
            h = 1.0 + c - lam * vtt
        pred = y - eloo
        return {"pred": pred, "leverage": h, "eloo": eloo, "press": float(np.sum(eloo * eloo)),
                "fitness": abs(O.pearson_r(pred, y)), "gap": float(np.min(1.0 - h))}


def loo_wide(idx, train, geno, pheno, h2, branch="auto", form=None):
    """loo_ref's arithmetic in np.longdouble (the centred rows, d and lambda from the exact counts, one longdouble
    column Cholesky), the fitness from tests/test_edge_cases_cpu.py::_pearson_wide.  pheno (n,) gives loo_ref's
    shapes; (n, t) gives pred / eloo (t, n_T), press / fitness (t,) from one factor.  None where the system is
    not positive definite."""
    from tests.test_edge_cases_cpu import _pearson_wide
    T = np.asarray(train)
    nT = len(T)
    Y = np.asarray(pheno, dtype=np.float64)
    one = Y.ndim == 1
    y = (Y[:, None] if one else Y)[T].astype(LD)
    branch = R._branch(len(idx), np.asarray(geno).shape[0], branch)
    _, wt, d, lam = Q._setup(idx, T, geno, h2, branch, LD)
    if not d > 0:
        return None
    c = LD(0) if branch == "gblup" else LD(1) / LD(nT)
    r = y - (LD(0) if branch == "gblup" else y.sum(axis=0) / LD(nT))
    if form is None:
        form = "snp" if wt.shape[1] <= nT else "kernel"
    if form == "snp":
        A = (wt.T @ wt) / d
        A[np.diag_indices_from(A)] += lam
        L = Q._chol(A)
        if L is None:
            return None
        beta = R._chol_solve(A, (wt.T @ r) / d)
        s = Q._forward(L, np.ascontiguousarray(wt.T))
        h = c + np.sum(s * s, axis=0) / d
        eloo = (r - wt @ beta) / (LD(1) - h)[:, None]
    else:
        A = (wt @ wt.T) / d
        A[np.diag_indices_from(A)] += lam
        L = Q._chol(A)
        if L is None:
            return None
        alpha = R._chol_solve(A, r)
        s = Q._forward(L, np.eye(nT, dtype=LD))
        vtt = np.sum(s * s, axis=0)
        eloo = lam * alpha / (lam * vtt - c)[:, None]
        h = LD(1) + c - lam * vtt
    pred = y - eloo
    fit = np.array([_pearson_wide(pred[:, t], y[:, t])[0] for t in range(y.shape[1])])
    out = {"pred": np.ascontiguousarray(pred.T), "leverage": h, "eloo": np.ascontiguousarray(eloo.T),
           "press": np.sum(eloo * eloo, axis=0), "fitness": fit, "gap": float(np.min(LD(1) - h))}
    if one:
        out.update(pred=out["pred"][0], eloo=out["eloo"][0], press=out["press"][0], fitness=float(fit[0]))
    return out


def loo_brute(idx, train, geno, pheno, h2, branch="auto", which=None):
    """y^_loo of the training animals at positions `which` (None: all) by refitting without each."""
    geno = np.asarray(geno)
    idx = np.asarray(idx, dtype=np.int64)
    T = np.asarray(train)
    y = np.asarray(pheno, dtype=np.float64)
    branch = R._branch(len(idx), geno.shape[0], branch)
    which = range(len(T)) if which is None else which
    out = []
    if branch == "gblup":
        data = geno.astype(np.float64)
        for i in which:
            rest = np.delete(T, i)
            # (two copies of t: the oracle's Pearson needs two values; the prediction is the first)
            out.append(O.gblup(idx, rest, np.array([T[i], T[i]]), data, y, h2, return_ebv=True)[1][0])
        return np.array(out)
    x = geno[:, idx].astype(np.float64)
    p = x[T].mean(axis=0) / 2.0
    d = 2.0 * np.sum(p * (1.0 - p))
    alpha = (1.0 - h2) / h2 * d
    for i in which:
        rest = np.delete(T, i)
        out.append(O._ridge_predict(x[rest], y[rest], x[T[i]:T[i] + 1], alpha)[0])
    return np.array(out)


# ---------------------------------------------------------------------------------------------
# Inputs: tests/reliability_ref.py's panel (331 x 600, with its k = 300 genome) plus one genome of
# k = 40, and its deeper panel (700 x 800, n_T = 520, k = 513).
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def panel():
    pn = dict(Q.panel())
    genomes = dict(pn["genomes"])
    genomes[K40] = np.random.default_rng(40331).choice(R.N_SNPS, K40, replace=False)
    pn["genomes"] = genomes
    return pn


RAGGED = [1, 65, K40, 200, K300, 332, 400, "dup"]      # k = 332, 400 > n: gblup, so a kernel-form batch
SINGLE = [1, K40, 128, 129, K300, "neg"]               # one at a time: the SNP form wherever k fits the train rows
GBLUP_KS = [64, 200]
SNP_KS = [K300, 400]                                    # forced snp at n_T < k <= n and at k > n


def cases():
    """(name, split, genome key, branch) of every comparison of group A on the 331 x 600 panel."""
    out = []
    for s in R.SPLITS:
        for k in dict.fromkeys(RAGGED + SINGLE):
            out.append(("auto-%d-%d-%s" % (s + (k,)), s, k, "auto"))
        for k in GBLUP_KS:
            out.append(("gblup-%d-%d-%s" % (s + (k,)), s, k, "gblup"))
        for k in SNP_KS:
            out.append(("snp-%d-%d-%s" % (s + (k,)), s, k, "snp"))
    return out


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case_ref(name, trait=0):
    """loo_ref of a case of cases() for phenotype column `trait`, computed once (read-only)."""
    pn = panel()
    _, s, k, br = next(c for c in cases() if c[0] == name)
    return _frozen(loo_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["Y"][:, trait], H2, br))


@functools.lru_cache(maxsize=None)
def deep_ref():
    dp = Q.deep_panel()
    return _frozen(loo_ref(dp["genome"], dp["train"], dp["geno"], dp["pheno"], H2, "auto"))
