"""Float64 restatement of the model the reference fits inside blup() (TEST INFRASTRUCTURE ONLY;
oracle/ is frozen, so it lives here), the wider solve that bounds its own error, and the inputs
shared by tests/test_model_host.py (CPU) and tests/test_gpu_model.py (GPU).

  snp    tblup/evaluator.py:288-314: p over the train rows, X -= 2p, Ridge(alpha = lambda d).  The
         restatement follows oracle.blup_oracle._ridge_predict's two solves (scikit-learn 1.7.2
         _solve_cholesky when k <= n_T, else _solve_cholesky_kernel) and returns Ridge's coef_ and
         intercept_ instead of its predictions.
  gblup  tblup/evaluator.py:265-286 with tblup/utils.py:7-18: G = W W^T / d, W = A - 2p over all
         animals; prediction = G[:, T] (G_TT + lambda I)^-1 y_T = W (W_T^T alpha / d), so
         effects = W_T^T alpha / d, intercept 0.

Both are pinned against the reference's own numbers by tests/golden/model.npz
(tests/golden/make_model_golden.py, tests/test_model_host.py).
"""
import functools

import numpy as np
import scipy.linalg

from oracle import blup_oracle as O

LD = np.longdouble
H2 = 0.4


def _branch(k, n, branch):
    return branch if branch != "auto" else ("gblup" if k > n else "snp")


def fit_ref(idx, train, geno, pheno, h2, branch="auto"):
    """{center (k,), effects (k,), intercept, branch} of one phenotype vector in float64."""
    geno = np.asarray(geno)
    idx = np.asarray(idx, dtype=np.int64)
    T = np.asarray(train)
    y = np.asarray(pheno, dtype=np.float64)
    branch = _branch(len(idx), geno.shape[0], branch)
    x = geno[:, idx].astype(np.float64)
    with np.errstate(all="ignore"):
        if branch == "snp":
            x_t = x[T]
            p = x_t.mean(axis=0) / 2.0
            d = 2.0 * np.sum(p * (1.0 - p))
            alpha = (1.0 - h2) / (h2 / d)
            x_t = x_t - 2.0 * p
            # Ridge(alpha).fit(x_t, y_T), as _ridge_predict
            x_off, y_off = x_t.mean(axis=0), y[T].mean()
            xc, yc = x_t - x_off, y[T] - y_off
            n_s, n_f = xc.shape
            try:
                if n_f > n_s:
                    K = xc @ xc.T
                    K.flat[:: n_s + 1] += alpha
                    coef = xc.T @ scipy.linalg.solve(K, yc, assume_a="pos")
                else:
                    A = xc.T @ xc
                    A.flat[:: n_f + 1] += alpha
                    coef = scipy.linalg.solve(A, xc.T @ yc, assume_a="pos")
            except (np.linalg.LinAlgError, ValueError):
                coef = np.full(n_f, np.nan)
            return {"center": 2.0 * p, "effects": coef, "intercept": float(y_off - x_off @ coef), "branch": branch}
        p = x.mean(axis=0) / 2.0
        d = 2.0 * np.sum(p * (1.0 - p))
        w = x - 2.0 * p
        A = (w[T] @ w[T].T) / d
        A.flat[:: len(T) + 1] += (1.0 - h2) / h2
        try:
            al = scipy.linalg.solve(A, y[T], assume_a="pos")
        except (np.linalg.LinAlgError, ValueError):
            al = np.full(len(T), np.nan)
        return {"center": 2.0 * p, "effects": (w[T].T @ al) / d, "intercept": 0.0, "branch": branch}


def gblup_all_ref(idx, train, geno, pheno, h2):
    """The all-animal `prediction` of evaluator.py:284 from the restated gblup model."""
    m = fit_ref(idx, train, geno, pheno, h2, "gblup")
    return (np.asarray(geno)[:, np.asarray(idx)].astype(np.float64) - m["center"]) @ m["effects"] + m["intercept"]


def _chol_solve(A, b):
    """A x = b for SPD A in A's precision (column Cholesky, two substitutions); None if a pivot
    is not positive.  As tests/test_edge_cases_cpu.py."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return None
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    z = np.zeros_like(b)
    for i in range(n):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (z[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def fit_wide(idx, train, geno, pheno, h2, branch="auto"):
    """The same model from exact integer counts centred in np.longdouble and a longdouble
    Cholesky (tests/test_edge_cases_cpu.py's wider solve, returning the effects): effects (k,)
    in longdouble -- (k, t) for an (n, t) phenotype matrix, one factor for every column -- or None
    when the system is not positive definite (d = 0)."""
    geno = np.asarray(geno)
    idx = np.asarray(idx, dtype=np.int64)
    T = np.asarray(train)
    branch = _branch(len(idx), geno.shape[0], branch)
    a = geno[:, idx].astype(np.float64)
    ref = np.arange(geno.shape[0]) if branch == "gblup" else T
    N = len(ref)
    m = a[ref].sum(axis=0).astype(np.int64)
    sm, q = int(m.sum()), int(np.sum(m * m))
    d = LD(2 * N * sm - q) / LD(2 * N * N)
    if not d > 0:
        return None
    y = np.asarray(pheno, dtype=np.float64).astype(LD)
    yc = y[T] - (LD(0) if branch == "gblup" else y[T].mean(axis=0))
    alpha = (LD(1) - LD(h2)) / LD(h2) * d
    wt = a[T].astype(LD) - m.astype(LD) / LD(N)
    if branch == "snp" and len(idx) <= len(T):
        S = N * (a[T].T @ a[T]).astype(np.int64) - np.outer(m, m)      # N W^T W, exact
        A = S.astype(LD) / LD(N)
        A[np.diag_indices_from(A)] += alpha
        return _chol_solve(A, wt.T @ yc)
    u = (a @ m.astype(np.float64)).astype(np.int64)
    M = (N * N) * (a[T] @ a[T].T).astype(np.int64) - N * (u[T][:, None] + u[T][None, :]) + q   # N^2 W_T W_T^T
    A = M.astype(LD) / LD(N * N)
    A[np.diag_indices_from(A)] += alpha
    w = _chol_solve(A, yc)      # (W W^T + lambda d I) w = yc: w = alpha / d
    return None if w is None else wt.T @ w


# ---------------------------------------------------------------------------------------------
# The panel and cases of tests/test_gpu_model.py: n = 331 animals (odd: the SNP-major rows are
# unaligned), P = 600, four phenotype columns (column 0 is the single-trait phenotype).
# ---------------------------------------------------------------------------------------------
N_ANIMALS, N_SNPS = 331, 600
SPLITS = [(127, 5), (128, 2), (129, 64), (257, 70)]
KS = [1, 2, 63, 64, 65, 127, 128, 129, 200, 332, 400]
FORCED_SPLITS = [(127, 5), (257, 70)]
GBLUP_KS = [1, 64, 65, 129, 200]      # forced gblup at k <= n


@functools.lru_cache(maxsize=None)
def panel():
    rng = np.random.default_rng(331600)
    geno = O.synth_geno(rng, N_ANIMALS, N_SNPS)
    Y = rng.standard_normal((N_ANIMALS, 4))
    splits = {}
    for nT, nV in SPLITS:
        perm = rng.permutation(N_ANIMALS)
        splits[nT, nV] = (perm[:nT].copy(), perm[nT:nT + nV].copy())
    genomes = {k: (rng.choice(N_SNPS, k, replace=False) if k <= N_SNPS else rng.integers(0, N_SNPS, k)) for k in KS}
    dup = rng.choice(N_SNPS, 100, replace=False)
    dup[50:60] = dup[:10]                        # duplicates: each occurrence its own column
    neg = rng.choice(N_SNPS, 90, replace=False).astype(np.int64)
    neg[::3] -= N_SNPS                           # negative indices wrap
    genomes["dup"], genomes["neg"] = dup, neg
    return {"geno": geno, "Y": Y, "pheno": np.ascontiguousarray(Y[:, 0]), "splits": splits, "genomes": genomes}


def effect_cases():
    """(name, split, genome key, branch) of every single-trait effects comparison of group A."""
    out = []
    for s in SPLITS:
        for k in KS + ["dup", "neg"]:
            out.append(("auto-%d-%d-%s" % (s + (k,)), s, k, "auto"))
        # forced snp: n_T < k <= n is auto's own branch (above; sklearn's dual solve); here k > n
        for k in (332, 400):
            out.append(("snp-%d-%d-%s" % (s + (k,)), s, k, "snp"))
    for s in FORCED_SPLITS:
        for k in GBLUP_KS:
            out.append(("gblup-%d-%d-%s" % (s + (k,)), s, k, "gblup"))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """fit_ref of a case of effect_cases(), computed once."""
    pn = panel()
    _, s, k, br = next(c for c in effect_cases() if c[0] == name)
    return fit_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], H2, br)


@functools.lru_cache(maxsize=None)
def ebv_all_ref(s, k, branch="auto"):
    """The oracle's EBV of every animal of the panel (valid = all animals), computed once."""
    pn = panel()
    fn = {"auto": O.blup, "gblup": O.gblup, "snp": O.snp_blup}[branch]
    _, e = fn(pn["genomes"][k], pn["splits"][s][0], np.arange(N_ANIMALS), pn["geno"].astype(np.float64), pn["pheno"],
              H2, return_ebv=True)
    e.setflags(write=False)
    return e
