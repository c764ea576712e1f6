"""Float64 restatement of the profile (restricted) log-likelihood of h2 (TEST INFRASTRUCTURE ONLY), the
wider computation that bounds its own error, the estimate_h2 procedure on the restatement's own values,
and the inputs shared by tests/test_loglik_host.py (CPU) and tests/test_gpu_loglik.py (GPU).

Only the dense N x N definition is used, for both branches (numpy's slogdet and solve), so that the
library's SNP-form identities (Sylvester, Woodbury) are tested, not restated.  With N = n_T, A the
gathered columns idx[0..k) (duplicates kept), c = 2p the exact allele count over the branch's reference
rows (all animals for gblup, the train rows for snp) divided once by their number, d = 2 sum p(1-p),
lambda = (1-h2)/h2, W_T = A_T - c, V = W_T W_T^T / d + lambda I, sigma2_g profiled out:

  gblup  no mean fitted (r = 0):  q = y_T^T V^-1 y_T
  snp    intercept mean(y_T) (r = 1):  q = yc^T V^-1 yc, yc = y_T - mean(y_T); the restricted likelihood
         of the N - 1 error contrasts, log|A^T V A| = log|V| - log lambda since V 1 = lambda 1
  l = -1/2 [ (N - r)(log 2pi + 1 + log(q / (N - r))) + log|V| - r log lambda ],  sigma2_g = q / (N - r)
"""
import functools

import numpy as np

from tests import model_ref as R
from tests import reliability_ref as Q

LD = np.longdouble
H2S = (0.05, 0.3, 0.6, 0.9)
TOL = 1e-9                       # the GPU tests' bound: |got - ref| <= TOL max(1, |ref|)
K300 = Q.K300
A_KEYS = Q.A_KEYS


def _inputs(idx, train, geno, pheno, h2, branch, dtype):
    w, wt, d, lam = Q._setup(idx, train, geno, h2, branch, dtype)
    branch = R._branch(len(np.asarray(idx)), np.asarray(geno).shape[0], branch)
    y = np.asarray(pheno, dtype=np.float64)
    y = (y[:, None] if y.ndim == 1 else y)[np.asarray(train)].astype(dtype)
    r = 1 if branch == "snp" else 0
    if r:
        y = y - y.sum(axis=0) / dtype(len(y))
    return wt, d, lam, y, r


def _combine(N, r, q, logdet, lam, dtype):
    df = dtype(N - r)
    with np.errstate(all="ignore"):
        two_pi = 8 * np.arctan(dtype(1))      # pi in dtype's own precision
        l = -(df * (np.log(two_pi) + 1 + np.log(q / df)) + logdet - r * np.log(lam)) / 2
    bad = ~(q > 0) | ~np.isfinite(q)
    return np.where(bad, np.nan, l), np.where(bad, np.nan, q / df)


def loglik_ref(idx, train, geno, pheno, h2, branch="auto"):
    """(loglik, sigma2_g), one value per phenotype column (scalars for a 1-D phenotype), in float64 from
    the dense V: slogdet and solve."""
    wt, d, lam, y, r = _inputs(idx, train, geno, pheno, h2, branch, np.float64)
    nt = y.shape[1]
    scalar = np.asarray(pheno).ndim == 1
    if not d > 0:
        out = np.full(nt, np.nan), np.full(nt, np.nan)
    else:
        N = wt.shape[0]
        V = (wt @ wt.T) / d
        V[np.diag_indices_from(V)] += lam
        sign, logdet = np.linalg.slogdet(V)
        assert sign > 0
        q = np.sum(y * np.linalg.solve(V, y), axis=0)
        out = _combine(N, r, q, logdet, lam, np.float64)
    return (float(out[0][0]), float(out[1][0])) if scalar else out


def loglik_wide(idx, train, geno, pheno, h2, branch="auto"):
    """The same quantities in np.longdouble: V from the exact integer N^2 W_T W_T^T (as
    tests/model_ref.py::fit_wide), a column Cholesky, log|V| = 2 sum log L_ii, q = |L^-1 y|^2."""
    geno, idx, T = np.asarray(geno), np.asarray(idx, dtype=np.int64), np.asarray(train)
    br = R._branch(len(idx), geno.shape[0], branch)
    a = geno[:, idx].astype(np.int64)
    ref = np.arange(geno.shape[0]) if br == "gblup" else T
    N = len(ref)
    m = a[ref].sum(axis=0)
    sm, qq = int(m.sum()), int(np.sum(m * m))
    d = LD(2 * N * sm - qq) / LD(2 * N * N)
    lam = (LD(1) - LD(h2)) / LD(h2)
    y = np.asarray(pheno, dtype=np.float64)
    y = (y[:, None] if y.ndim == 1 else y)[T].astype(LD)
    r = 1 if br == "snp" else 0
    if r:
        y = y - y.sum(axis=0) / LD(len(y))
    nt = y.shape[1]
    scalar = np.asarray(pheno).ndim == 1
    out = np.full(nt, np.nan, dtype=LD), np.full(nt, np.nan, dtype=LD)
    if d > 0:
        u = a[T] @ m
        M = (N * N) * (a[T] @ a[T].T) - N * (u[:, None] + u[None, :]) + qq      # N^2 W_T W_T^T, exact
        V = M.astype(LD) / (LD(N * N) * d)
        V[np.diag_indices_from(V)] += lam
        L = Q._chol(V)
        if L is not None:
            z = Q._forward(L, y)
            out = _combine(len(T), r, np.sum(z * z, axis=0), 2 * np.sum(np.log(np.diag(L))), lam, LD)
    return (out[0][0], out[1][0]) if scalar else out


def loglik_contrast(idx, train, geno, pheno, h2):
    """The snp branch's restricted likelihood as it is defined: the profile likelihood of the N - 1
    error contrasts A^T y_T, A an orthonormal basis of the complement of 1 (from an SVD of the centring
    matrix), with covariance sigma2_g A^T V A.  One phenotype vector."""
    w, wt, d, lam = Q._setup(idx, train, geno, h2, "snp", np.float64)
    N = wt.shape[0]
    V = (wt @ wt.T) / d
    V[np.diag_indices_from(V)] += lam
    U, s, _ = np.linalg.svd(np.eye(N) - np.full((N, N), 1.0 / N))
    A = U[:, :N - 1]
    assert s[N - 2] > 0.5 and s[N - 1] < 1e-10
    yc = A.T @ np.asarray(pheno, dtype=np.float64)[np.asarray(train)]
    Vc = A.T @ V @ A
    sign, logdet = np.linalg.slogdet(Vc)
    q = yc @ np.linalg.solve(Vc, yc)
    return -0.5 * ((N - 1) * (np.log(2 * np.pi) + 1 + np.log(q / (N - 1))) + logdet), q / (N - 1)


def estimate_ref(idx, train, geno, pheno, branch="auto", grid=np.linspace(0.02, 0.98, 25), refine=3, points=9):
    """GpuBlupEngine.estimate_h2's procedure for one model and one phenotype vector on loglik_ref's
    values: the grid, then `refine` rounds of `points` evenly spaced values between the neighbours of
    the current (first) argmax; the best point seen."""
    def ev(hs):
        out = [loglik_ref(idx, train, geno, pheno, float(h), branch) for h in hs]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])

    grid = np.asarray(grid, dtype=np.float64)
    h = grid
    best = None
    for rnd in range(refine + 1):
        ll, s2 = ev(h)
        if np.all(np.isnan(ll)):
            return {"h2": np.nan, "loglik": np.nan, "sigma2_g": np.nan, "at_bound": False, "step": np.nan}
        i = int(np.argmax(np.where(np.isnan(ll), -np.inf, ll)))
        if best is None or ll[i] > best[1]:
            best = (h[i], ll[i], s2[i])
        step = h[1] - h[0]
        if rnd == refine:
            break
        h = np.linspace(h[max(i - 1, 0)], h[min(i + 1, len(h) - 1)], points)
    return {"h2": float(best[0]), "loglik": float(best[1]), "sigma2_g": float(best[2]),
            "at_bound": bool(best[0] == grid[0] or best[0] == grid[-1]), "step": float(step)}


# ---------------------------------------------------------------------------------------------
# Inputs: tests/reliability_ref.py's panels, splits, genomes and cases; every case at every h2 of H2S.
# ---------------------------------------------------------------------------------------------
panel = Q.panel
deep_panel = Q.deep_panel
cases = Q.cases


@functools.lru_cache(maxsize=None)
def case_ref(name, h2):
    """loglik_ref (loglik, sigma2_g) of a case of cases() at h2 on the single-trait phenotype, once."""
    pn = panel()
    _, s, k, br = next(c for c in cases() if c[0] == name)
    return loglik_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], h2, br)


@functools.lru_cache(maxsize=None)
def deep_ref(h2):
    dp = deep_panel()
    return loglik_ref(dp["genome"], dp["train"], dp["geno"], dp["pheno"], h2, "auto")


def close(got, ref):
    """The tolerance of the GPU tests: |got - ref| / max(1, |ref|), elementwise maximum."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
