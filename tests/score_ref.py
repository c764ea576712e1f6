"""Float64 restatement of the mixed-model score statistics of SNPs (TEST INFRASTRUCTURE ONLY), the wider
computation that bounds its own error, and the inputs shared by tests/test_score_host.py (CPU) and
tests/test_gpu_score.py (GPU).

The model is tests/reliability_ref.py's and tests/loglik_ref.py's.  With A the gathered columns idx[0..k)
(duplicates kept), c the exact allele count over the branch's N reference rows (all animals for gblup, the
train rows for snp) divided once by N, d = 2 sum p(1-p), lambda = (1-h2)/h2, W_T = A_T - c,
V = W_T W_T^T / d + lambda I, r_t = y_T,t - mu_t (mu = 0 for gblup, mean(y_T) for snp), and for a listed
column j of the panel w_j = x_T,j - c_j with the same centring rule:

  u[t][j] = w_j^T V^-1 r_t,   v[j] = w_j^T V^-1 w_j,   q[t] = r_t^T V^-1 r_t

each through a column Cholesky M = L L^T and one forward substitution, in either form:

  kernel form (M = V)                       s_j = L^-1 w_j, z = L^-1 r:  u = s_j.z, v = s_j.s_j, q = |z|^2
  SNP form (M = W_T^T W_T / d + lambda I_k) s_j = L^-1 W_T^T w_j, z = L^-1 W_T^T r / d:
      u = (w_j.r - s_j.z) / lambda,  v = (w_j.w_j - s_j.s_j / d) / lambda,  q = (r.r - d |z|^2) / lambda
"""
import functools

import numpy as np

from tests import model_ref as R
from tests import reliability_ref as Q

LD = np.longdouble
H2 = R.H2
TOL = 1e-9                       # the GPU tests' bound: |got - ref| <= TOL max(1, max |ref|)
HOST_TOL = 1e-11                 # float64 against longdouble, relative to the largest |ref|
K300 = Q.K300
A_KEYS = Q.A_KEYS
LIST_LENGTHS = (1, 15, 16, 17, 33, 65)


def wrap(snps, P):
    s = np.asarray(snps, dtype=np.int64)
    return np.where(s < 0, s + P, s)


def _score(idx, train, geno, pheno, h2, branch, snps, form, dtype):
    geno = np.asarray(geno)
    T = np.asarray(train)
    _, wt, d, lam = Q._setup(idx, train, geno, h2, branch, dtype)
    br = R._branch(len(np.asarray(idx)), geno.shape[0], branch)
    cand = wrap(np.arange(geno.shape[1]) if snps is None else snps, geno.shape[1])
    x = geno[:, cand].astype(np.int64)
    ref = np.arange(geno.shape[0]) if br == "gblup" else T
    wc = x[T].astype(dtype) - x[ref].sum(axis=0).astype(dtype) / dtype(len(ref))      # (n_T, m)
    y = np.asarray(pheno, dtype=np.float64)
    y = (y[:, None] if y.ndim == 1 else y)[T].astype(dtype)
    if br == "snp":
        y = y - y.sum(axis=0) / dtype(len(y))
    nt, m = y.shape[1], len(cand)
    nan = np.full((nt, m), np.nan), np.full(m, np.nan), np.full(nt, np.nan)
    if not d > 0:
        return nan
    nT, k = wt.shape
    if form is None:
        form = "snp" if (br == "snp" and k <= nT) else "kernel"
    if form == "kernel":
        A = (wt @ wt.T) / d
        A[np.diag_indices_from(A)] += lam
        L = Q._chol(A)
        if L is None:
            return nan
        s, z = Q._forward(L, wc), Q._forward(L, y)
        return z.T @ s, np.sum(s * s, axis=0), np.sum(z * z, axis=0)
    A = (wt.T @ wt) / d
    A[np.diag_indices_from(A)] += lam
    L = Q._chol(A)
    if L is None:
        return nan
    s, z = Q._forward(L, wt.T @ wc), Q._forward(L, (wt.T @ y) / d)
    return ((y.T @ wc - z.T @ s) / lam, (np.sum(wc * wc, axis=0) - np.sum(s * s, axis=0) / d) / lam,
            (np.sum(y * y, axis=0) - d * np.sum(z * z, axis=0)) / lam)


def score_ref(idx, train, geno, pheno, h2, branch="auto", snps=None, form=None):
    """(u (nt, m), v (m,), q (nt,)) in float64 for the listed columns (None: all); form "snp" / "kernel"
    (None: the form the library takes for the model alone)."""
    return _score(idx, train, geno, pheno, h2, branch, snps, form, np.float64)


def score_wide(idx, train, geno, pheno, h2, branch="auto", snps=None, form=None):
    """The same in np.longdouble."""
    return _score(idx, train, geno, pheno, h2, branch, snps, form, LD)


def dof(idx, train, geno, branch="auto"):
    """N - r: the train animals, minus the snp branch's fitted intercept."""
    return len(train) - (1 if R._branch(len(np.asarray(idx)), np.asarray(geno).shape[0], branch) == "snp" else 0)


def d_of_center(center):
    """d = 2 sum p(1-p) from a model's centre c = 2p."""
    c = np.asarray(center, dtype=np.float64)
    return float(np.sum(c * (1.0 - c / 2.0)))


def close(got, ref):
    """The GPU tests' measure: max |got - ref| / max(1, max |ref|) over the array."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref)))))


# ---------------------------------------------------------------------------------------------
# Inputs: tests/reliability_ref.py's panels, splits, genomes and cases; the candidate lists.
# ---------------------------------------------------------------------------------------------
panel = Q.panel
deep_panel = Q.deep_panel
cases = Q.cases


def cand_list(genome, P, m, seed=0):
    """m columns: in-panel and out-of-panel columns alternating from a fixed draw, every third index
    negative (it wraps), and from m = 3 on the last entry repeats the first."""
    rng = np.random.default_rng(1000 * m + seed)
    inside = np.unique(wrap(genome, P))
    outside = np.setdiff1d(np.arange(P), inside)
    a = rng.permutation(inside)
    b = rng.permutation(outside) if len(outside) else a
    out = np.array([(a if i % 2 == 0 else b)[(i // 2) % len(a if i % 2 == 0 else b)] for i in range(m)], dtype=np.int64)
    out[::3] -= P
    if m >= 3:
        out[-1] = out[0]
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """score_ref (u, v, q) of a case of cases() over all 600 columns, single-trait phenotype, once (read-only)."""
    pn = panel()
    _, s, k, br = next(c for c in cases() if c[0] == name)
    out = score_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], H2, br)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def deep_ref():
    dp = deep_panel()
    out = score_ref(dp["genome"], dp["train"], dp["geno"], dp["pheno"], H2, "auto")
    for a in out:
        a.setflags(write=False)
    return out
