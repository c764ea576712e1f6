"""Float64 restatement of the reliability of a genomic value (TEST INFRASTRUCTURE ONLY), the wider
computation that bounds its own error, and the inputs shared by tests/test_reliability_host.py (CPU)
and tests/test_gpu_reliability.py (GPU).

With A the gathered columns idx[0..k) (duplicates kept), c = 2p the exact allele count over the
branch's N reference rows (all animals for gblup, the train rows for snp) divided once by N,
d = 2 sum p(1-p), lambda = (1-h2)/h2, w_a = A[a] - c and K = W W^T / d:

  kernel form  rel(a) = k_aT^T (K_TT + lambda I)^-1 k_Ta / K_aa,   k_Ta = W_T w_a / d, K_aa = w_a.w_a / d
  SNP form     rel(a) = 1 - lambda w_a^T (C + lambda I)^-1 w_a / (w_a.w_a),   C = W_T^T W_T / d

(equal by the Woodbury identity), each through a column Cholesky L L^T and one forward substitution:
|L^-1 k_Ta|^2 / K_aa and 1 - lambda |L^-1 w_a|^2 / (w_a.w_a).  The model is the reference's own
(beta ~ N(0, sigma_g^2 / d I), sigma_e^2 / sigma_g^2 = lambda; tblup/evaluator.py:265-314), the snp
branch's intercept taken as known.
"""
import functools

import numpy as np

from oracle import blup_oracle as O
from tests import model_ref as R

LD = np.longdouble
H2 = R.H2


def _chol(A):
    """Column Cholesky in A's precision (tests/model_ref.py::_chol_solve); None if a pivot is not positive."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return None
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def _forward(L, Bm):
    """L^-1 Bm, row by row as _chol_solve's first substitution, every column of Bm at once."""
    Z = np.zeros_like(Bm)
    for i in range(L.shape[0]):
        Z[i] = (Bm[i] - L[i, :i] @ Z[:i]) / L[i, i]
    return Z


def _setup(idx, train, geno, h2, branch, dtype):
    geno = np.asarray(geno)
    idx = np.asarray(idx, dtype=np.int64)
    T = np.asarray(train)
    branch = R._branch(len(idx), geno.shape[0], branch)
    a = geno[:, idx].astype(np.int64)
    ref = np.arange(geno.shape[0]) if branch == "gblup" else T
    N = len(ref)
    m = a[ref].sum(axis=0)
    sm, q = int(m.sum()), int(np.sum(m * m))
    d = dtype(2 * N * sm - q) / dtype(2 * N * N)              # 2 sum p(1-p) from the exact counts
    lam = (dtype(1) - dtype(h2)) / dtype(h2)
    w = a.astype(dtype) - m.astype(dtype) / dtype(N)
    return w, w[T], d, lam


def _rel(idx, train, geno, h2, branch, form, dtype):
    w, wt, d, lam = _setup(idx, train, geno, h2, branch, dtype)
    n, k = w.shape
    nan = np.full(n, np.nan)
    if not d > 0:
        return nan
    if form is None:
        form = "snp" if k <= wt.shape[0] else "kernel"
    ww = np.sum(w * w, axis=1)
    with np.errstate(all="ignore"):
        if form == "snp":
            A = (wt.T @ wt) / d
            A[np.diag_indices_from(A)] += lam
            L = _chol(A)
            if L is None:
                return nan
            v = _forward(L, np.ascontiguousarray(w.T))
            return dtype(1) - lam * np.sum(v * v, axis=0) / ww
        A = (wt @ wt.T) / d
        A[np.diag_indices_from(A)] += lam
        L = _chol(A)
        if L is None:
            return nan
        v = _forward(L, (wt @ w.T) / d)
        return np.sum(v * v, axis=0) / (ww / d)


def rel_ref(idx, train, geno, h2, branch="auto", form=None):
    """Reliabilities of all animals of `geno` in float64; form "snp" / "kernel" (None: the smaller system)."""
    return _rel(idx, train, geno, h2, branch, form, np.float64)


def rel_wide(idx, train, geno, h2, branch="auto", form=None):
    """The same in np.longdouble."""
    return _rel(idx, train, geno, h2, branch, form, LD)


# ---------------------------------------------------------------------------------------------
# Inputs: tests/model_ref.py's panel (331 x 600) plus one genome of k = 300 (with split (257, 70)
# it is auto/snp in the SNP form with 3 tile columns), and a deeper synthetic panel -- n = 700,
# P = 800, n_T = 520, n_V = 60, k = 513: 5 tile columns in the SNP form, 5 in the kernel form.
# ---------------------------------------------------------------------------------------------
K300 = 300
A_KEYS = R.KS + ["dup", "neg", K300]
DEEP_N, DEEP_P, DEEP_NT, DEEP_NV, DEEP_K = 700, 800, 520, 60, 513


@functools.lru_cache(maxsize=None)
def panel():
    pn = dict(R.panel())
    genomes = dict(pn["genomes"])
    genomes[K300] = np.random.default_rng(300331).choice(R.N_SNPS, K300, replace=False)
    pn["genomes"] = genomes
    return pn


@functools.lru_cache(maxsize=None)
def deep_panel():
    rng = np.random.default_rng(700800)
    geno = O.synth_geno(rng, DEEP_N, DEEP_P)
    pheno = rng.standard_normal(DEEP_N)
    perm = rng.permutation(DEEP_N)
    return {"geno": geno, "pheno": pheno, "train": perm[:DEEP_NT].copy(),
            "valid": perm[DEEP_NT:DEEP_NT + DEEP_NV].copy(), "genome": rng.choice(DEEP_P, DEEP_K, replace=False)}


def cases():
    """(name, split, genome key, branch) of every comparison of group A on the 331 x 600 panel."""
    out = []
    for s in R.SPLITS:
        for k in A_KEYS:
            out.append(("auto-%d-%d-%s" % (s + (k,)), s, k, "auto"))
        for k in A_KEYS:                      # forced snp where Ridge takes its kernel solve
            if not isinstance(k, str) and k > s[0]:
                out.append(("snp-%d-%d-%s" % (s + (k,)), s, k, "snp"))
    for s in R.FORCED_SPLITS:
        for k in R.GBLUP_KS:
            out.append(("gblup-%d-%d-%s" % (s + (k,)), s, k, "gblup"))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """rel_ref of a case of cases() over all 331 animals, computed once (read-only)."""
    pn = panel()
    _, s, k, br = next(c for c in cases() if c[0] == name)
    r = rel_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], H2, br)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def deep_ref():
    dp = deep_panel()
    r = rel_ref(dp["genome"], dp["train"], dp["geno"], H2, "auto")
    r.setflags(write=False)
    return r
