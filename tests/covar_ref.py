"""Dense float64 restatement of the fitted model with fixed-effect covariates (TEST INFRASTRUCTURE ONLY),
the wider computation that bounds its own error, an independent route through Henderson's mixed-model
equations, and the inputs shared by tests/test_covar_host.py (CPU) and tests/test_gpu_covar.py (GPU).

The model is tests/score_ref.py's: A the gathered columns idx[0..k) (duplicates kept), c the branch's centre
(all n animals for gblup, the train rows for snp), d = 2 sum p(1-p), lambda = (1-h2)/h2, W_T = A_T - c,
V = W_T W_T^T / d + lambda I, r_t = y_T,t - mu_t (mu = 0 for gblup, mean(y_T) for snp).  With Q (n x c) the
covariates, m their column means over the train rows under snp and 0 under gblup, Q~ = Q - m:

  b_t = (Q~_T^T V^-1 Q~_T)^-1 Q~_T^T V^-1 r_t,     y*_t = y_t - Q~ b_t   (every animal)

V is built explicitly; ebv and fitness are then oracle/blup_oracle's own blup of y* (the reference-pinned
oracle), effects / center / intercept tests/model_ref.py::fit_ref's of y*.
"""
import functools

import numpy as np

from oracle import blup_oracle as O
from tests import model_ref as R
from tests import reliability_ref as RQ
from tests import score_ref as S

LD = np.longdouble
H2 = R.H2
TOL = S.TOL                      # the GPU tests' bound: |got - ref| <= TOL max(1, max |ref|)
HOST_TOL = S.HOST_TOL            # float64 against longdouble, relative to the largest |ref|
COND_MAX = 1e6                   # cond(Q~^T V^-1 Q~) of every case: the inputs keep TOL meaningful
MAX_COV = 16
close = S.close
panel = RQ.panel
deep_panel = RQ.deep_panel


def make_cov(n, c, ones=False, seed=0):
    """(n, c) covariates from a fixed draw: a column of ones first when `ones` (gblup cases: the way to fit
    a mean there), then one 0/1 column when two or more columns remain, the rest standard normal."""
    rng = np.random.default_rng(7700 + 100 * c + seed)
    cols = [np.ones(n)] if ones else []
    if c - len(cols) >= 2:
        cols.append((rng.random(n) < 0.5).astype(np.float64))
    while len(cols) < c:
        cols.append(rng.standard_normal(n))
    return np.ascontiguousarray(np.stack(cols, axis=1))


PIV_RTOL = 1e-12                 # a pivot of G counts as positive above this fraction of its diagonal entry


def _chol_solve_mat(A, Bm):
    """A X = Bm through a column Cholesky (tests/reliability_ref.py::_chol's) and substitutions; None if a
    pivot is not positive -- above PIV_RTOL of its diagonal entry, the library's rule: an exactly repeated
    column leaves rounding noise of either sign -- and finite."""
    n = A.shape[0]
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(n):
            v = A[j:, j] - L[j:, :j] @ L[j, :j]
            if not (v[0] > PIV_RTOL * A[j, j] and np.isfinite(v[0])):
                return None
            L[j, j] = np.sqrt(v[0])
            L[j + 1:, j] = v[1:] / L[j, j]
    Z = RQ._forward(L, Bm)
    X = np.zeros_like(Z)
    for i in range(A.shape[0] - 1, -1, -1):
        X[i] = (Z[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def _gls(idx, train, geno, pheno, cov, h2, branch, dtype):
    """{b (nt, c), m (c,), ystar (n, nt), G (c, c)} in `dtype`, b / ystar NaN for a degenerate model."""
    geno = np.asarray(geno)
    T = np.asarray(train)
    _, wt, d, lam = RQ._setup(idx, train, geno, h2, branch, dtype)
    br = R._branch(len(np.asarray(idx)), geno.shape[0], branch)
    Y = np.asarray(pheno, dtype=np.float64)
    Y = (Y[:, None] if Y.ndim == 1 else Y).astype(dtype)
    Qd = np.asarray(cov, dtype=np.float64)
    Qd = (Qd[:, None] if Qd.ndim == 1 else Qd).astype(dtype)
    nT, c, nt = len(T), Qd.shape[1], Y.shape[1]
    m = Qd[T].sum(axis=0) / dtype(nT) if br == "snp" else np.zeros(c, dtype=dtype)
    Qc = Qd - m
    r = Y[T] - (Y[T].sum(axis=0) / dtype(nT) if br == "snp" else dtype(0))
    bad = {"b": np.full((nt, c), np.nan), "m": m, "ystar": np.full(Y.shape, np.nan), "G": np.full((c, c), np.nan),
           "branch": br}
    if not d > 0:
        return bad
    V = (wt @ wt.T) / d
    V[np.diag_indices_from(V)] += lam
    L = RQ._chol(V)
    if L is None:
        return bad
    Sm, z = RQ._forward(L, np.ascontiguousarray(Qc[T])), RQ._forward(L, np.ascontiguousarray(r))
    G = Sm.T @ Sm
    b = _chol_solve_mat(G, Sm.T @ z)                    # (c, nt)
    if b is None:
        return dict(bad, G=G)
    return {"b": np.ascontiguousarray(b.T), "m": m, "ystar": Y - Qc @ b, "G": G, "branch": br}


def gls_ref(idx, train, geno, pheno, cov, h2, branch="auto"):
    return _gls(idx, train, geno, pheno, cov, h2, branch, np.float64)


def gls_wide(idx, train, geno, pheno, cov, h2, branch="auto"):
    """The same in np.longdouble."""
    return _gls(idx, train, geno, pheno, cov, h2, branch, LD)


def cov_ref(idx, train, valid, geno, pheno, cov, h2, branch="auto"):
    """Everything tblup_fit_cov_batch returns for one model, in float64: cov_effects (nt, c), cov_center
    (c,), ystar (n, nt), ebv (nt, n_V) and fitness from the oracle's blup of y*, effects (nt, k), center (k,)
    and intercept (nt,) from fit_ref of y*, cond of G."""
    geno = np.asarray(geno)
    g = gls_ref(idx, train, geno, pheno, cov, h2, branch)
    nt = g["b"].shape[0]
    k = len(np.asarray(idx))
    out = {"cov_effects": g["b"], "cov_center": g["m"], "ystar": g["ystar"], "branch": g["branch"]}
    with np.errstate(all="ignore"):
        out["cond"] = float(np.linalg.cond(g["G"])) if np.all(np.isfinite(g["G"])) else np.inf
    if not np.all(np.isfinite(g["b"])):
        out.update(ebv=np.full((nt, len(valid)), np.nan), fitness=np.nan, effects=np.full((nt, k), np.nan),
                   center=np.full(k, np.nan), intercept=np.full(nt, np.nan), cov_center=np.full(len(g["m"]), np.nan))
        return out
    fn = {"auto": O.blup, "gblup": O.gblup, "snp": O.snp_blup}[branch]
    gf = geno.astype(np.float64)
    ebv, fits, eff, icpt, cen = [], [], [], [], None
    for t in range(nt):
        ys = np.ascontiguousarray(g["ystar"][:, t])
        f, e = fn(np.asarray(idx), train, valid, gf, ys, h2, return_ebv=True)
        fm = R.fit_ref(idx, train, geno, ys, h2, branch)
        ebv.append(e)
        fits.append(f)
        eff.append(fm["effects"])
        icpt.append(fm["intercept"])
        cen = fm["center"]
    out.update(ebv=np.array(ebv), fitness=float(np.mean(fits)), effects=np.array(eff), center=cen,
               intercept=np.array(icpt))
    return out


def mme_ref(idx, train, geno, pheno, cov, h2, branch="auto"):
    """Henderson's mixed-model equations on [1, Q~_T, W_T] (no column of ones under gblup, whose model has no
    mean), solved densely: (b (nt, c), snp effects (nt, k)) out of one system -- no V, no GLS step."""
    geno = np.asarray(geno)
    T = np.asarray(train)
    _, wt, d, lam = RQ._setup(idx, train, geno, h2, branch, np.float64)
    br = R._branch(len(np.asarray(idx)), geno.shape[0], branch)
    Y = np.asarray(pheno, dtype=np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    Qd = np.asarray(cov, dtype=np.float64)
    Qd = Qd[:, None] if Qd.ndim == 1 else Qd
    c = Qd.shape[1]
    Qc = Qd[T] - (Qd[T].mean(axis=0) if br == "snp" else 0.0)
    X = np.hstack([np.ones((len(T), 1)), Qc]) if br == "snp" else Qc
    Z = np.hstack([X, wt])
    A = Z.T @ Z
    nx = X.shape[1]
    A[np.arange(nx, A.shape[0]), np.arange(nx, A.shape[0])] += lam * d
    sol = np.linalg.solve(A, Z.T @ Y[T])
    return np.ascontiguousarray(sol[nx - c:nx].T), np.ascontiguousarray(sol[nx:].T)


# ---------------------------------------------------------------------------------------------
# Cases: (name, panel, split, genome key, branch, c).  The 331 x 600 panel of tests/reliability_ref.py with its
# four splits -- the covariate count goes round 1, 5, 16 with the split -- and the deeper 700 x 800 panel.
# Auto-branch genomes are evaluated by the GPU test as one ragged batch (kernel form) and, where k <= n_T,
# alone (SNP form), against the same reference.
# ---------------------------------------------------------------------------------------------
AUTO_KEYS = [1, 64, 65, 127, 129, 200, "dup", "neg", RQ.K300, 332]
SPLIT_COV = {(127, 5): 5, (128, 2): 1, (129, 64): 16, (257, 70): 5}
GBLUP_COV = {(127, 5): 16, (257, 70): 1}
DEEP_COV = 16


def cases():
    out = []
    for s in R.SPLITS:
        for k in AUTO_KEYS:
            out.append(("auto-%d-%d-%s" % (s + (k,)), "std", s, k, "auto", SPLIT_COV[s]))
        for k in (200, 332, 400):                       # forced snp at n_T < k <= n and k > n
            if k > s[0]:
                out.append(("snp-%d-%d-%s" % (s + (k,)), "std", s, k, "snp", SPLIT_COV[s]))
    for s in R.FORCED_SPLITS:
        for k in R.GBLUP_KS:
            out.append(("gblup-%d-%d-%s" % (s + (k,)), "std", s, k, "gblup", GBLUP_COV[s]))
    out.append(("deep", "deep", None, None, "auto", DEEP_COV))
    return out


def case_inputs(name):
    """(idx, train, valid, geno, pheno, cov, branch) of a case."""
    _, pnl, s, k, br, c = next(x for x in cases() if x[0] == name)
    if pnl == "deep":
        dp = deep_panel()
        return dp["genome"], dp["train"], dp["valid"], dp["geno"], dp["pheno"], make_cov(RQ.DEEP_N, c), br
    pn = panel()
    T, V = pn["splits"][s]
    return pn["genomes"][k], T, V, pn["geno"], pn["pheno"], make_cov(R.N_ANIMALS, c, ones=(br == "gblup")), br


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """cov_ref of a case, computed once (read-only)."""
    idx, T, V, geno, pheno, cov, br = case_inputs(name)
    out = cov_ref(idx, T, V, geno, pheno, cov, H2, br)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
