"""Dense float64 restatement of the score statistics and the restricted likelihood of h2 with fixed-effect
covariates (TEST INFRASTRUCTURE ONLY), the wider computation that bounds its own error, two independent
routes, and the inputs shared by tests/test_score_cov_host.py (CPU) and tests/test_gpu_score_cov.py /
tests/test_gpu_loglik_cov.py (GPU).

The model is tests/covar_ref.py's: V = W_T W_T^T / d + lambda I, r_t = y_T,t - mu_t, Q~ = Q - m (m the train
means under snp, 0 under gblup), N = n_T, r = 1 under snp and 0 under gblup, c the covariate count,
G = Q~_T^T V^-1 Q~_T = C C^T, h_t = Q~_T^T V^-1 r_t, P = V^-1 - V^-1 Q~_T G^-1 Q~_T^T V^-1.  For a listed column j
with w_j as tests/score_ref.py has it and a_j = Q~_T^T V^-1 w_j:

  u_P = w_j^T P r_t = u - (C^-1 a_j).(C^-1 h_t),  v_P = w_j^T P w_j = v - |C^-1 a_j|^2,  q_P = q - |C^-1 h_t|^2
  dof = N - r - c,  log|A^T V A| = log|V| - r log lambda + log|G| - log|Q~_T^T Q~_T|
  l_R = -1/2 [ dof (log 2 pi + 1 + log(q_P / dof)) + log|A^T V A| ],  sigma2_g = q_P / dof

Only the dense N x N V is used, for both branches (one column Cholesky), so that the library's SNP-form
identities are tested, not restated.  A listed SNP with v_P <= PIV_RTOL v gives u_P = v_P = 0, the library's rule.
"""
import functools

import numpy as np

from tests import covar_ref as C
from tests import loglik_ref as LR
from tests import model_ref as R
from tests import reliability_ref as RQ
from tests import score_ref as S

LD = np.longdouble
H2 = R.H2
TOL = S.TOL                      # the GPU tests' bound: |got - ref| <= TOL max(1, max |ref|)
LL_TOL = LR.TOL
HOST_TOL = S.HOST_TOL            # float64 against longdouble, relative to the largest |ref|
PIV_RTOL = C.PIV_RTOL
SPAN_MIN = 1e-6                  # v_P >= SPAN_MIN v for every listed SNP of the cases: TOL stays meaningful
close = S.close


def _chol_piv(A):
    """Column Cholesky with the library's pivot rule (positive above PIV_RTOL of the pivot's own diagonal
    entry, and finite); None otherwise."""
    n = A.shape[0]
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(n):
            v = A[j:, j] - L[j:, :j] @ L[j, :j]
            if not (v[0] > PIV_RTOL * A[j, j] and np.isfinite(v[0])):
                return None
            L[j, j] = np.sqrt(v[0])
            L[j + 1:, j] = v[1:] / L[j, j]
    return L


def _logdet(L):
    return 2 * np.sum(np.log(np.diag(L))) if L.shape[0] else L.dtype.type(0)


def _adj(idx, train, geno, pheno, cov, h2, branch, snps, dtype):
    geno = np.asarray(geno)
    T = np.asarray(train)
    _, wt, d, lam = RQ._setup(idx, train, geno, h2, branch, dtype)
    br = R._branch(len(np.asarray(idx)), geno.shape[0], branch)
    r = 1 if br == "snp" else 0
    cand = S.wrap(np.arange(geno.shape[1]) if snps is None else snps, geno.shape[1])
    x = geno[:, cand].astype(np.int64)
    refrows = np.arange(geno.shape[0]) if br == "gblup" else T
    wc = x[T].astype(dtype) - x[refrows].sum(axis=0).astype(dtype) / dtype(len(refrows))      # (n_T, m)
    Y = np.asarray(pheno, dtype=np.float64)
    y = (Y[:, None] if Y.ndim == 1 else Y)[T].astype(dtype)
    if r:
        y = y - y.sum(axis=0) / dtype(len(y))
    nT, nt, m = len(T), y.shape[1], len(cand)
    Qd = np.zeros((geno.shape[0], 0)) if cov is None else np.asarray(cov, dtype=np.float64)
    Qd = (Qd[:, None] if Qd.ndim == 1 else Qd).astype(dtype)
    c = Qd.shape[1]
    Qt = Qd[T] - (Qd[T].sum(axis=0) / dtype(nT) if r else dtype(0))
    dof = nT - r - c
    nan = {"u": np.full((nt, m), np.nan), "v": np.full(m, np.nan), "q": np.full(nt, np.nan),
           "loglik": np.full(nt, np.nan), "sigma2_g": np.full(nt, np.nan), "b": np.full((nt, c), np.nan),
           "dof": dof, "G": np.full((c, c), np.nan), "branch": br, "v_plain": np.full(m, np.nan)}
    if not d > 0:
        return nan
    V = (wt @ wt.T) / d
    V[np.diag_indices_from(V)] += lam
    L = RQ._chol(V)
    if L is None:
        return nan
    s, z, Sq = RQ._forward(L, wc), RQ._forward(L, y), RQ._forward(L, np.ascontiguousarray(Qt))
    u, v, q = z.T @ s, np.sum(s * s, axis=0), np.sum(z * z, axis=0)
    G = Sq.T @ Sq
    Cf = _chol_piv(G)
    if Cf is None:
        return dict(nan, G=G)
    ya, yh = RQ._forward(Cf, Sq.T @ s), RQ._forward(Cf, Sq.T @ z)        # (c, m), (c, nt)
    b = np.zeros((c, nt), dtype=dtype)
    for i in range(c - 1, -1, -1):
        b[i] = (yh[i] - Cf[i + 1:, i] @ b[i + 1:]) / Cf[i, i]
    uP, vP, qP = u - yh.T @ ya, v - np.sum(ya * ya, axis=0), q - np.sum(yh * yh, axis=0)
    span = ~(vP > PIV_RTOL * v)
    uP[:, span] = 0
    vP[span] = 0
    out = dict(nan, u=uP, v=vP, q=qP, b=np.ascontiguousarray(b.T), G=G, v_plain=v)
    Cq = _chol_piv(Qt.T @ Qt)
    if dof <= 0:
        return dict(out, u=nan["u"], v=nan["v"], q=nan["q"])
    if Cq is None:
        return out
    ldet = _logdet(L) - r * np.log(lam) + _logdet(Cf) - _logdet(Cq)
    with np.errstate(all="ignore"):
        two_pi = 8 * np.arctan(dtype(1))
        df = dtype(dof)
        ll = -(df * (np.log(two_pi) + 1 + np.log(qP / df)) + ldet) / 2
    bad = ~(qP > 0) | ~np.isfinite(qP)
    return dict(out, loglik=np.where(bad, np.nan, ll), sigma2_g=np.where(bad, np.nan, qP / df))


def adj_ref(idx, train, geno, pheno, cov, h2, branch="auto", snps=None):
    """{u (nt, m), v (m,), q (nt,), loglik (nt,), sigma2_g (nt,), b (nt, c), dof, G, v_plain} in float64 for the
    listed columns (None: all); cov None or (n, 0): no covariates."""
    return _adj(idx, train, geno, pheno, cov, h2, branch, snps, np.float64)


def adj_wide(idx, train, geno, pheno, cov, h2, branch="auto", snps=None):
    """The same in np.longdouble."""
    return _adj(idx, train, geno, pheno, cov, h2, branch, snps, LD)


def contrast_ref(idx, train, geno, pheno, cov, h2, branch="auto"):
    """(l_R, q_P) as they are defined, extending tests/loglik_ref.py::loglik_contrast: the profile likelihood
    of the N - r - c error contrasts A^T y_T, A an orthonormal basis of the complement of [1 Q~_T] (snp) or Q_T
    (gblup) from an SVD, with covariance sigma2_g A^T V A.  One phenotype vector."""
    geno = np.asarray(geno)
    T = np.asarray(train)
    _, wt, d, lam = RQ._setup(idx, train, geno, h2, branch, np.float64)
    br = R._branch(len(np.asarray(idx)), geno.shape[0], branch)
    N = wt.shape[0]
    V = (wt @ wt.T) / d
    V[np.diag_indices_from(V)] += lam
    Qd = np.asarray(cov, dtype=np.float64)
    Qd = Qd[:, None] if Qd.ndim == 1 else Qd
    X = np.hstack([np.ones((N, 1)), Qd[T] - Qd[T].mean(axis=0)]) if br == "snp" else Qd[T]
    U, sv, _ = np.linalg.svd(X, full_matrices=True)
    rank = X.shape[1]
    assert sv[rank - 1] > 1e-8 * sv[0]
    A = U[:, rank:]
    dof = N - rank
    yc = A.T @ np.asarray(pheno, dtype=np.float64)[T]
    Vc = A.T @ V @ A
    sign, logdet = np.linalg.slogdet(Vc)
    assert sign > 0
    q = yc @ np.linalg.solve(Vc, yc)
    return -0.5 * (dof * (np.log(2 * np.pi) + 1 + np.log(q / dof)) + logdet), q


def estimate_ref(idx, train, geno, pheno, cov, branch="auto", grid=np.linspace(0.02, 0.98, 25), refine=3, points=9):
    """GpuBlupEngine.estimate_h2's procedure (tests/loglik_ref.py::estimate_ref's) for one model and one phenotype
    vector on adj_ref's likelihood; cov None: on loglik_ref's."""
    if cov is None:
        return LR.estimate_ref(idx, train, geno, pheno, branch, grid, refine, points)
    none = np.zeros(0, dtype=np.int64)

    def ev(hs):
        out = [adj_ref(idx, train, geno, pheno, cov, float(h), branch, snps=none) for h in hs]
        return np.array([o["loglik"][0] for o in out]), np.array([o["sigma2_g"][0] for o in out])

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
# Inputs: tests/covar_ref.py's cases (panels, splits, genomes, covariates); every case over all columns.
# ---------------------------------------------------------------------------------------------
panel = C.panel
deep_panel = C.deep_panel
cases = C.cases
case_inputs = C.case_inputs
make_cov = C.make_cov
cand_list = S.cand_list
LIST_LENGTHS = S.LIST_LENGTHS
H2S = (0.05, 0.4, 0.9)           # the likelihood tests' grid


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name, h2=H2):
    """adj_ref of a case of cases() over all columns of its panel at h2, computed once (read-only)."""
    idx, T, V, geno, pheno, cov, br = case_inputs(name)
    return _freeze(adj_ref(idx, T, geno, pheno, cov, h2, br))


@functools.lru_cache(maxsize=None)
def case_loglik(name, h2):
    """(loglik, sigma2_g) of a case at h2 (no SNP listed), once."""
    idx, T, V, geno, pheno, cov, br = case_inputs(name)
    out = adj_ref(idx, T, geno, pheno, cov, h2, br, snps=np.zeros(0, dtype=np.int64))
    return float(out["loglik"][0]), float(out["sigma2_g"][0])


# The 1200 x 1100 synthetic panel of the LDS-limit tests: systems of exactly 1024 rows in both forms (snp with
# k = 1000 on n_T = 1100 pads to 1024; forced gblup on n_T = 1000) and one above (forced gblup on n_T = 1100).
BIG_N, BIG_P, BIG_C, BIG_M = 1200, 1100, 16, 33


@functools.lru_cache(maxsize=None)
def big_panel():
    rng = np.random.default_rng(120011)
    freq = rng.uniform(0.1, 0.9, BIG_P)
    geno = (rng.random((BIG_N, BIG_P)) < freq).astype(np.int8) + (rng.random((BIG_N, BIG_P)) < freq).astype(np.int8)
    cov = make_cov(BIG_N, BIG_C, ones=True, seed=3)
    beta = rng.standard_normal(BIG_P) * (rng.random(BIG_P) < 0.05)
    pheno = geno @ beta + cov[:, 1:] @ rng.standard_normal(BIG_C - 1) + 2.0 * rng.standard_normal(BIG_N)
    perm = rng.permutation(BIG_N)
    # (the snp case takes covariates without the column of ones: centred over the train rows it would vanish)
    out = {"geno": geno, "pheno": pheno, "cov": cov, "cov_snp": make_cov(BIG_N, BIG_C, seed=4), "T1100": perm[:1100], "V1100": perm[1100:],
           "T1000": perm[:1000], "V1000": perm[1000:1100], "g1000": rng.choice(BIG_P, 1000, replace=False),
           "gall": np.arange(BIG_P)}
    out["snps"] = cand_list(out["g1000"], BIG_P, BIG_M)
    return _freeze(out)


def big_cases():
    """(name, genome key, train key, valid key, covariates key, branch, system rows, plan in LDS)"""
    return [("snp-1000-on-1100", "g1000", "T1100", "V1100", "cov_snp", "snp", 1024, True),
            ("gblup-on-1000", "gall", "T1000", "V1000", "cov", "gblup", 1024, True),
            ("gblup-on-1100", "gall", "T1100", "V1100", "cov", "gblup", 1152, False)]


@functools.lru_cache(maxsize=None)
def big_ref(name):
    bp = big_panel()
    _, g, t, v, q, br, _, _ = next(x for x in big_cases() if x[0] == name)
    return _freeze(adj_ref(bp[g], bp[t], bp["geno"], bp["pheno"], bp[q], H2, br, snps=bp["snps"]))


# estimate_h2 with covariates: phenotypes with a strong covariate effect on the 331 x 600 panel
@functools.lru_cache(maxsize=None)
def est_inputs():
    pn = panel()
    rng = np.random.default_rng(4242)
    n = R.N_ANIMALS
    cov = make_cov(n, 3, seed=9)
    g = pn["genomes"][200]
    a = pn["geno"][:, S.wrap(g, R.N_SNPS)].astype(np.float64)
    a = a - a.mean(axis=0)
    gv = a @ rng.standard_normal(a.shape[1])
    gv = gv / gv.std()
    y = gv + cov @ np.array([3.0, -2.0, 2.5]) + rng.standard_normal(n)
    T, V = pn["splits"][257, 70]
    return _freeze({"geno": pn["geno"], "pheno": y, "cov": cov, "genome": g, "T": T, "V": V})
