"""Dense float64 restatement of the uncertainty under the model with fixed-effect covariates (TEST
INFRASTRUCTURE ONLY): reliabilities with the covariates' effects estimated, the error variance of a predicted
value and the sampling covariance of the covariates' effects -- by Henderson's mixed-model equations in SNP
space, a route that shares no identity with the library's factor algebra -- plus the V-form formulas in any
precision, and the inputs shared by tests/test_reliab_cov_host.py (CPU) and tests/test_gpu_reliab_cov.py (GPU).

The model is tests/covar_ref.py's: y_T - mu = Q~_T b + W_T beta + e, beta ~ N(0, sigma2_g / d I),
e ~ N(0, lambda sigma2_g I), Q~ = Q - m (m the train means under snp, 0 under gblup), g_a = w_a . beta.  With

    MME = [[Q~_T^T Q~_T, Q~_T^T W_T], [W_T^T Q~_T, W_T^T W_T + lambda d I]]

the error variance of l^T [b^; beta^] about l^T [b; beta] is lambda l^T MME^-1 l in units of sigma2_g:

    rel_cov(a)   = 1 - lambda l^T MME^-1 l / K_aa,   l = [0; w_a],  K_aa = w_a.w_a / d
    pev_total(a) = lambda l^T MME^-1 l,              l = [q~_a; w_a]
    cov_cov      = lambda (MME^-1)[:c, :c]

The V-form (include/tblup_gpu.h's definitions, as written there): V = W_T W_T^T / d + lambda I, k_Ta = W_T w_a / d,
G = Q~_T^T V^-1 Q~_T = C C^T, a_a = Q~_T^T V^-1 k_Ta,
    rel_cov = (k_Ta^T V^-1 k_Ta - |C^-1 a_a|^2) / K_aa,  pev_total = K_aa - k_Ta^T V^-1 k_Ta + |C^-1 (q~_a - a_a)|^2,
    cov_cov = G^-1.
"""
import functools

import numpy as np

from tests import covar_ref as C
from tests import model_ref as R
from tests import reliability_ref as RQ
from tests import score_cov_ref as A
from tests import score_ref as S

LD = np.longdouble
H2 = R.H2
TOL = S.TOL                      # the GPU tests' bound: |got - ref| <= TOL max(1, max |ref|)
HOST_TOL = C.HOST_TOL
PIV_RTOL = C.PIV_RTOL
COND_MAX = C.COND_MAX
close = S.close
panel = C.panel
deep_panel = C.deep_panel
cases = C.cases
case_inputs = C.case_inputs
make_cov = C.make_cov
big_panel = A.big_panel
big_cases = A.big_cases
LIST_LENGTHS = S.LIST_LENGTHS


def _inputs(idx, train, geno, cov, h2, branch, animals, dtype):
    geno = np.asarray(geno)
    T = np.asarray(train)
    w, wt, d, lam = RQ._setup(idx, train, geno, h2, branch, dtype)
    br = R._branch(len(np.asarray(idx)), geno.shape[0], branch)
    Qd = np.asarray(cov, dtype=np.float64)
    Qd = (Qd[:, None] if Qd.ndim == 1 else Qd).astype(dtype)
    m = Qd[T].sum(axis=0) / dtype(len(T)) if br == "snp" else np.zeros(Qd.shape[1], dtype=dtype)
    Qc = Qd - m
    an = np.arange(geno.shape[0]) if animals is None else np.asarray(animals, dtype=np.int64)
    return w[an], wt, d, lam, Qc[an], Qc[T], br


def _nan(n, c, br):
    return {"rel": np.full(n, np.nan), "pev": np.full(n, np.nan), "cov_cov": np.full((c, c), np.nan),
            "kaa": np.full(n, np.nan), "branch": br}


def mme_ref(idx, train, geno, cov, h2, branch="auto", animals=None, check=True):
    """{rel (m,), pev (m,), cov_cov (c, c), kaa (m,), branch} for the listed animals (None: all) from the
    mixed-model equations in SNP space, float64.  check: the inputs keep the GPU tolerance meaningful for the
    reference alone -- cond(G) <= COND_MAX (G = cov_cov^-1) and K_aa > 0 for every listed animal."""
    wa, wt, d, lam, qa, qt, br = _inputs(idx, train, geno, cov, h2, branch, animals, np.float64)
    n, c, k = wa.shape[0], qa.shape[1], wa.shape[1]
    if not d > 0:
        assert not check
        return _nan(n, c, br)
    Z = np.hstack([qt, wt])
    M = Z.T @ Z
    M[np.arange(c, c + k), np.arange(c, c + k)] += lam * d
    lg = np.vstack([np.zeros((c, n)), wa.T])
    lt = np.vstack([qa.T, wa.T])
    eye = np.vstack([np.eye(c), np.zeros((k, c))])
    X = np.linalg.solve(M, np.hstack([lg, lt, eye]))
    kaa = np.sum(wa * wa, axis=1) / d
    pev_g = lam * np.sum(lg * X[:, :n], axis=0)
    pev_t = lam * np.sum(lt * X[:, n:2 * n], axis=0)
    cc = lam * X[:c, 2 * n:]
    cc = (cc + cc.T) / 2
    if check:
        assert np.all(kaa > 0), "an animal with K_aa = 0"
        assert np.linalg.cond(cc) <= COND_MAX, np.linalg.cond(cc)
    with np.errstate(all="ignore"):
        rel = np.where(kaa > 0, 1 - pev_g / kaa, np.nan)
    return {"rel": rel, "pev": np.where(kaa > 0, pev_t, np.nan), "cov_cov": cc, "kaa": kaa, "branch": br}


def _vform(idx, train, geno, cov, h2, branch, animals, dtype):
    wa, wt, d, lam, qa, qt, br = _inputs(idx, train, geno, cov, h2, branch, animals, dtype)
    n, c = wa.shape[0], qa.shape[1]
    if not d > 0:
        return _nan(n, c, br)
    V = (wt @ wt.T) / d
    V[np.diag_indices_from(V)] += lam
    L = RQ._chol(V)
    if L is None:
        return _nan(n, c, br)
    s = RQ._forward(L, (wt @ wa.T) / d)                       # (n_T, n)
    Sq = RQ._forward(L, np.ascontiguousarray(qt))             # (n_T, c)
    G = Sq.T @ Sq
    Cf = A._chol_piv(G)
    if Cf is None:
        return _nan(n, c, br)
    a = Sq.T @ s                                              # (c, n)
    y, x = RQ._forward(Cf, a), RQ._forward(Cf, qa.T - a)
    kaa = np.sum(wa * wa, axis=1) / d
    kvk = np.sum(s * s, axis=0)
    Ci = RQ._forward(Cf, np.eye(c, dtype=dtype))
    with np.errstate(all="ignore"):
        rel = np.where(kaa > 0, (kvk - np.sum(y * y, axis=0)) / kaa, np.nan)
    pev = np.where(kaa > 0, kaa - kvk + np.sum(x * x, axis=0), np.nan)
    return {"rel": rel, "pev": pev, "cov_cov": Ci.T @ Ci, "kaa": kaa, "branch": br}


def vform_ref(idx, train, geno, cov, h2, branch="auto", animals=None):
    """The definitions as the header writes them (dense V, one column Cholesky), float64."""
    return _vform(idx, train, geno, cov, h2, branch, animals, np.float64)


def vform_wide(idx, train, geno, cov, h2, branch="auto", animals=None):
    """The same in np.longdouble."""
    return _vform(idx, train, geno, cov, h2, branch, animals, LD)


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """mme_ref of a case of cases() over all animals of its panel, computed once (read-only)."""
    idx, T, V, geno, pheno, cov, br = case_inputs(name)
    return _freeze(mme_ref(idx, T, geno, cov, H2, br))


@functools.lru_cache(maxsize=None)
def big_ref(name):
    """mme_ref of a case of big_cases() over all 1200 animals, once."""
    bp = big_panel()
    _, g, t, v, q, br, _, _ = next(x for x in big_cases() if x[0] == name)
    return _freeze(mme_ref(bp[g], bp[t], bp["geno"], bp[q], H2, br))


def animal_list(n, train, m, seed=0):
    """m row ids: train rows and rows outside the train part alternating from a fixed draw, and from m = 3 on
    the last entry repeats the first."""
    rng = np.random.default_rng(5000 + 10 * m + seed)
    a = rng.permutation(np.asarray(train))
    b = rng.permutation(np.setdiff1d(np.arange(n), train))
    out = np.array([(a if i % 2 == 0 else b)[(i // 2) % len(a if i % 2 == 0 else b)] for i in range(m)], dtype=np.int64)
    if m >= 3:
        out[-1] = out[0]
    return out
