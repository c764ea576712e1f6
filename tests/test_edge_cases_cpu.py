"""The inputs of tests/test_gpu_edges.py are fair: on every evaluator case of its groups A, B, C
and D1 the fp64 oracle agrees with a wider solve of the same system to 1e-11 (EBV relative,
fitness absolute), so the GPU suite's 1e-9 tolerance is a 100x margin over the reference's own
error and no seed is ill-conditioned by accident.  Cases where the oracle gives NaN give NaN here.

The wider solve: exact integer counts, centred in np.longdouble (x87 80-bit, eps 1.08e-19), a
plain column-by-column Cholesky and the two triangular solves in longdouble.  It solves the
system in the kernel form (n_T x n_T) or, for the snp branch with k <= n_T, in the SNP form
(k x k): the two are the same ridge solution in exact arithmetic.
"""
import numpy as np
import pytest

from oracle import blup_oracle as O
from tests import helpers as H

LD = np.longdouble
TOL = 1e-11


def test_longdouble_is_wide():
    assert np.finfo(LD).eps < 1e-18


def _chol_solve(A, b):
    """x with A x = b for SPD A, in A's precision: A = L L^T column by column, then two
    substitutions.  None if a pivot is not positive."""
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


def _pearson_wide(x, y):
    """O.pearson_r in longdouble: (|r| as the reference rounds it, the unrounded r)."""
    n = len(x)
    if np.any(np.isnan(x)) or np.all(x == x[0]) or np.all(y == y[0]):
        return float("nan"), float("nan")
    xm, ym = x - x.mean(), y - y.mean()
    r = np.sum(xm * ym) / np.sqrt(np.sum(xm * xm) * np.sum(ym * ym))
    r = min(max(r, LD(-1)), LD(1))
    return float(abs(np.round(r)) if n == 2 else abs(r)), float(r)


def blup_wide(idx, train, valid, geno, pheno, h2, branch):
    """(fitness, EBV_V, unrounded r) of the reference's blup() in longdouble."""
    geno = np.asarray(geno)
    n = geno.shape[0]
    idx = np.asarray(idx)
    if branch == "auto":
        branch = "gblup" if len(idx) > n else "snp"
    T, V = np.asarray(train), np.asarray(valid)
    a = geno[:, idx].astype(np.float64)              # products and sums below are exact integers < 2^53
    ref = np.arange(n) if branch == "gblup" else T
    N = len(ref)
    m = a[ref].sum(axis=0).astype(np.int64)
    sm, q = int(m.sum()), int(np.sum(m * m))
    d = LD(2 * N * sm - q) / LD(2 * N * N)           # 2 sum p (1 - p)
    y = np.asarray(pheno, dtype=np.float64).astype(LD)
    mu = LD(0) if branch == "gblup" else y[T].mean()
    yc = y[T] - mu
    alpha = (LD(1) - LD(h2)) / LD(h2) * d
    nan = np.full(len(V), np.nan, dtype=LD)
    if not d > 0:
        ebv = nan
    elif branch == "snp" and len(idx) <= len(T):
        # SNP form: (W^T W + alpha I) w = W^T yc, W = A_T - m / N; N W^T W = N A^T A - m m^T exactly
        S = N * (a[T].T @ a[T]).astype(np.int64) - np.outer(m, m)
        A = S.astype(LD) / LD(N)
        A[np.diag_indices_from(A)] += alpha
        cen = m.astype(LD) / LD(N)
        wt, wv = a[T].astype(LD) - cen, a[V].astype(LD) - cen
        w = _chol_solve(A, wt.T @ yc)
        ebv = nan if w is None else wv @ w + mu
    else:
        # kernel form: N^2 W_R W_T^T = N^2 A_R A_T^T - N (u_R + u_T) + q exactly, u = A m
        R = np.concatenate([T, V])
        u = (a @ m.astype(np.float64)).astype(np.int64)
        M = (N * N) * (a[R] @ a[T].T).astype(np.int64) - N * (u[R][:, None] + u[T][None, :]) + q
        K = M.astype(LD) / LD(N * N)
        A = K[:len(T)].copy()
        A[np.diag_indices_from(A)] += alpha
        w = _chol_solve(A, yc)
        ebv = nan if w is None else K[len(T):] @ w + mu
    f, r = _pearson_wide(ebv, y[V])
    return f, ebv, r


def _check(cases):
    n_nan = 0
    worst_e = worst_f = 0.0
    for c in cases:
        f, e = H.edge_oracle(c)
        fw, ew, rw = blup_wide(c["idx"], c["T"], c["V"], c["geno"], c["pheno"], H.EDGE_H2, c["branch"])
        if np.isnan(f) or np.isnan(fw):
            assert np.isnan(f) and np.isnan(fw), (c["name"], f, fw)
            n_nan += 1
            continue
        de = float(np.max(np.abs(e.astype(LD) - ew)) / np.max(np.abs(ew)))
        df = abs(f - fw)
        worst_e, worst_f = max(worst_e, de), max(worst_f, df)
        assert de <= TOL, (c["name"], de)
        assert df <= TOL, (c["name"], df)
        if len(c["V"]) == 2:
            assert abs(rw) > 0.1, (c["name"], rw)    # the n == 2 rounding is no coin toss
    print("cases %d, NaN %d, worst EBV rel %.2e, worst fitness abs %.2e" % (len(cases), n_nan, worst_e, worst_f))
    return n_nan


def test_group_a_unaligned_splits():
    cases = H.edge_a_cases()
    n_nan = _check(cases)
    # NaN where expected: the degenerate genome in every split, everything snp at n_T = 1
    names = {c["name"] for c in cases if np.isnan(H.edge_oracle(c)[0])}
    assert {"A-%d-%d-degenerate" % s for s in H.EDGE_A_SIZES} <= names
    assert n_nan < len(cases) // 4


def test_group_b_pearson_edges():
    cases = H.edge_b_cases()
    n_nan = _check(cases)
    const = [c for c in cases if "-const-" in c["name"]]
    assert n_nan == len(const) and all(np.isnan(H.edge_oracle(c)[0]) for c in const)


def test_group_c_trait_counts():
    assert _check(H.edge_c_cases()) == 0


def test_group_d1_int16_limit_snp_form():
    d = H.edge_d1()
    for nT, (T, _) in d["splits"].items():
        for g in d["genomes"]:
            a = d["geno"][np.ix_(T, g)].astype(np.float64)
            assert (a.T @ a).max() == 4 * nT            # the raw counts reach 4 n_T
    assert _check(H.edge_d1_cases()) == 0


def test_group_a_panel_is_as_described():
    a = H.edge_a()
    g = a["geno"]
    assert (g[:, 0] == 0).all() and (g[:, 1] == 2).all() and (g[:, 2] == 1).all()
    train_all = np.unique(np.concatenate([T for T, _ in a["splits"].values()]))
    assert len(np.unique(g[train_all, 3])) == 1 and len(np.unique(g[:, 3])) == 3
    for (nT, nV), (T, V) in a["splits"].items():
        assert len(T) == nT and len(V) == nV and not set(T) & set(V)
    assert any(np.any(np.diff(T) < 0) for T, _ in a["splits"].values())
    assert any(3 in gm for gm in a["genomes"].values())
    assert a["genomes"]["negative"].min() < 0


# ---- decode rows: the reference is defined, and the fallback rows do defeat the sample ------
def test_numpy_sort_order_of_special_keys():
    """What the GPU decode is held to: -0.0 ties with +0.0 by index; every NaN sorts last."""
    assert np.signbit(np.clip(-0.0, 0, 1))
    np.testing.assert_array_equal(np.argsort([0., -0., .5, -0., 0., -1., 0.], kind="stable"), [5, 0, 1, 3, 4, 6, 2])
    assert np.signbit(H.NEG_NAN) and np.isnan(H.NEG_NAN) and not np.signbit(H.POS_NAN)
    np.testing.assert_array_equal(np.argsort([H.NEG_NAN, np.inf, H.POS_NAN, -np.inf, H.NEG_NAN], kind="stable"),
                                  [3, 1, 0, 2, 4])


def test_decode_rows_cover_the_issue():
    for d in H.EDGE_G_D:
        rows = dict((kind, (keys, ks)) for kind, keys, ks in H.edge_g_rows(d))
        assert len(rows) == 8 and all(len(keys) == d for keys, _ in rows.values())
        assert all(1 <= k <= min(d, 8192) for _, ks in rows.values() for k in ks)
        if d >= 7:
            z, ks = rows["zeros"]
            order = np.argsort(z, kind="stable")
            assert any(z[order[-k]] == 0 and z[order[-k - 1]] == 0 for k in ks if k < d), d   # tie straddles k
            assert np.any(np.signbit(z) & (z == 0)) and np.any(~np.signbit(z) & (z == 0))
            nan = rows["nan"][0]
            assert np.any(np.isnan(nan) & np.signbit(nan)) and np.any(np.isnan(nan) & ~np.signbit(nan))


def test_decode_fallback_rows_defeat_the_sample():
    (n1, over, k1), (n2, few, k2) = H.edge_g_fallback_rows()
    assert H.decode_sample_candidates(over, k1) > 8192          # the candidate list overflows
    assert H.decode_sample_candidates(few, k2) < k2             # too few candidates
    ok = np.random.default_rng(1).uniform(size=50_000)          # the model itself: a plain row fits
    assert 1000 <= H.decode_sample_candidates(ok, 1000) <= 8192
