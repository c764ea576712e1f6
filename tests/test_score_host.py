"""The score statistics' restatement (tests/score_ref.py) against its own wider computation, against the
fitted effects and the likelihood's quadratic form, and tblup_amd.model.SnpScores -- no GPU.

  * float64 against np.longdouble within 1e-11 x the largest |ref| over the model's candidates, for u, v
    and q, in both forms, for every case of tests/reliability_ref.py::cases() and the deeper panel
    (measured: 5e-15)
  * the kernel-form and SNP-form restatements agree to the same bound
  * for in-panel candidates u_j = d * effects_j of tests/model_ref.py::fit_ref, d from the model's centre
  * q is tests/loglik_ref.py's quadratic form (sigma2_g * dof)
  * the candidate lists of the GPU tests mix in-panel and out-of-panel columns, negatives and repeats
  * SnpScores' derived statistics against direct formulas, NaN at v = 0
  * the entry is declared in the header and in the binding's table
"""
import os

import numpy as np
import pytest

from tests import loglik_ref as LL
from tests import model_ref as R
from tests import score_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.N_SNPS


def _rel(a, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / np.max(np.abs(ref)))


def _inputs(name):
    pn = S.panel()
    _, s, k, br = next(c for c in S.cases() if c[0] == name)
    return pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], br


def test_float64_against_longdouble_and_forms_agree():
    worst = {"wide": 0.0, "forms": 0.0}
    for name, *_ in S.cases():
        g, T, geno, y, br = _inputs(name)
        wide = S.score_wide(g, T, geno, y, S.H2, br, form="kernel")
        got = {f: S.score_ref(g, T, geno, y, S.H2, br, form=f) for f in ("kernel", "snp")}
        for f in got:
            for a, w, what in zip(got[f], wide, "uvq"):
                assert np.all(np.isfinite(a)), (name, f, what)
                e = _rel(a, w)
                worst["wide"] = max(worst["wide"], e)
                assert e <= S.HOST_TOL, (name, f, what, e)
        for a, b, what in zip(got["kernel"], got["snp"], "uvq"):
            e = _rel(a, b)
            worst["forms"] = max(worst["forms"], e)
            assert e <= S.HOST_TOL, (name, what, e)
        # the default form is one of the two, bit for bit
        auto = S.case_ref(name)
        k, nT = len(g), len(T)
        form = "snp" if (R._branch(k, geno.shape[0], br) == "snp" and k <= nT) else "kernel"
        for a, b in zip(auto, got[form]):
            np.testing.assert_array_equal(a, b)
    print("\nSCORE host: float64 vs longdouble %.3e, kernel vs SNP form %.3e" % (worst["wide"], worst["forms"]))


def test_deeper_panel_against_longdouble():
    dp = S.deep_panel()
    args = (dp["genome"], dp["train"], dp["geno"], dp["pheno"], S.H2, "auto")
    wide = S.score_wide(*args, form="snp")
    for f in ("kernel", "snp"):
        for a, w, what in zip(S.score_ref(*args, form=f), wide, "uvq"):
            assert _rel(a, w) <= S.HOST_TOL, (f, what)
    for a, b in zip(S.deep_ref(), S.score_ref(*args, form="snp")):
        np.testing.assert_array_equal(a, b)


def test_in_panel_score_is_d_times_effect():
    worst = 0.0
    for name, *_ in S.cases():
        g, T, geno, y, br = _inputs(name)
        m = R.fit_ref(g, T, geno, y, S.H2, br)
        d = S.d_of_center(m["center"])
        u = S.case_ref(name)[0][0]
        e = float(np.max(np.abs(u[S.wrap(g, P)] - d * m["effects"])) / np.max(np.abs(u)))
        worst = max(worst, e)
        assert e <= S.HOST_TOL, (name, e)
    print("\nSCORE host: u_j = d beta_j within %.3e" % worst)


def test_q_is_the_likelihoods_quadratic_form():
    for name, *_ in S.cases():
        g, T, geno, y, br = _inputs(name)
        _, s2 = LL.loglik_ref(g, T, geno, y, S.H2, br)
        q = S.case_ref(name)[2][0]
        assert abs(q - s2 * S.dof(g, T, geno, br)) <= S.HOST_TOL * abs(q), name


def test_several_traits_share_info():
    pn = S.panel()
    T = pn["splits"][129, 64][0]
    for k in (64, 200, 400):
        g = pn["genomes"][k]
        u4, v4, q4 = S.score_ref(g, T, pn["geno"], pn["Y"], S.H2)
        assert u4.shape == (4, P) and v4.shape == (P,) and q4.shape == (4,)
        for t in range(4):
            u1, v1, q1 = S.score_ref(g, T, pn["geno"], pn["Y"][:, t], S.H2)
            np.testing.assert_array_equal(v1, v4)
            assert _rel(u4[t], u1[0]) <= S.HOST_TOL and abs(q4[t] - q1[0]) <= S.HOST_TOL * abs(q1[0])


@pytest.mark.parametrize("m", S.LIST_LENGTHS)
def test_candidate_lists(m):
    pn = S.panel()
    g = pn["genomes"][65]
    T = pn["splits"][129, 64][0]
    lst = S.cand_list(g, P, m)
    assert lst.shape == (m,) and np.all((lst >= -P) & (lst < P))
    inside = np.isin(S.wrap(lst, P), S.wrap(g, P))
    if m >= 3:
        assert inside.any() and (~inside).any() and (lst < 0).any() and lst[-1] == lst[0]
    full = S.case_ref("auto-129-64-65")
    u, v, q = S.score_ref(g, T, pn["geno"], pn["pheno"], S.H2, snps=lst)
    assert _rel(u, full[0][:, S.wrap(lst, P)]) <= S.HOST_TOL and _rel(v, full[1][S.wrap(lst, P)]) <= S.HOST_TOL
    np.testing.assert_array_equal(q, full[2])


def test_monomorphic_inputs():
    pn = S.panel()
    geno = pn["geno"].copy()
    T = pn["splits"][129, 64][0]
    geno[:, 0] = 0
    geno[T, 1] = 2
    u, v, q = S.score_ref(np.array([0]), T, geno, pn["pheno"], S.H2)        # d = 0
    assert np.all(np.isnan(u)) and np.all(np.isnan(v)) and np.all(np.isnan(q))
    u, v, q = S.score_ref(pn["genomes"][64], T, geno, pn["pheno"], S.H2, snps=[0, 1, 2])
    assert u[0, 0] == 0 and v[0] == 0 and u[0, 1] == 0 and v[1] == 0 and v[2] > 0 and q[0] > 0


def test_snp_scores_methods():
    from tblup_amd.model import SnpScores
    rng = np.random.default_rng(5)
    B, nt, m = 3, 2, 7
    u = rng.standard_normal((B, nt, m))
    v = rng.uniform(0.5, 2.0, (B, m))
    q = rng.uniform(50.0, 60.0, (B, nt))
    dof = np.array([128.0, 129.0, 128.0])
    v[1, 3] = 0.0
    u[1, :, 3] = 0.0
    sc = SnpScores(u, v, q, dof, np.arange(m))
    eff, chi, gain = sc.effect(), sc.chi2(), sc.loglik_gain()
    assert eff.shape == chi.shape == gain.shape == (B, nt, m)
    for b in range(B):
        for t in range(nt):
            for j in range(m):
                if v[b, j] == 0:
                    assert np.isnan(eff[b, t, j]) and np.isnan(chi[b, t, j]) and np.isnan(gain[b, t, j])
                    continue
                assert eff[b, t, j] == pytest.approx(u[b, t, j] / v[b, j], rel=1e-14)
                assert chi[b, t, j] == pytest.approx(u[b, t, j] ** 2 / (v[b, j] * q[b, t] / dof[b]), rel=1e-14)
                assert gain[b, t, j] == pytest.approx(
                    dof[b] / 2 * np.log(q[b, t] / (q[b, t] - u[b, t, j] ** 2 / v[b, j])), rel=1e-12)
    assert np.all(gain[np.isfinite(gain)] >= 0)
    with pytest.raises(ValueError):
        SnpScores(u, v[:, :-1], q, dof, np.arange(m))
    with pytest.raises(ValueError):
        SnpScores(u[0], v, q, dof, np.arange(m))


def test_statistics_of_the_restatement():
    """chi2 and loglik_gain on the restatement's values: the gain is the rise of loglik_ref's profile
    likelihood's data term when the SNP joins as a fixed covariate (checked through its definition)."""
    from tblup_amd.model import SnpScores
    g, T, geno, y, br = _inputs("auto-129-64-65")
    u, v, q = S.case_ref("auto-129-64-65")
    sc = SnpScores(u[None], v[None], q[None], [S.dof(g, T, geno, br)], np.arange(P))
    q1 = q[0] - u[0] ** 2 / v                       # the residual quadratic form with the covariate fitted
    assert np.all(q1 > 0)
    np.testing.assert_allclose(sc.loglik_gain()[0, 0], sc.dof[0] / 2 * np.log(q[0] / q1), rtol=1e-12)
    np.testing.assert_allclose(sc.chi2()[0, 0], u[0] ** 2 / v / (q[0] / sc.dof[0]), rtol=1e-12)


def test_entry_is_declared():
    from tblup_amd import _native
    with open(os.path.join(ROOT, "include", "tblup_gpu.h")) as f:
        header = f.read()
    assert "int tblup_snp_score_batch(tblup_ctx* ctx, int split_id, const int64_t* snps, int64_t n_cand" in header
    res, args = _native.SIGNATURES["tblup_snp_score_batch"]
    assert len(args) == 13
