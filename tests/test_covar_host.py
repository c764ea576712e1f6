"""The restatement behind tests/test_gpu_covar.py, checked on the CPU on every case the GPU test uses, and the
host side of the covariate model (PanelModel's fields, predict, adjust, save / load).

  * float64 against np.longdouble: b and y* within 1e-11 of the largest |ref|
  * against Henderson's mixed-model equations on [1, Q~, W] (one dense system, no V and no GLS step): b and
    the SNP effects of y*'s model.  The two routes share no factorisation; the bound 1e-8 max(1, max |ref|)
    is eps (1.1e-16) times the equations' condition number, which lambda d on the SNP block keeps below
    ~1e7 on these panels, with a decade to spare.
  * cond(Q~^T V^-1 Q~) < 1e6: the chosen inputs keep the GPU tolerance meaningful
"""
import numpy as np
import pytest

from tests import covar_ref as C
from tests import model_ref as R
from tblup_amd.model import PanelModel

NAMES = [c[0] for c in C.cases()]
MME_TOL = 1e-8


@pytest.mark.parametrize("name", NAMES)
def test_restatement(name):
    idx, T, V, geno, pheno, cov, br = C.case_inputs(name)
    ref = C.case_ref(name)
    assert np.all(np.isfinite(ref["cov_effects"])) and np.isfinite(ref["fitness"]), name
    assert ref["cond"] < C.COND_MAX, (name, ref["cond"])
    wide = C.gls_wide(idx, T, geno, pheno, cov, C.H2, br)
    for f, g in (("cov_effects", "b"), ("ystar", "ystar"), ("cov_center", "m")):
        w = wide[g].astype(np.float64)
        err = float(np.max(np.abs(ref[f] - w)) / max(1.0, float(np.max(np.abs(w)))))
        assert err <= C.HOST_TOL, (name, f, err)
    b, eff = C.mme_ref(idx, T, geno, pheno, cov, C.H2, br)
    assert C.close(b, ref["cov_effects"]) <= MME_TOL, (name, C.close(b, ref["cov_effects"]))
    assert C.close(eff, ref["effects"]) <= MME_TOL, (name, C.close(eff, ref["effects"]))
    # the branch's centre rule
    if ref["branch"] == "gblup":
        assert np.all(ref["cov_center"] == 0.0)
    else:
        np.testing.assert_allclose(ref["cov_center"], cov[T].mean(axis=0), rtol=0, atol=1e-14)


def test_collinear_and_constant_columns_are_nan():
    pn = C.panel()
    T, V = pn["splits"][129, 64]
    q = C.make_cov(R.N_ANIMALS, 3)
    two = np.ascontiguousarray(np.stack([q[:, 2], q[:, 2]], axis=1))
    ref = C.cov_ref(pn["genomes"][64], T, V, pn["geno"], pn["pheno"], two, C.H2)
    assert np.all(np.isnan(ref["cov_effects"])) and np.isnan(ref["fitness"]) and np.all(np.isnan(ref["effects"]))
    const = q.copy()
    const[T, 1] = 3.0
    ref = C.cov_ref(pn["genomes"][64], T, V, pn["geno"], pn["pheno"], const, C.H2, "snp")
    assert np.all(np.isnan(ref["cov_effects"]))


def _model(nt=1, c=3, k=7, seed=0):
    rng = np.random.default_rng(seed)
    return PanelModel(rng.choice(50, k, replace=False), rng.random(k), rng.standard_normal((nt, k)),
                      rng.standard_normal(nt), 0.4, "snp", 0.5, cov_effects=rng.standard_normal((nt, c)),
                      cov_center=rng.standard_normal(c))


def test_panel_model_round_trip_and_old_format(tmp_path):
    m = _model(nt=2)
    p = str(tmp_path / "m.npz")
    m.save(p)
    back = PanelModel.load(p)
    for f in ("indices", "center", "effects", "intercept", "cov_effects", "cov_center"):
        np.testing.assert_array_equal(getattr(back, f), getattr(m, f))
    assert back.n_covariates == 3 and back.branch == "snp" and back.h2 == 0.4
    # a file written before the fields existed loads as a model without covariates
    old = str(tmp_path / "old.npz")
    np.savez(old, indices=m.indices, center=m.center, effects=m.effects, intercept=m.intercept, h2=np.float64(m.h2),
             branch=np.array(m.branch), fitness=np.float64(m.fitness))
    plain = PanelModel.load(old)
    assert plain.cov_effects is None and plain.cov_center is None and plain.n_covariates == 0
    np.testing.assert_array_equal(plain.effects, m.effects)
    # and a model without covariates writes that same old format
    plain.save(str(tmp_path / "again.npz"))
    with np.load(str(tmp_path / "again.npz")) as z:
        assert "cov_effects" not in z.files and "cov_center" not in z.files


@pytest.mark.parametrize("nt", [1, 3])
def test_predict_and_adjust(nt):
    m = _model(nt=nt)
    rng = np.random.default_rng(5)
    g = rng.integers(0, 3, (9, 50)).astype(np.int8)
    q = rng.standard_normal((9, 3))
    base = m.predict(g)
    part = m.cov_effects @ (q - m.cov_center).T
    want = (np.atleast_2d(base) + part)
    np.testing.assert_allclose(np.atleast_2d(m.predict(g, covariates=q)), want, rtol=0, atol=1e-13)
    np.testing.assert_array_equal(m.predict(g), base)            # without the argument: as before
    y = rng.standard_normal(9) if nt == 1 else rng.standard_normal((9, nt))
    ys = m.adjust(y, q)
    assert ys.shape == y.shape
    np.testing.assert_allclose(ys if nt > 1 else ys[:, None], (y if nt > 1 else y[:, None]) - part.T, rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        m.predict(g, covariates=q[:, :2])
    with pytest.raises(ValueError):
        PanelModel(m.indices, m.center, m.effects, m.intercept).predict(g, covariates=q)
    with pytest.raises(ValueError):
        PanelModel(m.indices, m.center, m.effects, m.intercept, cov_effects=m.cov_effects)


def test_binding_declares_the_entry():
    from tblup_amd import _native
    assert "tblup_fit_cov_batch" in _native.SIGNATURES and len(_native.SIGNATURES["tblup_fit_cov_batch"][1]) == 16
    assert hasattr(_native.load(), "tblup_fit_cov_batch")
