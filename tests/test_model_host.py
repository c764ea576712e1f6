"""The fitted-model export without a GPU: the float64 restatement of the reference's model
(tests/model_ref.py) pinned against the reference's own numbers, its own error bounded by a wider
solve on every case tests/test_gpu_model.py compares effects on, and tblup_amd.model.PanelModel.
"""
import os

import numpy as np
import pytest

from oracle import blup_oracle as O
from tests import model_ref as R
from tblup_amd.model import PanelModel

LD = np.longdouble
PIN_RTOL = 1e-10      # restatement against the reference's recorded numbers
WIDE_TOL = 1e-11      # restatement against the longdouble solve (tests/test_edge_cases_cpu.py's bound)


def _relmax(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- the restatement is the reference's model ---------------------------------------------------
def test_restatement_matches_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "model.npz"))
    geno, pheno, T, V, h2 = z["geno"], z["pheno"], z["T"], z["V"], float(z["h2"])
    names = sorted(k[:-4] for k in z.files if k.endswith("_idx"))
    assert len([n for n in names if n.startswith("snp")]) >= 4 and len([n for n in names if n.startswith("gblup")]) >= 3
    worst = {}
    for name in names:
        idx = z[name + "_idx"]
        assert len(idx) <= 400
        if name.startswith("snp"):
            m = R.fit_ref(idx, T, geno, pheno, h2, "snp")
            e = _relmax(m["effects"], z[name + "_coef"])
            worst["coef"] = max(worst.get("coef", 0.0), e)
            assert e <= PIN_RTOL, (name, e)
            assert abs(m["intercept"] - float(z[name + "_intercept"])) <= PIN_RTOL * abs(float(z[name + "_intercept"])), name
            # the centre the reference subtracted before the fit (evaluator.py:304-309)
            np.testing.assert_array_equal(m["center"], geno[np.ix_(T, idx)].sum(axis=0) / float(len(T)))
            fit = O.snp_blup(idx, T, V, geno, pheno, h2)
        else:
            e = _relmax(R.gblup_all_ref(idx, T, geno, pheno, h2), z[name + "_pred"])
            worst["pred"] = max(worst.get("pred", 0.0), e)
            assert e <= PIN_RTOL, (name, e)
            fit = O.gblup(idx, T, V, geno, pheno, h2)
        assert abs(fit - float(z[name + "_fit"])) <= 1e-10, name
    print("fixture pin: " + ", ".join("worst %s rel %.2e" % kv for kv in sorted(worst.items())))


# ---- the restatement's own error on the GPU suite's cases -----------------------------------------
def test_effect_cases_are_fair():
    """Every effects case of test_gpu_model.py group A: fit_ref within 1e-11 (relative to the
    individual's max |effect|) of the longdouble solve, so the GPU suite's 1e-9 is a 100x margin."""
    pn = R.panel()
    worst = {}
    for name, s, k, br in R.effect_cases():
        m = R.case_ref(name)
        w = R.fit_wide(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], R.H2, br)
        assert w is not None and not np.any(np.isnan(m["effects"])), name
        e = float(np.max(np.abs(m["effects"].astype(LD) - w)) / np.max(np.abs(w)))
        grp = name.split("-")[0]
        worst[grp] = max(worst.get(grp, 0.0), e)
        assert e <= WIDE_TOL, (name, e)
    assert set(worst) == {"auto", "snp", "gblup"}
    print("effects vs longdouble: " + ", ".join("%s worst rel %.2e" % kv for kv in sorted(worst.items())))


def test_panel_is_as_described():
    pn = R.panel()
    assert pn["geno"].shape == (331, 600) and pn["geno"].shape[0] % 4 != 0
    for (nT, nV), (T, V) in pn["splits"].items():
        assert len(T) == nT and len(V) == nV and not set(T) & set(V)
    assert len(set(pn["genomes"]["dup"])) < len(pn["genomes"]["dup"])
    assert pn["genomes"]["neg"].min() < 0 and pn["genomes"]["neg"].min() >= -600
    assert sorted(k for k in pn["genomes"] if isinstance(k, int)) == R.KS


# ---- PanelModel ---------------------------------------------------------------------------------
def _model(s, k, branch="auto"):
    pn = R.panel()
    idx = np.asarray(pn["genomes"][k])
    m = R.fit_ref(idx, pn["splits"][s][0], pn["geno"], pn["pheno"], R.H2, branch)
    return PanelModel(np.where(idx < 0, idx + R.N_SNPS, idx), m["center"], m["effects"], m["intercept"], R.H2,
                      m["branch"], 0.5)


@pytest.mark.parametrize("s,k", [((127, 5), 64), ((129, 64), 200), ((257, 70), 400), ((128, 2), "dup"),
                                 ((129, 64), "neg")])
def test_predict_matches_oracle_ebvs(s, k):
    """The formula on the restated effects is the oracle's EBV of every animal, in or out of the split."""
    pn = R.panel()
    got = _model(s, k).predict(pn["geno"])
    ref = R.ebv_all_ref(s, k)
    assert got.shape == (R.N_ANIMALS,)
    assert _relmax(got, ref) <= 1e-11
    sub = np.array([330, 0, 7, 7, 200])
    np.testing.assert_allclose(_model(s, k).predict(pn["geno"][sub]), ref[sub], rtol=0, atol=1e-11 * np.max(np.abs(ref)))


def test_predict_multi_trait_shapes():
    pn = R.panel()
    T = pn["splits"][129, 64][0]
    idx = pn["genomes"][65]
    ms = [R.fit_ref(idx, T, pn["geno"], pn["Y"][:, t], R.H2) for t in range(3)]
    m = PanelModel(idx, ms[0]["center"], np.stack([x["effects"] for x in ms]), [x["intercept"] for x in ms])
    out = m.predict(pn["geno"][:10])
    assert m.n_traits == 3 and out.shape == (3, 10)
    for t in range(3):
        one = PanelModel(idx, ms[t]["center"], ms[t]["effects"], ms[t]["intercept"])
        np.testing.assert_allclose(one.predict(pn["geno"][:10]), out[t], rtol=1e-13, atol=1e-14)   # (BLAS gemm against gemv)


def test_save_load_round_trip(tmp_path):
    pn = R.panel()
    m = _model((129, 64), 200)
    path = str(tmp_path / "panel_model.npz")
    m.save(path)
    b = PanelModel.load(path)
    for f in ("indices", "center", "effects", "intercept"):
        np.testing.assert_array_equal(getattr(m, f), getattr(b, f))
    assert (b.h2, b.branch, b.fitness) == (m.h2, m.branch, m.fitness)
    np.testing.assert_array_equal(m.predict(pn["geno"]), b.predict(pn["geno"]))


def test_argument_validation():
    ok = dict(indices=[3, 1, 3], center=[1.0, 0.5, 1.0], effects=[[0.1, 0.2, 0.3]], intercept=[0.0])
    PanelModel(**ok)
    PanelModel(**dict(ok, effects=[0.1, 0.2, 0.3], intercept=0.0))          # one trait given flat
    for bad in (dict(indices=[]), dict(indices=[-1, 0, 1]), dict(indices=[[1, 2, 3]]), dict(indices=[0.5, 1, 2]),
                dict(center=[1.0, 0.5]), dict(effects=[[0.1, 0.2]]), dict(intercept=[0.0, 1.0]),
                dict(effects=np.zeros((2, 3)), intercept=[0.0])):
        with pytest.raises(ValueError):
            PanelModel(**dict(ok, **bad))
    with pytest.raises(ValueError):
        PanelModel(branch="auto", **ok)
    m = PanelModel(**ok)
    with pytest.raises(IndexError):
        m.predict(np.zeros((4, 3), dtype=np.int8))       # index 3 needs four columns
    with pytest.raises(ValueError):
        m.predict(np.zeros(4, dtype=np.int8))
    assert m.predict(np.zeros((5, 4), dtype=np.int8)).shape == (5,)
