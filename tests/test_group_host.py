"""The class fixed effect on the host: tests/group_ref.py's expansion rules, the restatement's own error and its
invariance to the choice of reference level, PanelModel with a class factor, and the binding (no GPU).

The restatement is covar_ref's on the expanded design [Q, Z]; its float64 result is held against the longdouble
one at covar_ref.HOST_TOL, and cond(G) of every design the GPU tests use against covar_ref.COND_MAX.
"""
import numpy as np
import pytest

from tests import covar_ref as C
from tests import group_ref as G
from tests import model_ref as R

H2 = G.H2


def test_expansion_rules():
    n = 12
    train = np.array([0, 1, 2, 3, 4, 5, 6, 7])
    groups = np.array([7, 3, 3, 9, 7, 3, 9, 9, 3, 5, 7, 11])        # 5 and 11 are no train labels
    q = np.arange(2.0 * n).reshape(n, 2)
    Xg, lev = G.expand(q, groups, train, "gblup")
    np.testing.assert_array_equal(lev, [3, 7, 9])
    assert Xg.shape == (n, 5)
    np.testing.assert_array_equal(Xg[:, :2], q)
    np.testing.assert_array_equal(Xg[:, 2:], (groups[:, None] == np.array([3, 7, 9])).astype(float))
    np.testing.assert_array_equal(Xg[[9, 11], 2:], 0.0)               # unknown labels: a row of zeros
    np.testing.assert_array_equal(Xg[train, 2:].sum(axis=1), 1.0)     # one level per train animal
    Xs, _ = G.expand(q, groups, train, "snp")
    assert Xs.shape == (n, 4)
    np.testing.assert_array_equal(Xs, np.delete(Xg, 2, axis=1))       # the lowest level is the reference
    Xn, _ = G.expand(None, groups, train, "snp")
    np.testing.assert_array_equal(Xn, Xg[:, 3:])
    with pytest.raises(ValueError):
        G.expand(q, groups, train, "auto")
    # string labels sort as np.unique sorts them
    _, lev = G.expand(None, np.array(["b", "a", "c", "a"]), np.array([0, 1, 2]), "gblup")
    assert list(lev) == ["a", "b", "c"]


def test_make_groups_gives_every_level_a_train_record():
    pn = G.panel()
    for name, (L, _) in G.DESIGNS.items():
        for s in G.DESIGN_SPLITS[name]:
            T, V = pn["splits"][s]
            _, g = G.design_inputs(name, s)
            assert len(G.levels_of(g, T)) == L and set(g[V]) <= set(g[T])


def test_group_ref_fields_and_centres():
    pn = G.panel()
    s = (129, 64)
    T, V = pn["splits"][s]
    q, g = C.make_cov(R.N_ANIMALS, 3), G.make_groups(R.N_ANIMALS, 5, T)
    shares = np.array([np.mean(g[T] == l) for l in range(5)])
    rs = G.group_ref(pn["genomes"][64], T, V, pn["geno"], pn["pheno"], q, g, H2, "snp")
    assert rs["columns"] == 7 and rs["group_effects"].shape == (1, 5) and rs["cov_effects"].shape == (1, 3)
    assert rs["group_effects"][0, 0] == 0.0
    np.testing.assert_allclose(rs["group_center"], shares, rtol=0, atol=1e-15)
    rg = G.group_ref(pn["genomes"][64], T, V, pn["geno"], pn["pheno"], q, g, H2, "gblup")
    assert rg["columns"] == 8 and np.all(rg["group_center"] == 0.0) and np.all(rg["cov_center"] == 0.0)
    # y* is y minus the fitted fixed part
    Xs, _ = G.expand(q, g, T, "snp")
    ys = pn["pheno"] - (Xs - Xs[T].mean(axis=0)) @ np.concatenate([rs["cov_effects"][0], rs["group_effects"][0, 1:]])
    assert C.close(ys, rs["ystar"][:, 0]) <= 1e-12


@pytest.mark.parametrize("branch", ["snp", "gblup"])
def test_reference_level_invariance(branch):
    """Permuted level codes put another level first: under snp another reference level.  y*, ebv, fitness and
    the SNP effects stay; the level effects move by a constant under snp and are permuted under gblup."""
    pn = G.panel()
    T, V = pn["splits"][129, 64]
    L = 18
    g = G.make_groups(R.N_ANIMALS, L, T)
    perm = (7 * np.arange(L) + 5) % L          # a permutation (7 and 18 are coprime) that moves level 0
    a = G.group_ref(pn["genomes"][64], T, V, pn["geno"], pn["pheno"], None, g, H2, branch)
    b = G.group_ref(pn["genomes"][64], T, V, pn["geno"], pn["pheno"], None, perm[g], H2, branch)
    for f in ("ystar", "ebv", "fitness", "effects", "intercept", "center"):
        assert C.close(b[f], a[f]) <= 1e-10, f
    moved = b["group_effects"][:, perm] - a["group_effects"]
    if branch == "gblup":
        assert C.close(moved, np.zeros_like(moved)) <= 1e-10
    else:
        assert np.ptp(moved) <= 1e-10 * max(1.0, np.max(np.abs(a["group_effects"])))


def _conditions():
    pn = G.panel()
    for name in G.DESIGNS:
        for s in G.DESIGN_SPLITS[name]:
            for k, br in [(64, "snp"), (332, "gblup")] + [(k, "snp") for k in G.snp_keys(s[0])[:1]]:
                yield name, s, k, br, pn


def test_restatement_error_and_condition():
    """float64 against longdouble at HOST_TOL, cond(G) <= COND_MAX, for every design of the GPU tests."""
    worst, cond = 0.0, 0.0
    for name, s, k, br, pn in _conditions():
        T, _ = pn["splits"][s]
        cov, g = G.design_inputs(name, s)
        r64, rld = G.gls_pair(pn["genomes"][k], T, pn["geno"], pn["pheno"], cov, g, H2, br)
        assert np.all(np.isfinite(r64["b"]))
        worst = max(worst, C.close(r64["b"], rld["b"].astype(np.float64)), C.close(r64["ystar"], rld["ystar"].astype(np.float64)))
        cond = max(cond, float(np.linalg.cond(r64["G"])))
    print("\nGROUP host: float64 vs longdouble %.3e, worst cond(G) %.3e" % (worst, cond))
    assert worst <= G.HOST_TOL and cond <= G.COND_MAX


def test_limit_design_has_127_and_128_columns():
    pn = G.panel()
    T, _ = pn["splits"][257, 70]
    cov, g = G.design_inputs("L113c15", (257, 70))
    assert G.expand(cov, g, T, "snp")[0].shape[1] == 127 and G.expand(cov, g, T, "gblup")[0].shape[1] == G.MAX_FIXED


# ---------------------------------------------------------------------------------------------
# PanelModel with a class factor
# ---------------------------------------------------------------------------------------------
def _model(levels, **kw):
    from tblup_amd.model import PanelModel
    L = len(levels)
    return PanelModel([0, 2, 5], [1.0, 0.5, 1.5], [[0.1, -0.2, 0.3], [0.0, 0.4, -0.1]], [0.5, -1.0], 0.4, "snp", 0.25,
                      group_levels=levels, group_effects=np.arange(2.0 * L).reshape(2, L) / 7,
                      group_center=np.full(L, 1.0 / L), **kw)


@pytest.mark.parametrize("levels", [np.array([2, 5, 11]), np.array(["east", "north", "west"])])
def test_panel_model_groups_predict_adjust(levels):
    m = _model(levels)
    rng = np.random.default_rng(1)
    geno = rng.integers(0, 3, (5, 8))
    other = 7 if levels.dtype.kind == "i" else "south"
    labels = np.array([levels[2], levels[0], other, levels[1], levels[2]])
    plain = m.predict(geno)
    got = m.predict(geno, groups=labels)
    z = (labels[:, None] == levels[None, :]).astype(float)
    want = plain + m.group_effects @ (z - m.group_center).T
    known = np.array([True, True, False, True, True])
    np.testing.assert_allclose(got[:, known], want[:, known], rtol=0, atol=1e-14)
    assert np.all(np.isnan(got[:, ~known]))
    y = rng.standard_normal((5, 2))
    ys = m.adjust(y, groups=labels)
    np.testing.assert_allclose(ys[known], (y - (want - plain).T)[known], rtol=0, atol=1e-14)
    assert np.all(np.isnan(ys[~known]))
    assert m.n_levels == 3 and m.n_covariates == 0
    with pytest.raises(ValueError):
        m.predict(geno, groups=labels[:-1])
    with pytest.raises(ValueError):
        m.predict(geno, covariates=np.zeros((5, 1)))          # fitted without covariates


def test_panel_model_groups_with_covariates():
    levels = np.array([1, 2, 3])
    m = _model(levels, cov_effects=[[1.0, 2.0], [0.5, -1.0]], cov_center=[0.1, 0.2])
    geno = np.random.default_rng(2).integers(0, 3, (4, 8))
    q = np.random.default_rng(3).standard_normal((4, 2))
    lab = np.array([3, 1, 2, 2])
    both = m.predict(geno, covariates=q, groups=lab)
    np.testing.assert_allclose(both, m.predict(geno, covariates=q) + m.predict(geno, groups=lab) - m.predict(geno),
                               rtol=0, atol=1e-13)


def test_panel_model_groups_validation():
    from tblup_amd.model import PanelModel
    base = dict(indices=[0], center=[1.0], effects=[[0.1]], intercept=[0.0])
    with pytest.raises(ValueError):
        PanelModel(**base, group_levels=[1, 2])                                       # the three come together
    with pytest.raises(ValueError):
        PanelModel(**base, group_levels=[2, 1], group_effects=[[0.0, 1.0]], group_center=[0.5, 0.5])   # not sorted
    with pytest.raises(ValueError):
        PanelModel(**base, group_levels=[1, 2], group_effects=[[0.0, 1.0, 2.0]], group_center=[0.5, 0.5])
    m = PanelModel(**base)
    assert m.group_levels is None and m.n_levels == 0
    with pytest.raises(ValueError):
        m.predict(np.zeros((2, 3), dtype=int), groups=[1, 1])


@pytest.mark.parametrize("levels", [np.array([2, 5, 11]), np.array(["east", "north", "west"])])
def test_panel_model_groups_save_load(tmp_path, levels):
    from tblup_amd.model import PanelModel
    m = _model(levels, cov_effects=[[1.0], [2.0]], cov_center=[0.3])
    path = str(tmp_path / "m.npz")
    m.save(path)
    r = PanelModel.load(path)
    for f in ("indices", "center", "effects", "intercept", "cov_effects", "cov_center", "group_levels", "group_effects",
              "group_center"):
        np.testing.assert_array_equal(getattr(r, f), getattr(m, f), err_msg=f)
    assert r.group_levels.dtype.kind == levels.dtype.kind and (r.h2, r.branch, r.fitness) == (m.h2, m.branch, m.fitness)


def test_file_saved_without_groups_loads_unchanged(tmp_path):
    from tblup_amd.model import PanelModel
    m = PanelModel([0, 2], [1.0, 0.5], [[0.1, -0.2]], [0.5], 0.4, "gblup", 0.5, cov_effects=[[1.0]], cov_center=[0.0])
    path = str(tmp_path / "old.npz")
    m.save(path)
    with np.load(path) as z:
        assert not any(k.startswith("group_") for k in z.files)
    r = PanelModel.load(path)
    assert r.group_levels is None and r.group_effects is None and r.group_center is None
    np.testing.assert_array_equal(r.cov_effects, m.cov_effects)
    # a file as the parent wrote it: exactly these keys
    np.savez(str(tmp_path / "older.npz"), indices=m.indices, center=m.center, effects=m.effects, intercept=m.intercept,
             h2=np.float64(0.4), branch=np.array("gblup"), fitness=np.float64(0.5))
    o = PanelModel.load(str(tmp_path / "older.npz"))
    assert o.cov_effects is None and o.group_levels is None
    np.testing.assert_array_equal(o.predict(np.ones((2, 3), dtype=int)), m.predict(np.ones((2, 3), dtype=int)))


# ---------------------------------------------------------------------------------------------
# the binding
# ---------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_and_the_limits():
    import re
    from tblup_amd import _native
    from tblup_amd.engine import GpuBlupEngine
    assert _native.MAX_FIXED == 128 and _native.MAX_COV == 16
    assert len(_native.SIGNATURES["tblup_fit_group_batch"][1]) == 20
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tblup_gpu.h")).read()
    assert re.search(r"int tblup_fit_group_batch\(", header) and "#define TBLUP_MAX_FIXED 128" in header
    lib = _native.load()
    assert hasattr(lib, "tblup_fit_group_batch")
    GpuBlupEngine._no_groups(None, "evaluate()")
    with pytest.raises(ValueError, match="groups"):
        GpuBlupEngine._no_groups([1, 2], "evaluate()")
