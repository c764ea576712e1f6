"""Leave-one-out cross-validation of fitted models (tblup_loo_batch, k_loo, k_loo_fitness) on the GPU, against
the float64 restatement of tests/loo_ref.py (itself within 1e-9 of n_T brute-force refits, and with
min(1 - h_tt) >= 0.05 on every case used here: tests/test_loo_host.py).

Panel: 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64), (257, 70) -- 127, 128 and 129
straddle the tile edge, 257 leaves a last slab of one animal and three block rows -- and the deeper panel of
tests/reliability_ref.py (700 x 800, n_T = 520, k = 513: five tile columns in either form).

  A  pred, leverage, press and fitness against loo_ref: a ragged batch (kernel form), one genome at a time (the
     SNP form where k fits), forced gblup, forced snp at n_T < k <= n and k > n, the deeper panel in both forms;
     one brute-force spot check on the GPU result itself
  B  TBLUP_FORM=1 against TBLUP_FORM=2; TBLUP_PAD_FIRST=0; TBLUP_RELIAB_LDS=0 (the same bits as LDS)
  C  the same bits: twice, a genome alone or in a batch of 7, TBLUP_WORKSPACE_MB=1; eval_fitness is evaluate()'s;
     evaluate / fit / reliability before and after loo on one engine
  D  1 to 4 traits: the leverages do not move, a trait's pred is the single-trait engine's, the fitness is the mean
  E  a monomorphic panel (NaN, no error), k = 1, out-of-range indices, a context without a panel
  F  BlupParallelEvaluator.loo

Tolerances: the project's 1e-9 (EBV_RTOL) -- pred relative to max |y_T|, leverage and fitness absolute (both
live in [0, 1]), PRESS relative to n_T max |y_T|^2 (a sum of n_T squares of values that carry pred's error).
Each group prints the largest error it saw (pytest -s); the printed figures are no thresholds.
"""
import ctypes

import numpy as np
import pytest

from tests import loo_ref as Z
from tests import model_ref as R
from tests import reliability_ref as Q
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = Z.H2
TOL = 1e-9
N, P = R.N_ANIMALS, R.N_SNPS


class _Worst:
    def __init__(self, label):
        self.label = label
        self.v = {"pred": 0.0, "leverage": 0.0, "press": 0.0, "fitness": 0.0}

    def _one(self, what, got, ref, scale, name):
        got, ref = np.asarray(got), np.asarray(ref)
        assert got.shape == ref.shape, (name, what)
        assert np.all(np.isfinite(got)), (name, what)
        err = float(np.max(np.abs(got - ref))) / scale
        self.v[what] = max(self.v[what], err)
        assert err <= TOL, (name, what, err)

    def check(self, res, i, ref, yT, name, trait=None):
        """Model i of a LooResult against a loo_ref dict (trait: the trait plane of a multi-trait result)."""
        ymax = float(np.max(np.abs(yT)))
        pred = res.pred[i] if trait is None else res.pred[i, trait]
        press = res.press[i] if trait is None else res.press[i, trait]
        self._one("pred", pred, ref["pred"], ymax, name)
        self._one("press", press, ref["press"], len(yT) * ymax * ymax, name)
        if res.leverage is not None:
            self._one("leverage", res.leverage[i], ref["leverage"], 1.0, name)
        if trait is None:
            self._one("fitness", res.fitness[i], ref["fitness"], 1.0, name)

    def show(self):
        print("\nLOO %s: worst errors pred %.3e (rel. max |y_T|), leverage %.3e, press %.3e, fitness %.3e"
              % (self.label, self.v["pred"], self.v["leverage"], self.v["press"], self.v["fitness"]))


def _same(a, b):
    """Two LooResults, bit for bit."""
    for f in ("fitness", "pred", "press", "eval_fitness", "train"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert (a.leverage is None) == (b.leverage is None)
    if a.leverage is not None:
        np.testing.assert_array_equal(a.leverage, b.leverage, err_msg="leverage")


def _row(res, i):
    """Model i of a LooResult as a tuple of arrays."""
    return (res.fitness[i], res.pred[i], res.press[i], res.eval_fitness[i]) + \
        (() if res.leverage is None else (res.leverage[i],))


def _same_row(a, i, b, j, msg=""):
    for x, y in zip(_row(a, i), _row(b, j)):
        np.testing.assert_array_equal(x, y, err_msg=msg)


@pytest.fixture(scope="module")
def eng(gpu):
    pn = Z.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_ragged_batch(eng):
    """k = 332 and 400 are gblup under auto, so the batch runs in the kernel form, both branches in it."""
    pn = Z.panel()
    genomes = [pn["genomes"][k] for k in Z.RAGGED]
    w = _Worst("A ragged batch")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        res = eng.loo(genomes, T, V, H2, return_leverage=True)
        assert res.pred.shape == (len(genomes), s[0]) and res.leverage.shape == (len(genomes), s[0])
        np.testing.assert_array_equal(res.train, T)
        for i, k in enumerate(Z.RAGGED):
            name = "auto-%d-%d-%s" % (s + (k,))
            w.check(res, i, Z.case_ref(name), pn["pheno"][T], name)
    w.show()


def test_a_one_at_a_time(eng):
    """One genome per call: the SNP form wherever k fits the padded train rows, else the kernel form."""
    pn = Z.panel()
    w = _Worst("A one at a time")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        for k in Z.SINGLE:
            name = "auto-%d-%d-%s" % (s + (k,))
            res = eng.loo([pn["genomes"][k]], T, V, H2, return_leverage=True)
            w.check(res, 0, Z.case_ref(name), pn["pheno"][T], name)
            plain = eng.loo([pn["genomes"][k]], T, V, H2)
            assert plain.leverage is None
            np.testing.assert_array_equal(plain.pred, res.pred)
    w.show()


def test_a_forced_branches(eng):
    """Forced gblup at k <= n; forced snp at n_T < k <= n and at k > n (the kernel form under the train centre)."""
    pn = Z.panel()
    w = _Worst("A forced branches")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        for br, keys in (("gblup", Z.GBLUP_KS), ("snp", Z.SNP_KS)):
            res = eng.loo([pn["genomes"][k] for k in keys], T, V, H2, branch=br, return_leverage=True)
            for i, k in enumerate(keys):
                name = "%s-%d-%d-%s" % ((br,) + s + (k,))
                w.check(res, i, Z.case_ref(name), pn["pheno"][T], name)
    w.show()


def test_a_deeper_panel(gpu):
    """n_T = 520, k = 513: five tile columns -- the three-register ring wraps and the kernel form's skipped steps
    cross block rows -- in the SNP form (auto) and in the kernel form."""
    dp = Q.deep_panel()
    w = _Worst("A deep")
    got = {}
    yT = dp["pheno"][dp["train"]]
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.loo([dp["genome"]], dp["train"], dp["valid"], H2, return_leverage=True)
            w.check(got[form], 0, Z.deep_ref(), yT, "form " + form)
    assert np.max(np.abs(got["1"].pred - got["2"].pred)) <= TOL * np.max(np.abs(yT))
    assert np.max(np.abs(got["1"].leverage - got["2"].leverage)) <= TOL
    w.show()


def test_a_brute_force_spot_check(eng):
    """The GPU result itself against refits without each animal: split (127, 5), one genome per branch."""
    pn = Z.panel()
    T, V = pn["splits"][127, 5]
    ymax = float(np.max(np.abs(pn["pheno"][T])))
    for k in (Z.K40, 400):
        res = eng.loo([pn["genomes"][k]], T, V, H2)
        brute = Z.loo_brute(pn["genomes"][k], T, pn["geno"], pn["pheno"], H2)
        err = float(np.max(np.abs(res.pred[0] - brute))) / ymax
        print("\nLOO A brute force k=%d: max rel err against 127 refits %.3e" % (k, err))
        assert err <= TOL, k
        np.testing.assert_array_equal(res.residuals(pn["pheno"])[0], pn["pheno"][T] - res.pred[0])


# ---------------------------------------------------------------------------------------------
# B. forms, padding, where V lives
# ---------------------------------------------------------------------------------------------
B_KEYS = [1, Z.K40, 65, 128, 129, 200, "dup", "neg"]


def test_b_forms_agree(gpu):
    pn = Z.panel()
    w = _Worst("B forms")
    genomes = [pn["genomes"][k] for k in B_KEYS]
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            for s in R.SPLITS:
                T, V = pn["splits"][s]
                got[form, s] = e.loo(genomes, T, V, H2, return_leverage=True)
    for s in R.SPLITS:
        yT = pn["pheno"][pn["splits"][s][0]]
        ymax = float(np.max(np.abs(yT)))
        for i, k in enumerate(B_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            ref = Z.case_ref(name) if k in Z.RAGGED + Z.SINGLE else \
                Z.loo_ref(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], H2)
            w.check(got["1", s], i, ref, yT, name + " form 1")
            w.check(got["2", s], i, ref, yT, name + " form 2")
            assert np.max(np.abs(got["1", s].pred[i] - got["2", s].pred[i])) <= TOL * ymax, name
            assert np.max(np.abs(got["1", s].leverage[i] - got["2", s].leverage[i])) <= TOL, name
            assert abs(got["1", s].fitness[i] - got["2", s].fitness[i]) <= TOL, name
    w.show()


def test_b_trailing_padding(gpu):
    pn = Z.panel()
    w = _Worst("B PAD_FIRST=0")
    keys = [1, Z.K40, 129, 200, "neg"]
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_PAD_FIRST": "0", "TBLUP_FORM": "2"}) as e:
        for s in R.SPLITS:
            T, V = pn["splits"][s]
            res = e.loo([pn["genomes"][k] for k in keys], T, V, H2, return_leverage=True)
            for i, k in enumerate(keys):
                name = "auto-%d-%d-%s" % (s + (k,))
                w.check(res, i, Z.case_ref(name), pn["pheno"][T], name)
    w.show()


def test_b_workspace_right_hand_sides_same_bits(eng):
    """TBLUP_RELIAB_LDS=0 keeps V in the workspace (the path of systems above 1024 rows): the same bits in both
    forms, also when a 1 MB budget walks the slabs a few per launch."""
    pn = Z.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, 65, 129, 200, "dup", Z.K300)]
    mixed = snp + [pn["genomes"][400]]
    for env in ({"TBLUP_RELIAB_LDS": "0"}, {"TBLUP_RELIAB_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for genomes in (snp, mixed):
                _same(e.loo(genomes, T, V, H2, return_leverage=True), eng.loo(genomes, T, V, H2, return_leverage=True))


# ---------------------------------------------------------------------------------------------
# C. the same bits
# ---------------------------------------------------------------------------------------------
def test_c_twice_alone_and_in_a_batch(eng):
    pn = Z.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, Z.K40, 65, 129, 200, "dup", Z.K300)]      # 7 genomes, SNP form
    mixed = snp[:6] + [pn["genomes"][400]]                                          # 7 genomes, kernel form
    for genomes in (snp, mixed):
        a = eng.loo(genomes, T, V, H2, return_leverage=True)
        _same(a, eng.loo(genomes, T, V, H2, return_leverage=True))
        rev = eng.loo(genomes[::-1], T, V, H2, return_leverage=True)
        for i in range(len(genomes)):
            _same_row(a, i, rev, len(genomes) - 1 - i, "reversed %d" % i)
    a = eng.loo(snp, T, V, H2, return_leverage=True)
    for i in range(len(snp)):      # alone the system has fewer leading padding tiles, exact zeros in every contraction
        _same_row(eng.loo([snp[i]], T, V, H2, return_leverage=True), 0, a, i, "alone %d" % i)
    k_inb = eng.loo(mixed, T, V, H2, return_leverage=True)      # kernel form: the system size is n_T whatever the batch
    _same_row(eng.loo([mixed[-1]], T, V, H2, return_leverage=True), 0, k_inb, 6, "kernel form alone")


def test_c_chunked_workspace_is_identical(eng, monkeypatch):
    from tblup_amd.engine import GpuBlupEngine
    pn = Z.panel()
    T, V = pn["splits"][257, 70]
    genomes = [pn["genomes"][k] for k in Z.RAGGED] * 2
    ref = eng.loo(genomes, T, V, H2, return_leverage=True)
    ref_snp = eng.loo(genomes[:5], T, V, H2, return_leverage=True)
    monkeypatch.setenv("TBLUP_WORKSPACE_MB", "1")
    with GpuBlupEngine(pn["geno"], pn["pheno"]) as e:
        _same(e.loo(genomes, T, V, H2, return_leverage=True), ref)
        _same(e.loo(genomes[:5], T, V, H2, return_leverage=True), ref_snp)


def test_c_other_entries_do_not_move(gpu):
    """eval_fitness is evaluate()'s; evaluate, fit and reliability before and after loo on one engine return
    unchanged bits."""
    pn = Z.panel()
    T, V = pn["splits"][129, 64]
    an = np.arange(0, N, 3)
    with _engine(pn["geno"], pn["pheno"]) as e:
        for genomes in ([pn["genomes"][k] for k in (1, Z.K40, 128)], [pn["genomes"][k] for k in Z.RAGGED]):
            fit0 = e.evaluate(genomes, T, V, H2)
            models0 = e.fit(genomes, T, V, H2)
            rel0 = e.reliability(genomes, T, V, H2, an)
            res = e.loo(genomes, T, V, H2, return_leverage=True)
            np.testing.assert_array_equal(res.eval_fitness, fit0)
            np.testing.assert_array_equal(e.evaluate(genomes, T, V, H2), fit0)
            np.testing.assert_array_equal(e.reliability(genomes, T, V, H2, an), rel0)
            for m0, m1 in zip(models0, e.fit(genomes, T, V, H2)):
                for f in ("indices", "center", "effects", "intercept", "fitness"):
                    np.testing.assert_array_equal(getattr(m0, f), getattr(m1, f), err_msg=f)
            _same(e.loo(genomes, T, V, H2, return_leverage=True), res)


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits(gpu):
    pn = Z.panel()
    T, V = pn["splits"][129, 64]
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    single = {}
    for tr in range(4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, tr])) as e:
            single[tr] = [e.loo(b, T, V, H2, return_leverage=True) for b in batches]
    w = _Worst("D traits")
    for j, b in enumerate(batches):      # against the restatement, trait by trait
        for tr in (0, 3):
            for i, g in enumerate(b):
                ref = Z.loo_ref(g, T, pn["geno"], pn["Y"][:, tr], H2)
                w.check(single[tr][j], i, ref, pn["Y"][T, tr], "trait %d batch %d model %d" % (tr, j, i))
    for nt in (1, 2, 3, 4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
            for j, b in enumerate(batches):
                got = e.loo(b, T, V, H2, return_leverage=True)
                assert got.pred.shape == ((len(b), len(T)) if nt == 1 else (len(b), nt, len(T)))
                assert got.press.shape == ((len(b),) if nt == 1 else (len(b), nt))
                np.testing.assert_array_equal(got.leverage, single[0][j].leverage, err_msg=str(nt))
                per_trait = np.zeros(len(b))
                for tr in range(nt):
                    one = single[tr][j]
                    np.testing.assert_array_equal(got.pred if nt == 1 else got.pred[:, tr], one.pred, err_msg=str((nt, tr)))
                    np.testing.assert_array_equal(got.press if nt == 1 else got.press[:, tr], one.press)
                    per_trait += one.fitness
                np.testing.assert_array_equal(got.fitness, per_trait if nt == 1 else per_trait / nt, err_msg=str(nt))
                res = got.residuals(pn["Y"][:, :nt])
                assert res.shape == got.pred.shape
    w.show()


# ---------------------------------------------------------------------------------------------
# E. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_e_monomorphic_panel_gives_nan(gpu):
    pn = Z.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            res = e.loo(genomes, T, V, H2, branch=br, return_leverage=True)
            assert np.all(np.isnan(res.pred[:2])) and np.all(np.isnan(res.leverage[:2]))
            assert np.all(np.isnan(res.fitness[:2])) and np.all(np.isnan(res.press[:2]))
            ref = Z.loo_ref(genomes[2], T, geno, pn["pheno"], H2, br)
            assert np.max(np.abs(res.pred[2] - ref["pred"])) <= TOL * np.max(np.abs(pn["pheno"][T]))
            assert abs(res.fitness[2] - ref["fitness"]) <= TOL


def test_e_one_snp(eng):
    """k = 1 in every split and under either branch."""
    pn = Z.panel()
    w = _Worst("E k = 1")
    g = pn["genomes"][1]
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        for br in ("snp", "gblup"):
            res = eng.loo([g], T, V, H2, branch=br, return_leverage=True)
            w.check(res, 0, Z.loo_ref(g, T, pn["geno"], pn["pheno"], H2, br), pn["pheno"][T], str((s, br)))
    w.show()


def test_e_errors(eng):
    from tblup_amd._native import TblupIndexError
    pn = Z.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    for bad in (P, -P - 1):
        with pytest.raises(TblupIndexError):
            eng.loo(g + [np.array([3, bad, 5])], T, V, H2)
        with pytest.raises(TblupIndexError):
            eng.fit(g + [np.array([3, bad, 5])], T, V, H2)
    ok = eng.loo([np.array([3, -P, P - 1])], T, V, H2)      # the bounds themselves are valid
    ref = Z.loo_ref(np.array([3, 0, P - 1]), T, pn["geno"], pn["pheno"], H2)
    assert np.max(np.abs(ok.pred[0] - ref["pred"])) <= TOL * np.max(np.abs(pn["pheno"][T]))
    empty = eng.loo([], T, V, H2, return_leverage=True)
    assert empty.pred.shape == (0, len(T)) and empty.fitness.shape == (0,)
    for kw in ({"covariates": np.zeros((N, 1))}, {"groups": np.zeros(N, dtype=np.int64)}):
        with pytest.raises(ValueError, match="not built"):
            eng.loo(g, T, V, H2, **kw)


def test_e_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        out = np.zeros(4)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_loo_batch(ctx, 0, one.ctypes.data_as(i64), off.ctypes.data_as(i64), 1, 0.4, 0,
                                 out.ctypes.data_as(f64), out.ctypes.data_as(f64), None, None, None)
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# F. evaluator level
# ---------------------------------------------------------------------------------------------
def test_f_evaluator_loo(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = Z.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    with E.BlupParallelEvaluator(gp, pp, H2) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        genomes = [np.sort(i.genome) for i in pop]      # final=True: evaluate_testing's set-up (sorted, distinct)
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        res = ev.loo(pop, return_leverage=True)
        _same(res, ev.engine.loo(genomes, train, ev.testing_indices, H2, return_leverage=True))
        w = _Worst("F evaluator")
        for i, g in enumerate(genomes):
            w.check(res, i, Z.loo_ref(g, train, pn["geno"], pn["pheno"], H2), pn["pheno"][train], str(i))
        own = ev.loo(pop, final=False)
        _same(own, ev.engine.loo([i.genome for i in pop], ev.training_indices, ev.validation_indices, H2))
        w.show()
