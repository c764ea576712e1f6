"""Reliabilities of predicted breeding values (tblup_reliability_batch, k_reliab) on the GPU, against
the float64 restatement of tests/reliability_ref.py (itself within 1e-11 of a longdouble computation:
tests/test_reliability_host.py).

Panel: 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64), (257, 70), the
genomes of tests/model_ref.py plus one of k = 300; a deeper panel (700 x 800, n_T = 520, k = 513:
5 tile columns in either form).

  A  against rel_ref over all animals: auto branch (ragged batch: kernel form; one genome at a time:
     SNP form), forced gblup, forced snp at n_T < k <= n and k > n, the deeper panel in both forms
  B  TBLUP_FORM=1 against TBLUP_FORM=2; TBLUP_PAD_FIRST=0; TBLUP_RELIAB_LDS=0 (the right-hand sides
     in the workspace instead of LDS: the same bits)
  C  arbitrary animal lists (n_pred around 64, 256 and the slab width 16): the same bits twice, every
     animal's value identical across lists and equal to the whole-herd call's
  D  1 to 4 traits and another phenotype: the same bits
  E  TBLUP_WORKSPACE_MB=1, TBLUP_SOLVE_CHAIN / TBLUP_SOLVE_PULL: the same bits; fitness and models
     bit-equal to evaluate's and fit's
  F  a monomorphic panel (NaN, no error), out-of-range animals and indices, a context without a panel,
     an empty animal list
  G  BlupParallelEvaluator.reliability / fit_models(reliability_of=)

Tolerance: the project's 1e-9 (EBV_RTOL) as an absolute difference -- reliabilities live in [0, 1].
Each group prints the largest error it saw (pytest -s); the printed figures are no thresholds.
"""
import ctypes

import numpy as np
import pytest

from tests import model_ref as R
from tests import reliability_ref as Q
from tblup_amd._native import RELIAB_SLAB as W
from tests.test_gpu_model import _animal_list, _engine

pytestmark = pytest.mark.gpu
K300 = Q.K300

H2 = Q.H2
TOL = 1e-9
N, P = R.N_ANIMALS, R.N_SNPS
HERD = np.arange(N)


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def check(self, got, ref, name):
        assert got.shape == ref.shape, name
        assert np.all(np.isfinite(got)), name
        err = float(np.max(np.abs(got - ref)))
        self.v = max(self.v, err)
        assert err <= TOL, name

    def show(self):
        print("\nRELIABILITY %s: worst max abs err %.3e" % (self.label, self.v))


@pytest.fixture(scope="module")
def eng(gpu):
    pn = Q.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    pn = Q.panel()
    genomes = [pn["genomes"][k] for k in Q.A_KEYS]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        batch = eng.reliability(genomes, T, V, H2, HERD)
        assert batch.shape == (len(genomes), N)
        for i, k in enumerate(Q.A_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            w.check(batch[i], Q.case_ref(name), name + " (batch)")
            w.check(eng.reliability([genomes[i]], T, V, H2, HERD)[0], Q.case_ref(name), name + " (alone)")
    w.show()


def test_a_forced_gblup(eng):
    pn = Q.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        genomes = [pn["genomes"][k] for k in R.GBLUP_KS]
        got = eng.reliability(genomes, T, V, H2, HERD, branch="gblup")
        for i, k in enumerate(R.GBLUP_KS):
            name = "gblup-%d-%d-%s" % (s + (k,))
            w.check(got[i], Q.case_ref(name), name)
    w.show()


def test_a_forced_snp_dual(eng):
    """Forced snp at n_T < k <= n and k > n (the kernel form under the train rows' centre)."""
    pn = Q.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in Q.A_KEYS if not isinstance(k, str) and k > s[0]]
        assert any(k > N for k in ks) and (any(k <= N for k in ks))
        got = eng.reliability([pn["genomes"][k] for k in ks], T, V, H2, HERD, branch="snp")
        for i, k in enumerate(ks):
            name = "snp-%d-%d-%s" % (s + (k,))
            w.check(got[i], Q.case_ref(name), name)
    w.show()


def test_a_deeper_panel(gpu):
    """n_T = 520, k = 513: five tile columns, in the SNP form (auto) and in the kernel form."""
    dp = Q.deep_panel()
    herd = np.arange(Q.DEEP_N)
    w = _Worst("A deep")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.reliability([dp["genome"]], dp["train"], dp["valid"], H2, herd)[0]
            w.check(got[form], Q.deep_ref(), "form " + form)
    assert np.max(np.abs(got["1"] - got["2"])) <= TOL
    w.show()


# ---------------------------------------------------------------------------------------------
# B. forms, padding, where V lives
# ---------------------------------------------------------------------------------------------
def _snp_keys():
    return [k for k in R.KS if k <= 200] + ["dup", "neg"]


def test_b_forms_agree(gpu):
    pn = Q.panel()
    w = _Worst("B forms")
    keys = _snp_keys()
    genomes = [pn["genomes"][k] for k in keys]
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            for s in R.SPLITS:
                T, V = pn["splits"][s]
                got[form, s] = e.reliability(genomes, T, V, H2, HERD)
    for s in R.SPLITS:
        for i, k in enumerate(keys):
            name = "auto-%d-%d-%s" % (s + (k,))
            w.check(got["1", s][i], Q.case_ref(name), name + " form 1")
            w.check(got["2", s][i], Q.case_ref(name), name + " form 2")
            w.check(got["1", s][i], got["2", s][i], name + " form 1 vs 2")
    w.show()


def test_b_trailing_padding(gpu):
    pn = Q.panel()
    w = _Worst("B PAD_FIRST=0")
    keys = _snp_keys()
    genomes = [pn["genomes"][k] for k in keys]
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_PAD_FIRST": "0", "TBLUP_FORM": "2"}) as e:
        for s in R.SPLITS:
            T, V = pn["splits"][s]
            got = e.reliability(genomes, T, V, H2, HERD)
            for i, k in enumerate(keys):
                name = "auto-%d-%d-%s" % (s + (k,))
                w.check(got[i], Q.case_ref(name), name)
                w.check(e.reliability([genomes[i]], T, V, H2, HERD)[0], Q.case_ref(name), name + " (alone)")
    w.show()


def test_b_workspace_right_hand_sides_same_bits(eng):
    """TBLUP_RELIAB_LDS=0 keeps V in the workspace (the path of systems above 1024 rows): the same bits
    in both forms."""
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, 65, 129, 200, "dup", K300)]
    mixed = snp + [pn["genomes"][400]]
    an = _animal_list((257, 70), 257)
    # (with a 1 MB workspace budget the list is walked a few slabs per launch)
    for env in ({"TBLUP_RELIAB_LDS": "0"}, {"TBLUP_RELIAB_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for genomes in (snp, mixed):
                for animals in (HERD, an):
                    np.testing.assert_array_equal(e.reliability(genomes, T, V, H2, animals),
                                                  eng.reliability(genomes, T, V, H2, animals))


# ---------------------------------------------------------------------------------------------
# C. arbitrary animal lists
# ---------------------------------------------------------------------------------------------
C_NPRED = sorted({1, 2, 63, 64, 65, 257, 331, W - 1, W, W + 1, 2 * W + 1})


def test_c_arbitrary_animals(eng):
    pn = Q.panel()
    keys = [2, 65, 200, 400, "dup"]
    w = _Worst("C")
    for s in ((129, 64), (257, 70)):
        T, V = pn["splits"][s]
        genomes = [pn["genomes"][k] for k in keys]
        snp_form = [genomes[1], genomes[4]]               # without k = 400: an SNP-form batch
        herd = eng.reliability(genomes, T, V, H2, HERD)
        herd_snp = eng.reliability(snp_form, T, V, H2, HERD)
        for i, k in enumerate(keys):
            w.check(herd[i], Q.case_ref("auto-%d-%d-%s" % (s + (k,))), str((s, k)))
        for n_pred in C_NPRED:
            an = _animal_list(s, n_pred)
            if n_pred >= 65:
                assert set(an) & set(T) and set(an) & set(V) and set(an) - set(T) - set(V)
            got = eng.reliability(genomes, T, V, H2, an)
            got_snp = eng.reliability(snp_form, T, V, H2, an)
            assert got.shape == (len(genomes), n_pred)
            np.testing.assert_array_equal(got, eng.reliability(genomes, T, V, H2, an))     # the same bits twice
            np.testing.assert_array_equal(got_snp, eng.reliability(snp_form, T, V, H2, an))
            # every animal's value is the whole-herd call's, wherever it stands and whatever n_pred is
            np.testing.assert_array_equal(got, herd[:, an], err_msg=str((s, n_pred)))
            np.testing.assert_array_equal(got_snp, herd_snp[:, an], err_msg=str((s, n_pred)))
    w.show()


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits_and_phenotypes_do_not_matter(gpu):
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    an = _animal_list((129, 64), 65)
    with _engine(pn["geno"], pn["pheno"]) as e:
        single = [e.reliability(b, T, V, H2, an) for b in batches]
    with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, 3])) as e:
        for b, ref in zip(batches, single):
            np.testing.assert_array_equal(e.reliability(b, T, V, H2, an), ref)
    for nt in (1, 2, 3, 4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
            for b, ref in zip(batches, single):
                got = e.reliability(b, T, V, H2, an)
                assert got.shape == (len(b), len(an))
                np.testing.assert_array_equal(got, ref, err_msg=str(nt))
                models, rel = e.fit(b, T, V, H2, reliability_of=an)
                np.testing.assert_array_equal(rel, ref, err_msg=str(nt))
                assert all(m.effects.shape == (nt, len(g)) for m, g in zip(models, b))


# ---------------------------------------------------------------------------------------------
# E. chunking, solve kernels, and the other outputs of the same pass
# ---------------------------------------------------------------------------------------------
def _same_models(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("indices", "center", "effects", "intercept"):
            np.testing.assert_array_equal(getattr(x, f), getattr(y, f), err_msg=f)
        np.testing.assert_array_equal(x.fitness, y.fitness)


def test_e_chunked_workspace_is_identical(eng, monkeypatch):
    from tblup_amd.engine import GpuBlupEngine
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    genomes = [pn["genomes"][k] for k in Q.A_KEYS] * 2
    an = HERD[::-1].copy()
    ref = eng.reliability(genomes, T, V, H2, an)
    ref_snp = eng.reliability(genomes[:8], T, V, H2, an)
    monkeypatch.setenv("TBLUP_WORKSPACE_MB", "1")
    with GpuBlupEngine(pn["geno"], pn["pheno"]) as e:
        np.testing.assert_array_equal(e.reliability(genomes, T, V, H2, an), ref)
        np.testing.assert_array_equal(e.reliability(genomes[:8], T, V, H2, an), ref_snp)


def test_e_solve_kernels_are_identical(gpu):
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, 2, 63, 64, 65, 127, 128, 129, 200, "dup", "neg")]   # SNP form
    mixed = snp + [pn["genomes"][400]]                                                       # kernel form
    got = {}
    for env in ({"TBLUP_SOLVE_CHAIN": "0"}, {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "1"},
                {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "0"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            got[tuple(env.values())] = (e.reliability(snp, T, V, H2, HERD), e.reliability(mixed, T, V, H2, HERD))
    base = got["0",]
    for val in got.values():
        np.testing.assert_array_equal(val[0], base[0])
        np.testing.assert_array_equal(val[1], base[1])


def test_e_forced_expiry_keeps_models_and_reliabilities(gpu):
    """fit(reliability_of=) on a context whose first chained solve gives up a wait
    (TBLUP_CHAIN_DEBUG="1000,20000,1"): the effects and reliability launches run once, beside the
    first pass, and the recovery pass re-solves for the fitness only -- models, fitnesses and
    reliabilities bit-equal to a clean context's, chain_recoveries = 1.  SNP form with three tile
    columns (k in 257..331 on split (257, 70)), so that a wait can expire."""
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    rng = np.random.default_rng(331257)
    genomes = [rng.choice(P, int(k), replace=False) for k in rng.integers(257, 332, 4)]
    an = HERD[::-3].copy()
    with _engine(pn["geno"], pn["pheno"]) as e:
        ref_models, ref_rel = e.fit(genomes, T, V, H2, reliability_of=an)
        assert e.chain_recoveries() == 0
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_CHAIN_DEBUG": "1000,20000,1"}) as e:
        models, rel = e.fit(genomes, T, V, H2, reliability_of=an)
        rec = e.chain_recoveries()
    print("\nforced expiry in fit(reliability_of=): chain_recoveries", rec)
    _same_models(models, ref_models)
    np.testing.assert_array_equal(rel, ref_rel)
    assert np.all(np.isfinite(ref_rel)) and np.all(np.isfinite([m.fitness for m in ref_models]))
    assert rec == 1


def test_e_one_pass_outputs(eng):
    """fit(reliability_of=) returns fit()'s models and reliability()'s array, bit for bit; the entry's
    fitness is evaluate()'s."""
    from tblup_amd import _native
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    an = _animal_list((129, 64), 65)
    for genomes in ([pn["genomes"][k] for k in (63, 64, 127)], [pn["genomes"][k] for k in Q.A_KEYS]):
        models, rel = eng.fit(genomes, T, V, H2, reliability_of=an)
        _same_models(models, eng.fit(genomes, T, V, H2))
        np.testing.assert_array_equal(rel, eng.reliability(genomes, T, V, H2, an))
        fit = eng.evaluate(genomes, T, V, H2)
        np.testing.assert_array_equal([m.fitness for m in models], fit)
        # the C entry with a fitness buffer and no model triple
        from tblup_amd.engine import concat_genomes
        idx, off = concat_genomes(genomes)
        a64 = np.ascontiguousarray(an, dtype=np.int64)
        f2, r2 = np.empty(len(genomes)), np.empty((len(genomes), len(an)))
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        sid = eng.split_id(T, V)
        rc = eng._lib.tblup_reliability_batch(eng._ctx, sid, a64.ctypes.data_as(i64), len(a64), idx.ctypes.data_as(i64),
                                              off.ctypes.data_as(i64), len(genomes), H2, 0, f2.ctypes.data_as(f64),
                                              None, None, None, r2.ctypes.data_as(f64))
        assert rc == 0
        np.testing.assert_array_equal(f2, fit)
        np.testing.assert_array_equal(r2, rel)
        # a partial model triple is an argument error
        rc = eng._lib.tblup_reliability_batch(eng._ctx, sid, a64.ctypes.data_as(i64), len(a64), idx.ctypes.data_as(i64),
                                              off.ctypes.data_as(i64), len(genomes), H2, 0, None,
                                              f2.ctypes.data_as(f64), None, None, r2.ctypes.data_as(f64))
        assert rc != 0 and rc not in (_native.ERR_STATE, _native.ERR_INDEX)


# ---------------------------------------------------------------------------------------------
# F. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_f_monomorphic_panel_gives_nan(gpu):
    pn = Q.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            rel = e.reliability(genomes, T, V, H2, HERD, branch=br)
            assert np.all(np.isnan(rel[:2]))
            assert np.all(np.isfinite(rel[2]))
            ref = Q.rel_ref(genomes[2], T, geno, H2, br)
            assert np.max(np.abs(rel[2] - ref)) <= TOL


def test_f_errors(eng):
    from tblup_amd._native import TblupError, TblupIndexError
    pn = Q.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    for bad in (N, -1):
        with pytest.raises(TblupError):
            eng.reliability(g, T, V, H2, [0, bad])
    for bad in (P, -P - 1):
        with pytest.raises(TblupIndexError):
            eng.reliability(g + [np.array([3, bad, 5])], T, V, H2, HERD)
    ok = eng.reliability([np.array([3, -P, P - 1])], T, V, H2, HERD)      # the bounds themselves are valid
    ref = Q.rel_ref(np.array([3, 0, P - 1]), T, pn["geno"], H2)
    assert np.max(np.abs(ok[0] - ref)) <= TOL
    empty = eng.reliability(g * 3, T, V, H2, [])
    assert empty.shape == (3, 0)
    models, rel = eng.fit(g * 3, T, V, H2, reliability_of=[])
    assert rel.shape == (3, 0) and len(models) == 3


def test_f_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        out = np.zeros(1)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_reliability_batch(ctx, 0, one.ctypes.data_as(i64), 1, one.ctypes.data_as(i64),
                                         off.ctypes.data_as(i64), 1, 0.4, 0, None, None, None, None,
                                         out.ctypes.data_as(f64))
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# G. evaluator level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("removed", [(), (5, 17, 301, 599)])
def test_g_evaluator_reliability(gpu, tmp_path, removed):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = Q.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, H2, False)
    rem.removed = np.array(removed, dtype=np.float64)
    with E.BlupParallelEvaluator(gp, pp, H2, snp_remover=rem) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        an = np.concatenate([ev.testing_indices[:9], ev.training_indices[:5]])
        rel = ev.reliability(pop, an)
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        np.testing.assert_array_equal(rel, ev.engine.reliability(genomes, train, ev.testing_indices, H2, an))
        for i, g in enumerate(genomes):
            ref = Q.rel_ref(g, train, pn["geno"], H2)[an]
            assert np.max(np.abs(rel[i] - ref)) <= TOL
        models, rel2 = ev.fit_models(pop, reliability_of=an)
        np.testing.assert_array_equal(rel2, rel)
        _same_models(models, ev.fit_models(pop))
        own = ev.reliability(pop, an, final=False)
        np.testing.assert_array_equal(own, ev.engine.reliability([i.genome for i in pop], ev.training_indices,
                                                                 ev.validation_indices, H2, an))
