"""Taking the fitted model out (tblup_fit_batch / tblup_predict_batch) on the GPU, against the
float64 restatement of the reference's model (tests/model_ref.py), the oracle's EBVs and the
evaluator's own outputs.

Panel: 331 animals (odd: the SNP-major rows k_predict reads are unaligned) x 600 SNPs; splits
(n_T, n_V) = (127, 5), (128, 2), (129, 64), (257, 70); k in {1, 2, 63, 64, 65, 127, 128, 129, 200,
332, 400} -- around the 64-SNP block, the 128-row tile and across k > n.

  A  effects, centre and intercept: auto branch (ragged batch: kernel form; one genome at a time:
     both forms), forced gblup at k <= n, forced snp at n_T < k <= n and k > n, TBLUP_FORM 1 / 2,
     TBLUP_PAD_FIRST=0, duplicate and negative indices; centre bit-equal to colsum / N
  B  fit's fitness bit-equal to evaluate's; predict(model, V) against evaluate's EBVs and the oracle
  C  prediction for arbitrary animal lists (n_pred 1 .. 331, reverse order, repeats, any split role)
  D  1 to 4 traits, each trait bit-equal to the single-trait fit of its phenotype column
  E  TBLUP_WORKSPACE_MB=1, TBLUP_SOLVE_CHAIN=0/1, TBLUP_SOLVE_PULL=0/1: the same bits
  F  a monomorphic panel (NaN, no error), out-of-range indices, a context without a panel
  G  BlupParallelEvaluator.fit_models / predict, PanelModel save / load
  H  the host entries back to back on one context, each bit-equal to the same call on a fresh context
  I  every entry's one call on a fresh context (its workspace is exactly the measured carve), bit-equal to
     the same call behind a larger one

Tolerances: EBV_RTOL = 1e-9 relative max-norm (tests/test_gpu_parity.py); effects the same 1e-9
relative to the individual's max |effect|, on cases where tests/test_model_host.py shows the
restatement itself within 1e-11 of a longdouble solve.  Each test prints the largest error it saw
(pytest -s) for PERFLOG.md; the printed figures are no thresholds.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from oracle import blup_oracle as O
from tests import model_ref as R

pytestmark = pytest.mark.gpu

H2 = R.H2
EBV_RTOL = 1e-9
EFF_RTOL = 1e-9
N, P = R.N_ANIMALS, R.N_SNPS


@contextlib.contextmanager
def _engine(geno, pheno, env=None, **kw):
    """A context created under `env` (the TBLUP_* knobs are read at context creation)."""
    from tblup_amd.engine import GpuBlupEngine
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = GpuBlupEngine(geno, pheno, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield eng
    finally:
        eng.close()


def _relmax(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, {}

    def add(self, key, x):
        self.v[key] = max(self.v.get(key, 0.0), float(x))
        return x

    def show(self):
        print("\nMODEL %s: %s" % (self.label, ", ".join("max %s %.3e" % kv for kv in sorted(self.v.items()))))


def _colsum_center(idx, rows):
    """2p as the issue defines it: the exact integer column sum divided once by the row count."""
    g = R.panel()["geno"]
    return g[np.ix_(rows, np.asarray(idx))].astype(np.int64).sum(axis=0) / float(len(rows))


def _check_model(w, name, m, ref, idx, T):
    """One single-trait PanelModel against fit_ref's dict."""
    assert m.branch == ref["branch"], name
    np.testing.assert_array_equal(m.indices, np.where(np.asarray(idx) < 0, np.asarray(idx) + P, idx), err_msg=name)
    rows = np.arange(N) if ref["branch"] == "gblup" else T
    np.testing.assert_array_equal(m.center, _colsum_center(idx, rows), err_msg=name)
    assert m.effects.shape == (1, len(idx)) and m.intercept.shape == (1,), name
    assert w.add("effects", _relmax(m.effects[0], ref["effects"])) <= EFF_RTOL, name
    if ref["branch"] == "gblup":
        assert m.intercept[0] == 0.0, name
    else:
        assert w.add("intercept", abs(m.intercept[0] - ref["intercept"]) / abs(ref["intercept"])) <= EBV_RTOL, name


@pytest.fixture(scope="module")
def eng(gpu):
    pn = R.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. effects, centre and intercept
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    """Every split x every genome: as one ragged batch (k = 400 takes gblup, so the batch runs in the
    kernel form) and one genome at a time (the SNP form wherever it gives no more tiles)."""
    pn = R.panel()
    keys = R.KS + ["dup", "neg"]
    genomes = [pn["genomes"][k] for k in keys]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        batch = eng.fit(genomes, T, V, H2)
        for i, k in enumerate(keys):
            name = "auto-%d-%d-%s" % (s + (k,))
            _check_model(w, name + " (batch)", batch[i], R.case_ref(name), genomes[i], T)
            _check_model(w, name + " (alone)", eng.fit([genomes[i]], T, V, H2)[0], R.case_ref(name), genomes[i], T)
    w.show()


def test_a_forced_gblup(eng):
    pn = R.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        genomes = [pn["genomes"][k] for k in R.GBLUP_KS]
        for i, m in enumerate(eng.fit(genomes, T, V, H2, branch="gblup")):
            name = "gblup-%d-%d-%s" % (s + (R.GBLUP_KS[i],))
            _check_model(w, name, m, R.case_ref(name), genomes[i], T)
    w.show()


def test_a_forced_snp_dual(eng):
    """Forced snp where sklearn's Ridge takes its kernel solve: n_T < k <= n (the reference's own
    branch there) and k > n."""
    pn = R.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in R.KS if k > s[0]]
        genomes = [pn["genomes"][k] for k in ks]
        assert any(k <= N for k in ks) or s[0] == 257
        for i, m in enumerate(eng.fit(genomes, T, V, H2, branch="snp")):
            name = ("snp-%d-%d-%s" if ks[i] > N else "auto-%d-%d-%s") % (s + (ks[i],))
            _check_model(w, name, m, R.case_ref(name), genomes[i], T)
    w.show()


def _snp_keys(s):
    return [k for k in R.KS if k <= 200] + ["dup", "neg"]


def test_a_forms_agree(gpu):
    """TBLUP_FORM=1 (kernel form: W_T^T alpha / d) against TBLUP_FORM=2 (SNP form: the solved beta)
    on the snp-branch genomes, one at a time and as a batch."""
    pn = R.panel()
    w = _Worst("A forms")
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            for s in R.SPLITS:
                T, V = pn["splits"][s]
                keys = _snp_keys(s)
                got[form, s] = (e.fit([pn["genomes"][k] for k in keys], T, V, H2),
                                [e.fit([pn["genomes"][k]], T, V, H2)[0] for k in keys])
    for s in R.SPLITS:
        T = pn["splits"][s][0]
        for i, k in enumerate(_snp_keys(s)):
            name = "auto-%d-%d-%s" % (s + (k,))
            for j in (0, 1):
                m1, m2 = got["1", s][j][i], got["2", s][j][i]
                _check_model(w, name + " form 1", m1, R.case_ref(name), pn["genomes"][k], T)
                _check_model(w, name + " form 2", m2, R.case_ref(name), pn["genomes"][k], T)
                assert w.add("form 1 vs 2", _relmax(m1.effects, m2.effects)) <= EFF_RTOL, name
                np.testing.assert_array_equal(m1.center, m2.center)
                np.testing.assert_array_equal(m1.intercept, m2.intercept)
    w.show()


def test_a_trailing_padding(gpu):
    """TBLUP_PAD_FIRST=0: the SNP form's padding rows trail, the effects are still rows [0, k)."""
    pn = R.panel()
    w = _Worst("A PAD_FIRST=0")
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_PAD_FIRST": "0", "TBLUP_FORM": "2"}) as e:
        for s in R.SPLITS:
            T, V = pn["splits"][s]
            keys = _snp_keys(s)
            genomes = [pn["genomes"][k] for k in keys]
            alone = [e.fit([g], T, V, H2)[0] for g in genomes]
            for i, (mb, ma) in enumerate(zip(e.fit(genomes, T, V, H2), alone)):
                name = "auto-%d-%d-%s" % (s + (keys[i],))
                _check_model(w, name, mb, R.case_ref(name), genomes[i], T)
                _check_model(w, name, ma, R.case_ref(name), genomes[i], T)
    w.show()


# ---------------------------------------------------------------------------------------------
# B. consistency with the evaluator
# ---------------------------------------------------------------------------------------------
def test_b_consistent_with_evaluate(eng):
    pn = R.panel()
    keys = R.KS + ["dup", "neg"]
    genomes = [pn["genomes"][k] for k in keys]
    g64 = pn["geno"].astype(np.float64)
    w = _Worst("B")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        for sel in (slice(None), slice(0, 5)):          # the kernel-form batch and an SNP-form batch
            fit, ebv = eng.evaluate(genomes[sel], T, V, H2, return_ebv=True)
            models = eng.fit(genomes[sel], T, V, H2)
            np.testing.assert_array_equal([m.fitness for m in models], fit)
            pred = eng.predict(models, V)
            assert pred.shape == ebv.shape
            for i, g in enumerate(genomes[sel]):
                assert w.add("vs evaluate", _relmax(pred[i], ebv[i])) <= EBV_RTOL, (s, keys[i])
                _, e_ref = O.blup(g, T, V, g64, pn["pheno"], H2, return_ebv=True)
                assert w.add("vs oracle", _relmax(pred[i], e_ref)) <= EBV_RTOL, (s, keys[i])
    w.show()


# ---------------------------------------------------------------------------------------------
# C. prediction for arbitrary animals
# ---------------------------------------------------------------------------------------------
C_NPRED = [1, 2, 63, 64, 65, 257, 331]


def _animal_list(s, n_pred):
    """Train, valid and untouched animals mixed, in descending row order, with repeats."""
    pn = R.panel()
    T, V = pn["splits"][s]
    rest = np.setdiff1d(np.arange(N), np.concatenate([T, V]))
    rng = np.random.default_rng(1000 + n_pred)
    if n_pred == 1:
        return rest[-1:].copy()
    pool = np.concatenate([rng.choice(T, max(1, n_pred // 3)), rng.choice(V, max(1, n_pred // 4)),
                           rng.choice(rest, n_pred)])[:n_pred]
    pool[-1] = pool[0]                                   # at least one repeat
    out = np.sort(pool)[::-1].copy()
    assert len(out) == n_pred and len(np.unique(out)) < n_pred
    return out


def test_c_arbitrary_animals(eng):
    pn = R.panel()
    g64 = pn["geno"].astype(np.float64)
    keys = [2, 65, 200, 400, "dup"]
    w = _Worst("C")
    for s in ((129, 64), (257, 70)):
        T, V = pn["splits"][s]
        genomes = [pn["genomes"][k] for k in keys]
        models = eng.fit(genomes, T, V, H2)
        models[1] = eng.fit([genomes[1]], T, V, H2)[0]   # k = 65 alone: an SNP-form model
        seen = {}
        for n_pred in C_NPRED:
            an = _animal_list(s, n_pred)
            if n_pred >= 65:
                assert set(an) & set(T) and set(an) & set(V) and set(an) - set(T) - set(V)
            pred = eng.predict(models, an)
            assert pred.shape == (len(models), n_pred)
            np.testing.assert_array_equal(pred, eng.predict(models, an))        # the same bits twice
            for i, g in enumerate(genomes):
                vv = an if n_pred > 1 else np.concatenate([an, an])             # (pearson needs two)
                _, e_ref = O.blup(g, T, vv, g64, pn["pheno"], H2, return_ebv=True)
                assert w.add("vs oracle", _relmax(pred[i], e_ref[:n_pred])) <= EBV_RTOL, (s, keys[i], n_pred)
                host = models[i].predict(pn["geno"][an])
                assert w.add("vs numpy", _relmax(pred[i], host)) <= EBV_RTOL, (s, keys[i], n_pred)
                for a, x in zip(an, pred[i]):                                    # position independence
                    assert seen.setdefault((i, int(a)), x) == x, (s, keys[i], n_pred, a)
        # and against one call on the whole herd in row order
        herd = eng.predict(models, np.arange(N))
        for (i, a), x in seen.items():
            assert herd[i, a] == x
    w.show()


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits(gpu):
    """One factor serves every trait: trait t of an nt-trait fit is the single-trait fit of
    phenotype column t, bit for bit (effects, intercept, centre), and so are its predictions."""
    pn = R.panel()
    T, V = pn["splits"][129, 64]
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    an = _animal_list((129, 64), 65)
    single = {}
    for t in range(4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, t])) as e:
            single[t] = [(ms, e.predict(ms, an)) for ms in (e.fit(b, T, V, H2) for b in batches)]
    for nt in (1, 2, 3, 4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
            for bi, b in enumerate(batches):
                ms = e.fit(b, T, V, H2)
                pred = e.predict(ms, an)
                assert pred.shape == ((len(b), len(an)) if nt == 1 else (len(b), nt, len(an)))
                fit = e.evaluate(b, T, V, H2)
                np.testing.assert_array_equal([m.fitness for m in ms], fit)
                for i, m in enumerate(ms):
                    assert m.effects.shape == (nt, len(b[i])) and m.intercept.shape == (nt,)
                    for t in range(nt):
                        one = single[t][bi][0][i]
                        np.testing.assert_array_equal(m.effects[t], one.effects[0], err_msg=str((nt, bi, i, t)))
                        np.testing.assert_array_equal(m.center, one.center)
                        assert m.intercept[t] == one.intercept[0]
                        got = pred[i] if nt == 1 else pred[i, t]
                        np.testing.assert_array_equal(got, single[t][bi][1][i], err_msg=str((nt, bi, i, t)))


# ---------------------------------------------------------------------------------------------
# E. chunking and solve kernels
# ---------------------------------------------------------------------------------------------
def _same_models(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("indices", "center", "effects", "intercept"):
            np.testing.assert_array_equal(getattr(x, f), getattr(y, f), err_msg=f)
        np.testing.assert_array_equal(x.fitness, y.fitness)


def test_e_chunked_workspace_is_identical(gpu, monkeypatch):
    """A tiny workspace budget forces many chunks in fit and in predict; the same bits."""
    from tblup_amd.engine import GpuBlupEngine
    pn = R.panel()
    T, V = pn["splits"][257, 70]
    genomes = [pn["genomes"][k] for k in R.KS + ["dup", "neg"]] * 3
    an = np.arange(N)[::-1].copy()
    with GpuBlupEngine(pn["geno"], pn["pheno"]) as e:
        ref = e.fit(genomes, T, V, H2)
        ref_snp = e.fit(genomes[:8], T, V, H2)
        ref_pred = e.predict(ref, an)
    monkeypatch.setenv("TBLUP_WORKSPACE_MB", "1")
    with GpuBlupEngine(pn["geno"], pn["pheno"]) as e:
        got = e.fit(genomes, T, V, H2)
        got_snp = e.fit(genomes[:8], T, V, H2)
        got_pred = e.predict(got, an)
    _same_models(got, ref)
    _same_models(got_snp, ref_snp)
    np.testing.assert_array_equal(got_pred, ref_pred)


def test_e_solve_kernels_are_identical(gpu):
    """The effects come from L, the diagonal inverses and z, which neither solve kernel writes:
    TBLUP_SOLVE_CHAIN=0/1 and TBLUP_SOLVE_PULL=0/1 give the same models and fitnesses."""
    pn = R.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, 2, 63, 64, 65, 127, 128, 129, 200, "dup", "neg")]   # SNP form
    mixed = snp + [pn["genomes"][400]]                                                       # kernel form
    got = {}
    for env in ({"TBLUP_SOLVE_CHAIN": "0"}, {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "1"},
                {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "0"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            got[tuple(env.values())] = (e.fit(snp, T, V, H2), e.fit(mixed, T, V, H2))
    base = got["0",]
    for key, val in got.items():
        _same_models(val[0], base[0])
        _same_models(val[1], base[1])


# ---------------------------------------------------------------------------------------------
# F. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_f_monomorphic_panel_gives_nan(gpu):
    pn = R.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            ms = e.fit(genomes, T, V, H2, branch=br)
            fit = e.evaluate(genomes, T, V, H2, branch=br)
            for m, f in zip(ms[:2], fit[:2]):
                assert np.isnan(m.fitness) and np.isnan(f)
                assert np.all(np.isnan(m.effects))
                assert np.all(np.isnan(e.predict([m], V)))
            assert not np.isnan(ms[2].fitness) and not np.any(np.isnan(ms[2].effects))
            np.testing.assert_array_equal(ms[0].center, [0.0])
            np.testing.assert_array_equal(ms[1].center, [0.0, 2.0, 0.0])


def test_f_index_errors(eng):
    from tblup_amd._native import TblupIndexError
    from tblup_amd.model import PanelModel
    pn = R.panel()
    T, V = pn["splits"][129, 64]
    for bad in (P, -P - 1):
        with pytest.raises(TblupIndexError):
            eng.fit([pn["genomes"][64], np.array([3, bad, 5])], T, V, H2)
    ok = eng.fit([np.array([3, -P, P - 1])], T, V, H2)[0]          # the bounds themselves are valid
    np.testing.assert_array_equal(ok.indices, [3, 0, P - 1])
    with pytest.raises(TblupIndexError):
        eng.predict([PanelModel([3, P], [1.0, 1.0], [[0.1, 0.2]], [0.0])], V)
    from tblup_amd._native import TblupError
    with pytest.raises(TblupError):
        eng.predict([ok], [0, N])                                   # an animal outside the panel


def test_f_predict_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        d = np.zeros(1)
        out = np.zeros(1)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_predict_batch(ctx, one.ctypes.data_as(i64), 1, one.ctypes.data_as(i64), off.ctypes.data_as(i64),
                                     1, d.ctypes.data_as(f64), d.ctypes.data_as(f64), d.ctypes.data_as(f64), 1,
                                     out.ctypes.data_as(f64))
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# G. evaluator level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("removed", [(), (5, 17, 301, 599)])
def test_g_fit_models_matches_evaluate_testing(gpu, tmp_path, removed):
    from tblup_amd import evaluator as E
    from tblup_amd.model import PanelModel
    from tests.helpers import IdxIndividual
    pn = R.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, H2, False)
    rem.removed = np.array(removed, dtype=np.float64)
    with E.BlupParallelEvaluator(gp, pp, H2, snp_remover=rem) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        testing = ev.evaluate_testing(pop)
        models = ev.fit_models(pop)
        np.testing.assert_array_equal([m.fitness for m in models], testing)
        for m, indv in zip(models, pop):
            np.testing.assert_array_equal(m.indices, rem.combine_with_removed(indv.genome))
        # the testing animals' EBVs through predict are what evaluate_testing correlated
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        pred = ev.predict(models, ev.testing_indices)
        for i, m in enumerate(models):
            f, e_ref = O.blup(m.indices, train, ev.testing_indices, pn["geno"].astype(np.float64), pn["pheno"], H2,
                              return_ebv=True)
            assert _relmax(pred[i], e_ref) <= EBV_RTOL and abs(m.fitness - f) <= 1e-9
        # the evaluator's own split instead, and an explicit one
        own = ev.fit_models(pop, final=False)
        fit = ev.engine.evaluate([i.genome for i in pop], ev.training_indices, ev.validation_indices, H2)
        np.testing.assert_array_equal([m.fitness for m in own], fit)
        T, V = pn["splits"][129, 64]
        explicit = ev.fit_models(pop, train=T, valid=V)
        np.testing.assert_array_equal([m.fitness for m in explicit],
                                      ev.engine.evaluate([m.indices for m in models], T, V, H2))
        # save / load: the same predictions, on the GPU and on the host
        herd = np.arange(N)
        loaded = []
        for i, m in enumerate(models):
            m.save(str(tmp_path / ("m%d.npz" % i)))
            loaded.append(PanelModel.load(str(tmp_path / ("m%d.npz" % i))))
        np.testing.assert_array_equal(ev.predict(loaded, herd), ev.predict(models, herd))
        for m, l in zip(models, loaded):
            np.testing.assert_array_equal(l.predict(pn["geno"]), m.predict(pn["geno"]))


# ---------------------------------------------------------------------------------------------
# H. the host entries share one workspace
# ---------------------------------------------------------------------------------------------
def _model_arrays(m):
    extra = [m.cov_effects, m.cov_center] if m.cov_effects is not None else []
    return [m.center, m.effects, m.intercept, np.asarray(m.fitness)] + extra


def _entry_calls():
    """(name, call(engine) -> list of arrays) of the host entries on the (257, 70) split, three SNP-form
    genomes (k in 257..331: three tile columns), in an order that alternates small and large workspace
    layouts."""
    from tests.covar_ref import make_cov
    pn = R.panel()
    T, V = pn["splits"][257, 70]
    rng = np.random.default_rng(331)
    genomes = [rng.choice(P, k, replace=False) for k in (257, 300, 331)]
    animals, snps = rng.integers(0, N, 17), rng.integers(0, P, 17)
    q = make_cov(N, 2)

    model = _model_arrays

    def evaluate(e):
        return list(e.evaluate(genomes, T, V, H2, return_ebv=True))

    def fit_cov(e):
        models, ebv = e.fit(genomes, T, V, H2, covariates=q, return_ebv=True)
        return [ebv] + [a for m in models for a in model(m)]

    def loglik(e):
        return list(e.log_likelihood(genomes, T, V, [0.2, 0.45, 0.7], return_sigma2=True))

    def reliability_fit(e):
        models, rel = e.fit(genomes, T, V, H2, reliability_of=animals)
        return [rel] + [a for m in models for a in model(m)]

    def score(e):
        sc = e.snp_scores(genomes, T, V, H2, snps)
        return [sc.score, sc.info, sc.q]

    return [("eval", evaluate), ("fit_cov", fit_cov), ("eval", evaluate), ("loglik", loglik),
            ("reliability+fit", reliability_fit), ("score", score), ("eval", evaluate)]


def test_h_entries_back_to_back_leave_nothing_behind(gpu):
    """One context, the host entries back to back (eval, fit with covariates, eval, log-likelihood,
    reliabilities with the model, SNP scores, eval): every result is bit-equal to the same call on a fresh
    context, so nothing that an entry leaves in the shared workspace reaches an entry of another layout."""
    pn = R.panel()
    calls = _entry_calls()
    with _engine(pn["geno"], pn["pheno"]) as e:
        shared = [call(e) for _, call in calls]
    fresh = {}
    for name, call in calls:
        if name not in fresh:
            with _engine(pn["geno"], pn["pheno"]) as e:
                fresh[name] = call(e)
    for (name, _), got in zip(calls, shared):
        assert len(got) == len(fresh[name]), name
        for i, (a, b) in enumerate(zip(got, fresh[name])):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype, (name, i)
            assert np.all(np.isfinite(a)), (name, i)
            assert a.tobytes() == b.tobytes(), (name, i)


def _single_call_paths():
    """(name, env, n_traits, call(engine) -> list of arrays): one call per workspace layout, on the 331 x 600
    panel.  Together they carve every conditional buffer of the pipeline at least once: the int16 counts and
    the partial sums (SNP form, three tile columns), the last-term tiles, the chained solve's buffers, the K
    block (debug_grm stage 1), the folds' shared counts and row maps (TBLUP_DUAL_ST=0)."""
    from tests.covar_ref import make_cov
    pn = R.panel()
    T, V = pn["splits"][257, 70]
    rng = np.random.default_rng(331)
    snp = [rng.choice(P, k, replace=False) for k in (257, 300, 331)]      # SNP form, three tile columns
    kern = [pn["genomes"][400], snp[1]]                                   # k = 400 / 300: kernel form
    animals, snps = rng.integers(0, N, 17), rng.integers(0, P, 17)
    q, keys = make_cov(N, 2), rng.random((3, P))
    parts = np.array_split(np.random.default_rng(17).permutation(330), 3)
    folds = [(np.concatenate([parts[g] for g in range(3) if g != f]), parts[f]) for f in range(3)]
    fold_snp = [pn["genomes"][k] for k in (63, 129, 200, "neg")]
    fold_kern = [pn["genomes"][400], snp[1], pn["genomes"][332]]

    def models(ms):
        return [a for m in ms for a in _model_arrays(m)]

    def scores(e):
        sc = e.snp_scores(snp, T, V, H2, snps)
        return [sc.score, sc.info, sc.q]

    def grm_block(e):
        K, _ = e.debug_grm(snp[1], T, V, H2, stage=1)     # (stage 1 stops before z is formed)
        return [np.tril(K[:len(T)]), K[len(T):]]          # k_grm computes the lower-triangle tiles of K_TT only

    def keys_async(e):
        import torch
        ev, host, status = e.eval_keys_async(torch.from_numpy(keys).to("cuda:0"), [257, 300, 331], T, V, H2)
        ev.synchronize()
        e.raise_status(status)
        return [host.numpy().copy()]

    paths = []
    for nt in (1, 2):
        paths.append(("evaluate nt=%d" % nt, {}, nt, lambda e: [e.evaluate(snp, T, V, H2)]))
        paths.append(("evaluate+ebv nt=%d" % nt, {}, nt, lambda e: list(e.evaluate(snp, T, V, H2, return_ebv=True))))
    paths += [
        ("evaluate kernel form", {}, 1, lambda e: list(e.evaluate(kern, T, V, H2, return_ebv=True))),
        ("fit", {}, 1, lambda e: models(e.fit(snp, T, V, H2))),
        ("reliability", {}, 1, lambda e: [e.reliability(snp, T, V, H2, animals)]),
        ("snp_scores", {}, 1, scores),
        ("log_likelihood", {}, 1, lambda e: list(e.log_likelihood(snp, T, V, [0.2, 0.45, 0.7], return_sigma2=True))),
        ("fit covariates", {}, 1, lambda e: models(e.fit(snp, T, V, H2, covariates=q))),
        ("folds fused", {}, 1, lambda e: [e.evaluate_folds(fold_snp, folds, H2)]),
        ("folds fused kernel form", {}, 1, lambda e: [e.evaluate_folds(fold_kern, folds, H2)]),
        ("folds DUAL_ST=0", {"TBLUP_DUAL_ST": "0"}, 1, lambda e: [e.evaluate_folds(fold_kern, folds, H2)]),
        ("debug_grm 1", {}, 1, grm_block),
        ("debug_grm 2", {}, 1, lambda e: list(e.debug_grm(snp[1], T, V, H2, stage=2))),
        ("eval_keys_async", {}, 1, keys_async),
    ]
    return paths, (snp, T, V, animals)


def test_i_fresh_context_fits_every_layout(gpu):
    """A context's workspace only grows, so in one context a large early call hides a later call whose measured
    size misses a buffer.  Every workspace size is the measured carve with nothing added: each path makes its
    one call on a fresh context, which allocates exactly that size, so a missed buffer fails the call
    (TBLUP_ERR_STATE from ws_check).  It must succeed and equal, bit for bit, the same call on a context that
    first made a larger one (8 genomes of k = 331 with EBVs)."""
    pn = R.panel()
    paths, (snp, T, V, animals) = _single_call_paths()
    big = [snp[2]] * 8

    def pheno(nt):
        return pn["pheno"] if nt == 1 else np.ascontiguousarray(pn["Y"][:, :nt])

    with _engine(pn["geno"], pn["pheno"]) as e:          # predict needs models: from a context of their own
        fitted = e.fit(snp + [pn["genomes"][400]], T, V, H2)
    paths.append(("predict", {}, 1, lambda e: [e.predict(fitted, animals)]))
    want = {}
    for env, nt in sorted({(tuple(p[1].items()), p[2]) for p in paths}):
        with _engine(pn["geno"], pheno(nt), dict(env)) as e:
            e.evaluate(big, T, V, H2, return_ebv=True)
            for name, penv, pnt, call in paths:
                if (tuple(penv.items()), pnt) == (env, nt):
                    want[name] = call(e)
    for name, env, nt, call in paths:
        with _engine(pn["geno"], pheno(nt), env) as e:
            got = call(e)
        assert len(got) == len(want[name]), name
        for i, (a, b) in enumerate(zip(got, want[name])):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype, (name, i)
            assert a.tobytes() == b.tobytes(), (name, i)
