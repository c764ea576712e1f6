"""Profile (restricted) log-likelihood of h2 from the fitted factor (tblup_loglik_batch, k_loglik) and
estimate_h2 on the GPU, against the dense float64 restatement of tests/loglik_ref.py (itself within
1e-11 max(1, |ref|) of a longdouble computation: tests/test_loglik_host.py).

Panel: 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64), (257, 70) -- one tile
with one padding row, an exact tile, two tiles with 127 padding rows, three tiles -- the genomes of
tests/model_ref.py plus one of k = 300 and the k > n ones; a deeper panel (700 x 800, n_T = 520,
k = 513: five tile columns in either form).  h2 in {0.05, 0.3, 0.6, 0.9}.

  A  loglik and sigma2_g against loglik_ref: auto branch (ragged batch: kernel form; one genome at a
     time: SNP form), forced gblup, forced snp at n_T < k <= n and k > n, the deeper panel in both
     forms, genomes with duplicated and negative indices
  B  TBLUP_FORM=1 against TBLUP_FORM=2; TBLUP_PAD_FIRST=0
  C  the same bits: twice, TBLUP_WORKSPACE_MB=1, TBLUP_SOLVE_CHAIN / TBLUP_SOLVE_PULL, a model alone and
     inside a batch, a (G, B) matrix with constant rows against the (G,) grid, distinct per-model values
     against per-model scalar calls, fitness[g] against evaluate(h2_g)
  D  1 to 4 traits: each trait's values are the single-trait call's on that column, bit for bit
  E  a monomorphic panel (NaN, no error), h2 = 1 / h2 <= 0 / NaN h2, an out-of-range index, a context
     without a panel, an empty grid and an empty batch
  F  estimate_h2 on the engine and on BlupParallelEvaluator against the procedure on the restatement

Tolerance: |got - ref| <= 1e-9 max(1, |ref|), the project's parity bar taken relative because the
log-likelihood is of order N.  Each group prints the largest error it saw (pytest -s); the printed
figures are no thresholds.
"""
import ctypes

import numpy as np
import pytest

from tests import loglik_ref as LL
from tests import model_ref as R
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

TOL = LL.TOL
H2S = np.array(LL.H2S)
N, P = R.N_ANIMALS, R.N_SNPS
K300 = LL.K300


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def check(self, got, ref, name):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, name
        assert np.all(np.isfinite(got)), name
        err = LL.close(got, ref)
        self.v = max(self.v, err)
        assert err <= TOL, (name, err)

    def show(self):
        print("\nLOGLIK %s: worst |got - ref| / max(1, |ref|) %.3e" % (self.label, self.v))


def _refs(name):
    """(loglik, sigma2_g) of a case at every h2 of H2S: two (4,) arrays."""
    r = [LL.case_ref(name, float(h)) for h in H2S]
    return np.array([x[0] for x in r]), np.array([x[1] for x in r])


def _check_case(w, ll, s2, name, tag=""):
    rl, rs = _refs(name)
    w.check(ll, rl, name + tag + " loglik")
    w.check(s2, rs, name + tag + " sigma2_g")


@pytest.fixture(scope="module")
def eng(gpu):
    pn = LL.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    """The ragged batch holds k > n_T and k > n genomes (kernel form; k = 332, 400: gblup); a genome of
    k <= n_T alone takes the SNP form.  dup / neg: duplicated and negative indices."""
    pn = LL.panel()
    genomes = [pn["genomes"][k] for k in LL.A_KEYS]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ll, s2 = eng.log_likelihood(genomes, T, V, H2S, return_sigma2=True)
        assert ll.shape == s2.shape == (len(H2S), len(genomes))
        for i, k in enumerate(LL.A_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            _check_case(w, ll[:, i], s2[:, i], name, " (batch)")
            l1, s1 = eng.log_likelihood([genomes[i]], T, V, H2S, return_sigma2=True)
            _check_case(w, l1[:, 0], s1[:, 0], name, " (alone)")
    w.show()


def test_a_forced_gblup(eng):
    pn = LL.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        genomes = [pn["genomes"][k] for k in R.GBLUP_KS]
        ll, s2 = eng.log_likelihood(genomes, T, V, H2S, branch="gblup", return_sigma2=True)
        for i, k in enumerate(R.GBLUP_KS):
            _check_case(w, ll[:, i], s2[:, i], "gblup-%d-%d-%s" % (s + (k,)))
    w.show()


def test_a_forced_snp_dual(eng):
    """Forced snp at n_T < k <= n and k > n (the kernel form under the train rows' centre: the
    restricted likelihood with q = |z|^2)."""
    pn = LL.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in LL.A_KEYS if not isinstance(k, str) and k > s[0]]
        assert any(k > N for k in ks) and any(k <= N for k in ks)
        ll, s2 = eng.log_likelihood([pn["genomes"][k] for k in ks], T, V, H2S, branch="snp", return_sigma2=True)
        for i, k in enumerate(ks):
            _check_case(w, ll[:, i], s2[:, i], "snp-%d-%d-%s" % (s + (k,)))
    w.show()


def test_a_deeper_panel(gpu):
    """n_T = 520, k = 513: five tile columns, in the SNP form (auto) and in the kernel form."""
    dp = LL.deep_panel()
    w = _Worst("A deep")
    rl = np.array([LL.deep_ref(float(h))[0] for h in H2S])
    rs = np.array([LL.deep_ref(float(h))[1] for h in H2S])
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            ll, s2 = e.log_likelihood([dp["genome"]], dp["train"], dp["valid"], H2S, return_sigma2=True)
            got[form] = ll[:, 0]
            w.check(ll[:, 0], rl, "form %s loglik" % form)
            w.check(s2[:, 0], rs, "form %s sigma2_g" % form)
    assert LL.close(got["1"], got["2"]) <= TOL
    w.show()


# ---------------------------------------------------------------------------------------------
# B. forms and padding
# ---------------------------------------------------------------------------------------------
def _snp_keys():
    return [k for k in R.KS if k <= 200] + ["dup", "neg"]


def test_b_forms_agree(gpu):
    pn = LL.panel()
    w = _Worst("B forms")
    keys = _snp_keys()
    genomes = [pn["genomes"][k] for k in keys]
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            for s in R.SPLITS:
                T, V = pn["splits"][s]
                got[form, s] = e.log_likelihood(genomes, T, V, H2S, return_sigma2=True)
    for s in R.SPLITS:
        for i, k in enumerate(keys):
            name = "auto-%d-%d-%s" % (s + (k,))
            for form in ("1", "2"):
                _check_case(w, got[form, s][0][:, i], got[form, s][1][:, i], name, " form " + form)
            w.check(got["1", s][0][:, i], got["2", s][0][:, i], name + " form 1 vs 2")
            w.check(got["1", s][1][:, i], got["2", s][1][:, i], name + " form 1 vs 2 sigma2_g")
    w.show()


def test_b_trailing_padding(gpu):
    pn = LL.panel()
    w = _Worst("B PAD_FIRST=0")
    keys = _snp_keys() + [K300]
    genomes = [pn["genomes"][k] for k in keys]
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_PAD_FIRST": "0", "TBLUP_FORM": "2"}) as e:
        for s in R.SPLITS:
            T, V = pn["splits"][s]
            ll, s2 = e.log_likelihood(genomes, T, V, H2S, return_sigma2=True)
            for i, k in enumerate(keys):
                _check_case(w, ll[:, i], s2[:, i], "auto-%d-%d-%s" % (s + (k,)))
    w.show()


# ---------------------------------------------------------------------------------------------
# C. the same bits
# ---------------------------------------------------------------------------------------------
def _snp_batch(pn):
    return [pn["genomes"][k] for k in (1, 2, 63, 64, 65, 127, 128, 129, 200, "dup", "neg")]     # SNP form on (257, 70)


def test_c_twice_alone_and_in_a_batch(eng):
    pn = LL.panel()
    T, V = pn["splits"][257, 70]
    snp = _snp_batch(pn)
    mixed = snp + [pn["genomes"][400]]                                                         # kernel form
    for genomes in (snp, mixed):
        a = eng.log_likelihood(genomes, T, V, H2S, return_sigma2=True)
        b = eng.log_likelihood(genomes, T, V, H2S, return_sigma2=True)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        # a model's bits depend neither on the batch around it nor on its position -- within a form
        rev = eng.log_likelihood(genomes[::-1], T, V, H2S, return_sigma2=True)
        np.testing.assert_array_equal(rev[0][:, ::-1], a[0])
        np.testing.assert_array_equal(rev[1][:, ::-1], a[1])
    # alone against inside an SNP-form batch: alone the system has fewer leading padding tiles, whose
    # rows are exact zeros in every contraction
    a = eng.log_likelihood(snp, T, V, H2S, return_sigma2=True)
    for i in range(len(snp)):
        one = eng.log_likelihood([snp[i]], T, V, H2S, return_sigma2=True)
        assert one[0].shape == (len(H2S), 1)
        np.testing.assert_array_equal(one[0][:, 0], a[0][:, i], err_msg=str(i))
        np.testing.assert_array_equal(one[1][:, 0], a[1][:, i], err_msg=str(i))
    # kernel form: the system size is n_T whatever the batch
    k_alone = eng.log_likelihood([pn["genomes"][400]], T, V, H2S, return_sigma2=True)
    k_inb = eng.log_likelihood(mixed, T, V, H2S, return_sigma2=True)
    np.testing.assert_array_equal(k_inb[0][:, -1], k_alone[0][:, 0])
    np.testing.assert_array_equal(k_inb[1][:, -1], k_alone[1][:, 0])


def test_c_chunked_workspace_is_identical(eng, monkeypatch):
    from tblup_amd.engine import GpuBlupEngine
    pn = LL.panel()
    T, V = pn["splits"][257, 70]
    genomes = [pn["genomes"][k] for k in LL.A_KEYS] * 2
    snp = _snp_batch(pn) + [pn["genomes"][K300]]
    ref = eng._loglik(genomes, T, V, H2S, "auto", True)
    ref_snp = eng._loglik(snp, T, V, H2S, "auto", True)
    monkeypatch.setenv("TBLUP_WORKSPACE_MB", "1")
    with GpuBlupEngine(pn["geno"], pn["pheno"]) as e:
        for g, r in ((genomes, ref), (snp, ref_snp)):
            got = e._loglik(g, T, V, H2S, "auto", True)
            for x, y in zip(got, r):
                np.testing.assert_array_equal(x, y)


def test_c_solve_kernels_are_identical(gpu):
    pn = LL.panel()
    T, V = pn["splits"][257, 70]
    snp = _snp_batch(pn) + [pn["genomes"][K300]]
    mixed = snp + [pn["genomes"][400]]
    got = []
    for env in ({"TBLUP_SOLVE_CHAIN": "0"}, {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "1"},
                {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "0"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            got.append(e._loglik(snp, T, V, H2S, "auto", True) + e._loglik(mixed, T, V, H2S, "auto", True))
    for val in got[1:]:
        for x, y in zip(val, got[0]):
            np.testing.assert_array_equal(x, y)


def test_c_forced_expiry_recovers(gpu):
    """A context whose first chained solve gives up a wait (TBLUP_CHAIN_DEBUG="1000,20000,1"): the
    likelihoods were launched beside the first passes and the recovery re-runs every pass for the
    fitness -- all outputs bit-equal to a clean context's, chain_recoveries = 1."""
    pn = LL.panel()
    T, V = pn["splits"][257, 70]
    rng = np.random.default_rng(331257)
    genomes = [rng.choice(P, int(k), replace=False) for k in rng.integers(257, 332, 4)]
    with _engine(pn["geno"], pn["pheno"]) as e:
        ref = e._loglik(genomes, T, V, H2S, "auto", True)
        assert e.chain_recoveries() == 0
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_CHAIN_DEBUG": "1000,20000,1"}) as e:
        got = e._loglik(genomes, T, V, H2S, "auto", True)
        rec = e.chain_recoveries()
    for x, y in zip(got, ref):
        assert np.all(np.isfinite(y))
        np.testing.assert_array_equal(x, y)
    assert rec == 1


def test_c_matrix_rows_grid_scalars_and_fitness(eng):
    pn = LL.panel()
    T, V = pn["splits"][129, 64]
    for genomes in ([pn["genomes"][k] for k in (63, 64, 127, "dup")],            # SNP form
                    [pn["genomes"][k] for k in (65, 200, 400, "neg")]):         # kernel form
        B = len(genomes)
        grid = eng._loglik(genomes, T, V, H2S, "auto", True)
        assert grid[0].shape == grid[1].shape == grid[2].shape == (len(H2S), B)
        const = eng._loglik(genomes, T, V, np.repeat(H2S[:, None], B, axis=1), "auto", True)
        for x, y in zip(const, grid):
            np.testing.assert_array_equal(x, y)
        for g, h in enumerate(H2S):
            np.testing.assert_array_equal(grid[2][g], eng.evaluate(genomes, T, V, float(h)))
            sc = eng.log_likelihood(genomes, T, V, float(h), return_sigma2=True)
            assert sc[0].shape == (B,)
            np.testing.assert_array_equal(sc[0], grid[0][g])
            np.testing.assert_array_equal(sc[1], grid[1][g])
        # distinct per-model values: each model's column is its own scalar call's
        rng = np.random.default_rng(12964)
        hm = rng.uniform(0.03, 0.97, (3, B))
        mat = eng._loglik(genomes, T, V, hm, "auto", True)
        for g in range(3):
            for b in range(B):
                one = eng._loglik(genomes, T, V, float(hm[g, b]), "auto", True)
                for x, y in zip(mat, one):
                    np.testing.assert_array_equal(x[g, b], y[b], err_msg=str((g, b)))


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits(gpu):
    pn = LL.panel()
    T, V = pn["splits"][129, 64]
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    single = []
    for t in range(4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, t])) as e:
            single.append([e.log_likelihood(b, T, V, H2S, return_sigma2=True) for b in batches])
    w = _Worst("D traits")
    for nt in (1, 2, 3, 4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
            for j, b in enumerate(batches):
                ll, s2 = e.log_likelihood(b, T, V, H2S, return_sigma2=True)
                if nt == 1:
                    ll, s2 = ll[..., None], s2[..., None]
                assert ll.shape == s2.shape == (len(H2S), len(b), nt)
                for t in range(nt):
                    np.testing.assert_array_equal(ll[:, :, t], single[t][j][0], err_msg=str((nt, t)))
                    np.testing.assert_array_equal(s2[:, :, t], single[t][j][1], err_msg=str((nt, t)))
    # and against the restatement on the four columns at once
    with _engine(pn["geno"], pn["Y"]) as e:
        for b in batches:
            ll, s2 = e.log_likelihood(b, T, V, H2S, return_sigma2=True)
            for g, h in enumerate(H2S):
                for i, genome in enumerate(b):
                    rl, rs = LL.loglik_ref(genome, T, pn["geno"], pn["Y"], float(h))
                    w.check(ll[g, i], rl, "traits loglik")
                    w.check(s2[g, i], rs, "traits sigma2_g")
    w.show()


# ---------------------------------------------------------------------------------------------
# E. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_e_monomorphic_panel_gives_nan(gpu):
    pn = LL.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            ll, s2 = e.log_likelihood(genomes, T, V, H2S, branch=br, return_sigma2=True)
            assert np.all(np.isnan(ll[:, :2])) and np.all(np.isnan(s2[:, :2]))
            for g, h in enumerate(H2S):
                rl, rs = LL.loglik_ref(genomes[2], T, geno, pn["pheno"], float(h), br)
                assert LL.close(ll[g, 2], rl) <= TOL and LL.close(s2[g, 2], rs) <= TOL
        est = e.estimate_h2(genomes, T, V, refine=1)
        assert np.all(np.isnan(est["h2"][:2])) and np.all(np.isnan(est["loglik"][:2]))
        assert not est["at_bound"][:2].any() and np.isfinite(est["h2"][2])


def test_e_errors(eng):
    from tblup_amd._native import ERR_INDEX, ERR_STATE, TblupError, TblupIndexError
    pn = LL.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64], pn["genomes"][200]]
    for bad in (1.0, 0.0, -0.1, 1.5, float("nan")):
        for h2 in (bad, [0.3, bad], [[0.3, 0.4], [bad, 0.5]]):
            with pytest.raises(TblupError) as ei:
                eng.log_likelihood(g, T, V, h2)
            assert not isinstance(ei.value, TblupIndexError) and ei.value.code not in (ERR_STATE, ERR_INDEX)
    eng.evaluate(g, T, V, 1.0)                                  # h2 = 1 stays valid for the evaluation
    for bad in (P, -P - 1):
        with pytest.raises(TblupIndexError):
            eng.log_likelihood(g + [np.array([3, bad, 5])], T, V, H2S)
    ok = eng.log_likelihood([np.array([3, -P, P - 1])], T, V, 0.3)            # the bounds themselves are valid
    assert LL.close(ok[0], LL.loglik_ref(np.array([3, 0, P - 1]), T, pn["geno"], pn["pheno"], 0.3)[0]) <= TOL
    with pytest.raises(ValueError):
        eng.log_likelihood(g, T, V, np.full((2, 3), 0.3))
    empty = eng.log_likelihood(g, T, V, [])
    assert empty.shape == (0, 2)
    none = eng.log_likelihood([], T, V, H2S)
    assert none.shape == (len(H2S), 0)


def test_e_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        h2 = np.array([0.4])
        out = np.zeros(1)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_loglik_batch(ctx, 0, one.ctypes.data_as(i64), off.ctypes.data_as(i64), 1, h2.ctypes.data_as(f64),
                                    1, 0, None, out.ctypes.data_as(f64), None)
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# F. estimate_h2
# ---------------------------------------------------------------------------------------------
def _check_estimate(w, est, b, ref, name, t=None):
    pick = (lambda a: a[b]) if t is None else (lambda a: a[b, t])
    h, step = pick(est["h2"]), max(pick(est["step"]), ref["step"])      # the last round's spacing
    assert 0.0 < pick(est["step"]) < 1.0, name
    assert abs(h - ref["h2"]) <= step * (1 + 1e-9), (name, h, ref["h2"], step)
    tol = TOL * max(1.0, abs(ref["loglik"]))
    assert pick(est["loglik"]) >= ref["loglik"] - tol, (name, pick(est["loglik"]), ref["loglik"])
    w.v = max(w.v, (ref["loglik"] - pick(est["loglik"])) / max(1.0, abs(ref["loglik"])))
    assert bool(pick(est["at_bound"])) == ref["at_bound"], name
    lam = (1.0 - h) / h
    assert abs(pick(est["sigma2_e"]) - lam * pick(est["sigma2_g"])) <= 1e-12 * max(1.0, pick(est["sigma2_e"]))


def test_f_estimate_h2(eng):
    pn = LL.panel()
    w = _Worst("F estimate_h2 (ref max - loglik at the estimate, relative)")
    T, V = pn["splits"][129, 64]
    for keys, br in (((63, 64, "dup"), "auto"), ((65, 200, 400), "auto"), ((64, 200), "gblup")):
        genomes = [pn["genomes"][k] for k in keys]
        est = eng.estimate_h2(genomes, T, V, branch=br)
        assert set(est) == {"h2", "loglik", "sigma2_g", "sigma2_e", "at_bound", "step"}
        assert est["h2"].shape == (len(keys),) and est["at_bound"].dtype == bool
        for b, k in enumerate(keys):
            ref = LL.estimate_ref(pn["genomes"][k], T, pn["geno"], pn["pheno"], br)
            _check_estimate(w, est, b, ref, "%s %s" % (br, k))
            # the returned likelihood is the likelihood at the returned h2
            again = eng.log_likelihood([genomes[b]], T, V, float(est["h2"][b]), branch=br)
            assert LL.close(again[0], est["loglik"][b]) <= TOL
    print("\nestimate_h2 (129, 64):", np.round(est["h2"], 4), "at_bound", est["at_bound"])
    w.show()


def test_f_estimate_h2_at_the_bound_and_traits(gpu):
    """A phenotype that is pure noise against the markers, or one they explain almost fully, is pushed
    to an end of the grid: at_bound agrees with the restatement's; with four traits the refinement runs
    per trait."""
    pn = LL.panel()
    T, V = pn["splits"][128, 2]
    g64 = pn["geno"].astype(np.float64)
    idx = pn["genomes"][127]
    rng = np.random.default_rng(1282)
    beta = rng.standard_normal(len(idx))
    signal = (g64[:, idx] - g64[:, idx].mean(axis=0)) @ beta
    Y = np.stack([pn["pheno"], signal + 0.05 * signal.std() * rng.standard_normal(N), rng.standard_normal(N),
                  signal + signal.std() * rng.standard_normal(N)], axis=1)
    w = _Worst("F traits (ref max - loglik at the estimate, relative)")
    with _engine(pn["geno"], Y) as e:
        genomes = [idx, pn["genomes"][200]]
        est = e.estimate_h2(genomes, T, V, grid=np.linspace(0.05, 0.95, 10), refine=2, points=5)
        assert est["h2"].shape == (2, 4)
        refs = {}
        for b, g in enumerate(genomes):
            for t in range(4):
                refs[b, t] = LL.estimate_ref(g, T, pn["geno"], Y[:, t], "auto", np.linspace(0.05, 0.95, 10), 2, 5)
                _check_estimate(w, est, b, refs[b, t], str((b, t)), t)
    print("\nestimate_h2 traits:\n", np.round(est["h2"], 4), "\n", est["at_bound"])
    assert refs[0, 1]["at_bound"] and refs[0, 1]["h2"] == 0.95      # the case is what it claims to be
    w.show()


def test_f_evaluator(gpu, tmp_path):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = LL.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, 0.4, False)
    rem.removed = np.array((5, 17, 301, 599), dtype=np.float64)
    w = _Worst("F evaluator")
    with E.BlupParallelEvaluator(gp, pp, 0.4, snp_remover=rem) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 129, 200)]
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        ll = ev.log_likelihood(pop, H2S)
        np.testing.assert_array_equal(ll, ev.engine.log_likelihood(genomes, train, ev.testing_indices, H2S))
        for i, g in enumerate(genomes):
            w.check(ll[:, i], [LL.loglik_ref(g, train, pn["geno"], pn["pheno"], float(h))[0] for h in H2S], "final")
        own = ev.log_likelihood(pop, 0.3, final=False, return_sigma2=True)
        ref = ev.engine.log_likelihood([i.genome for i in pop], ev.training_indices, ev.validation_indices, 0.3,
                                       return_sigma2=True)
        np.testing.assert_array_equal(own[0], ref[0])
        np.testing.assert_array_equal(own[1], ref[1])
        est = ev.estimate_h2(pop, refine=2, points=5)
        direct = ev.engine.estimate_h2(genomes, train, ev.testing_indices, refine=2, points=5)
        for k in est:
            np.testing.assert_array_equal(est[k], direct[k])
        for b, g in enumerate(genomes):
            _check_estimate(w, est, b, LL.estimate_ref(g, train, pn["geno"], pn["pheno"], "auto", refine=2, points=5),
                            "evaluator %d" % b)
    w.show()
