"""Mixed-model score statistics of SNPs (tblup_snp_score_batch, k_snpscore) on the GPU, against the
float64 restatement of tests/score_ref.py (itself within 1e-11 of a longdouble computation:
tests/test_score_host.py).

Panel: 331 animals x 600 SNPs, splits (n_T, n_V) = (127, 5), (128, 2), (129, 64), (257, 70), the genomes
of tests/reliability_ref.py; a deeper panel (700 x 800, n_T = 520, k = 513: 5 tile columns in either form).

  A  against score_ref over all 600 columns: auto branch (ragged batch: kernel form; one genome at a time:
     SNP form where k <= n_T), forced gblup, forced snp at n_T < k <= n and k > n, the deeper panel in both
     forms; in-panel scores = d * effects of fit(); q / dof = sigma2_g of log_likelihood()
  B  TBLUP_FORM=1 against 2 and TBLUP_PAD_FIRST=0: other arithmetic for the same numbers (another
     factorisation, another row order), so they agree within the tolerance, as the reliabilities' group B;
     TBLUP_SCORE_LDS=0 (right-hand sides in the workspace), also with TBLUP_WORKSPACE_MB=1: the same bits
  C  candidate lists of length 1, 15, 16, 17, 33, 65 (in and out of the panel, negatives, repeats): the
     same bits twice, every (model, SNP) value the all-SNP call's, a repeated SNP repeated bits
  D  1 to 4 traits: info bit-identical whatever the phenotypes, score[:, t] and q[:, t] within tolerance of
     the single-trait run on column t
  E  TBLUP_WORKSPACE_MB=1, TBLUP_SOLVE_CHAIN / TBLUP_SOLVE_PULL: the same bits; fitness bit-equal to
     evaluate's; a forced chained-solve expiry recovers with the same bits
  F  a monomorphic model panel (NaN, no error), a candidate monomorphic over the train rows (exact zeros,
     NaN chi2), out-of-range candidates and indices, an empty list, a context without a panel
  G  BlupParallelEvaluator.snp_scores

Tolerance: |got - ref| <= 1e-9 max(1, max |ref|) over the model's candidates (per trait for the score), the
project's EBV_RTOL used as tests/loglik_ref.py::TOL is.  Each group prints the largest error it saw
(pytest -s); the printed figures are no thresholds.
"""
import ctypes

import numpy as np
import pytest

from tests import model_ref as R
from tests import score_ref as S
from tests.test_gpu_model import _engine

pytestmark = pytest.mark.gpu

H2 = S.H2
TOL = S.TOL
N, P = R.N_ANIMALS, R.N_SNPS


class _Worst:
    def __init__(self, label):
        self.label, self.v = label, 0.0

    def close(self, got, ref, name):
        got, ref = np.asarray(got), np.asarray(ref)
        assert got.shape == ref.shape, name
        assert np.all(np.isfinite(got)), name
        err = S.close(got, ref)
        self.v = max(self.v, err)
        assert err <= TOL, (name, err)

    def check(self, sc, b, ref, name):
        """model b of a SnpScores against (u (nt, m), v (m,), q (nt,))."""
        u, v, q = ref
        for t in range(u.shape[0]):
            self.close(sc.score[b, t], u[t], name + " u[%d]" % t)
            self.close(sc.q[b, t], q[t], name + " q[%d]" % t)
        self.close(sc.info[b], v, name + " v")

    def show(self):
        print("\nSCORE %s: worst error / max(1, max |ref|) %.3e" % (self.label, self.v))


def _same(a, b, msg=""):
    for f in ("score", "info", "q", "dof", "snps"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f + " " + msg)


@pytest.fixture(scope="module")
def eng(gpu):
    pn = S.panel()
    with _engine(pn["geno"], pn["pheno"]) as e:
        yield e


# ---------------------------------------------------------------------------------------------
# A. against the restatement
# ---------------------------------------------------------------------------------------------
def test_a_auto_branch(eng):
    pn = S.panel()
    genomes = [pn["genomes"][k] for k in S.A_KEYS]
    w = _Worst("A auto")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        batch = eng.snp_scores(genomes, T, V, H2)
        assert batch.score.shape == (len(genomes), 1, P) and batch.info.shape == (len(genomes), P)
        assert batch.q.shape == (len(genomes), 1)
        np.testing.assert_array_equal(batch.snps, np.arange(P))
        for i, k in enumerate(S.A_KEYS):
            name = "auto-%d-%d-%s" % (s + (k,))
            assert batch.dof[i] == S.dof(genomes[i], T, pn["geno"])
            w.check(batch, i, S.case_ref(name), name + " (batch)")
            w.check(eng.snp_scores([genomes[i]], T, V, H2), 0, S.case_ref(name), name + " (alone)")
    w.show()


def test_a_forced_gblup(eng):
    pn = S.panel()
    w = _Worst("A forced gblup")
    for s in R.FORCED_SPLITS:
        T, V = pn["splits"][s]
        got = eng.snp_scores([pn["genomes"][k] for k in R.GBLUP_KS], T, V, H2, branch="gblup")
        assert np.all(got.dof == len(T))
        for i, k in enumerate(R.GBLUP_KS):
            name = "gblup-%d-%d-%s" % (s + (k,))
            w.check(got, i, S.case_ref(name), name)
    w.show()


def test_a_forced_snp_dual(eng):
    """Forced snp at n_T < k <= n and k > n (the kernel form under the train rows' centre)."""
    pn = S.panel()
    w = _Worst("A forced snp")
    for s in R.SPLITS:
        T, V = pn["splits"][s]
        ks = [k for k in S.A_KEYS if not isinstance(k, str) and k > s[0]]
        assert any(k > N for k in ks) and any(k <= N for k in ks)
        got = eng.snp_scores([pn["genomes"][k] for k in ks], T, V, H2, branch="snp")
        assert np.all(got.dof == len(T) - 1)
        for i, k in enumerate(ks):
            name = "snp-%d-%d-%s" % (s + (k,))
            w.check(got, i, S.case_ref(name), name)
    w.show()


def test_a_deeper_panel(gpu):
    """n_T = 520, k = 513: five tile columns, in the SNP form (TBLUP_FORM=2) and in the kernel form."""
    dp = S.deep_panel()
    w = _Worst("A deep")
    got = {}
    for form in ("2", "1"):
        with _engine(dp["geno"], dp["pheno"], {"TBLUP_FORM": form}) as e:
            got[form] = e.snp_scores([dp["genome"]], dp["train"], dp["valid"], H2)
            w.check(got[form], 0, S.deep_ref(), "form " + form)
    for f in ("score", "info", "q"):
        w.close(getattr(got["1"], f)[0], getattr(got["2"], f)[0], "form 1 vs 2 " + f)
    w.show()


def test_a_in_panel_scores_and_q(eng):
    """For the model's own SNPs u_j = d * effects_j of fit() on the same genomes (d from the model's
    centre); q / dof is log_likelihood()'s sigma2_g at the same h2."""
    pn = S.panel()
    w = _Worst("A effects / sigma2_g")
    T, V = pn["splits"][129, 64]
    for genomes in ([pn["genomes"][k] for k in (1, 63, 64, 127, "dup", "neg")],          # SNP form
                    [pn["genomes"][k] for k in S.A_KEYS]):                              # kernel form
        sc = eng.snp_scores(genomes, T, V, H2)
        models = eng.fit(genomes, T, V, H2)
        _, s2 = eng.log_likelihood(genomes, T, V, H2, return_sigma2=True)
        for b, (g, m) in enumerate(zip(genomes, models)):
            ref = S.d_of_center(m.center) * m.effects[0]
            got = sc.score[b, 0, S.wrap(g, P)]
            assert np.all(np.isfinite(got))
            err = float(np.max(np.abs(got - ref)) / max(1.0, np.max(np.abs(sc.score[b, 0]))))
            w.v = max(w.v, err)
            assert err <= TOL, (b, err)
            w.close(sc.q[b, 0] / sc.dof[b], s2[b], "sigma2_g %d" % b)
    w.show()


# ---------------------------------------------------------------------------------------------
# B. forms, padding, where V lives
# ---------------------------------------------------------------------------------------------
def _snp_keys():
    return [k for k in R.KS if k <= 200] + ["dup", "neg"]


def test_b_forms_agree(gpu):
    pn = S.panel()
    w = _Worst("B forms")
    keys = _snp_keys()
    genomes = [pn["genomes"][k] for k in keys]
    got = {}
    for form in ("1", "2"):
        with _engine(pn["geno"], pn["pheno"], {"TBLUP_FORM": form}) as e:
            for s in R.SPLITS:
                T, V = pn["splits"][s]
                got[form, s] = e.snp_scores(genomes, T, V, H2)
    for s in R.SPLITS:
        for i, k in enumerate(keys):
            name = "auto-%d-%d-%s" % (s + (k,))
            w.check(got["1", s], i, S.case_ref(name), name + " form 1")
            w.check(got["2", s], i, S.case_ref(name), name + " form 2")
            for f in ("score", "info", "q"):
                w.close(getattr(got["1", s], f)[i], getattr(got["2", s], f)[i], name + " form 1 vs 2 " + f)
    w.show()


def test_b_trailing_padding(gpu):
    pn = S.panel()
    w = _Worst("B PAD_FIRST=0")
    keys = _snp_keys()
    genomes = [pn["genomes"][k] for k in keys]
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_PAD_FIRST": "0", "TBLUP_FORM": "2"}) as e:
        for s in R.SPLITS:
            T, V = pn["splits"][s]
            got = e.snp_scores(genomes, T, V, H2)
            for i, k in enumerate(keys):
                name = "auto-%d-%d-%s" % (s + (k,))
                w.check(got, i, S.case_ref(name), name)
    w.show()


def test_b_workspace_right_hand_sides_same_bits(eng):
    """TBLUP_SCORE_LDS=0 keeps V in the workspace (the path of systems above 1024 rows): the same bits in
    both forms; with a 1 MB workspace budget the list is walked a few slabs per launch."""
    pn = S.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, 65, 129, 200, "dup", S.K300)]
    mixed = snp + [pn["genomes"][400]]
    lst = S.cand_list(pn["genomes"][65], P, 65)
    ref = {(i, j): eng.snp_scores(g, T, V, H2, c) for i, g in enumerate((snp, mixed)) for j, c in enumerate((None, lst))}
    for env in ({"TBLUP_SCORE_LDS": "0"}, {"TBLUP_SCORE_LDS": "0", "TBLUP_WORKSPACE_MB": "1"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            for i, g in enumerate((snp, mixed)):
                for j, c in enumerate((None, lst)):
                    _same(e.snp_scores(g, T, V, H2, c), ref[i, j], str(env))


# ---------------------------------------------------------------------------------------------
# C. candidate lists
# ---------------------------------------------------------------------------------------------
def test_c_candidate_lists(eng):
    pn = S.panel()
    keys = [2, 65, 200, 400, "dup"]
    for s in ((129, 64), (257, 70)):
        T, V = pn["splits"][s]
        genomes = [pn["genomes"][k] for k in keys]                 # kernel form
        snp_form = [genomes[1], genomes[4]]                        # k = 65 and 100: an SNP-form batch
        full = {0: eng.snp_scores(genomes, T, V, H2), 1: eng.snp_scores(snp_form, T, V, H2)}
        for m in S.LIST_LENGTHS:
            lst = S.cand_list(genomes[1], P, m)
            cols = S.wrap(lst, P)
            for which, batch in ((0, genomes), (1, snp_form)):
                got = eng.snp_scores(batch, T, V, H2, lst)
                assert got.score.shape == (len(batch), 1, m) and got.info.shape == (len(batch), m)
                np.testing.assert_array_equal(got.snps, cols)
                _same(got, eng.snp_scores(batch, T, V, H2, lst), "twice")
                # every (model, SNP) value is the all-SNP call's, wherever it stands and whatever n_cand is
                np.testing.assert_array_equal(got.score, full[which].score[:, :, cols], err_msg=str((s, m)))
                np.testing.assert_array_equal(got.info, full[which].info[:, cols], err_msg=str((s, m)))
                np.testing.assert_array_equal(got.q, full[which].q, err_msg=str((s, m)))
                if m >= 3:      # the list's last entry repeats its first
                    np.testing.assert_array_equal(got.score[:, :, -1], got.score[:, :, 0])
                    np.testing.assert_array_equal(got.info[:, -1], got.info[:, 0])


# ---------------------------------------------------------------------------------------------
# D. traits
# ---------------------------------------------------------------------------------------------
def test_d_traits(gpu):
    pn = S.panel()
    T, V = pn["splits"][129, 64]
    batches = [[pn["genomes"][k] for k in (63, 64, 127)],            # SNP form
               [pn["genomes"][k] for k in (65, 200, 400)]]          # kernel form (k = 400: gblup)
    lst = S.cand_list(pn["genomes"][65], P, 65)
    w = _Worst("D traits")
    single = []
    for t in range(4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, t])) as e:
            single.append([e.snp_scores(b, T, V, H2, lst) for b in batches])
    for nt in (1, 2, 3, 4):
        with _engine(pn["geno"], np.ascontiguousarray(pn["Y"][:, :nt])) as e:
            for i, b in enumerate(batches):
                got = e.snp_scores(b, T, V, H2, lst)
                assert got.score.shape == (len(b), nt, len(lst)) and got.q.shape == (len(b), nt)
                np.testing.assert_array_equal(got.info, single[0][i].info, err_msg=str(nt))
                np.testing.assert_array_equal(got.info, single[3][i].info, err_msg=str(nt))
                for t in range(nt):
                    for m in range(len(b)):
                        w.close(got.score[m, t], single[t][i].score[m, 0], "u nt=%d t=%d" % (nt, t))
                        w.close(got.q[m, t], single[t][i].q[m, 0], "q nt=%d t=%d" % (nt, t))
                if nt == 4:
                    for m, g in enumerate(b):
                        w.check(got, m, S.score_ref(g, T, pn["geno"], pn["Y"], H2, snps=lst,
                                                    form="snp" if i == 0 else "kernel"), "4 traits")
    w.show()


# ---------------------------------------------------------------------------------------------
# E. chunking, solve kernels, and the other outputs of the same pass
# ---------------------------------------------------------------------------------------------
def test_e_chunked_workspace_is_identical(eng):
    pn = S.panel()
    T, V = pn["splits"][257, 70]
    genomes = [pn["genomes"][k] for k in S.A_KEYS] * 2
    lst = np.arange(P)[::-3].copy()
    ref = eng.snp_scores(genomes, T, V, H2, lst)
    ref_snp = eng.snp_scores(genomes[:8], T, V, H2, lst)
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_WORKSPACE_MB": "1"}) as e:
        _same(e.snp_scores(genomes, T, V, H2, lst), ref)
        _same(e.snp_scores(genomes[:8], T, V, H2, lst), ref_snp)


def test_e_solve_kernels_are_identical(gpu):
    pn = S.panel()
    T, V = pn["splits"][257, 70]
    snp = [pn["genomes"][k] for k in (1, 2, 63, 64, 65, 127, 128, 129, 200, "dup", "neg")]   # SNP form
    mixed = snp + [pn["genomes"][400]]                                                       # kernel form
    lst = S.cand_list(pn["genomes"][65], P, 65)
    got = []
    for env in ({"TBLUP_SOLVE_CHAIN": "0"}, {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "1"},
                {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "0"}):
        with _engine(pn["geno"], pn["pheno"], env) as e:
            got.append((e.snp_scores(snp, T, V, H2, lst), e.snp_scores(mixed, T, V, H2, lst)))
    for val in got[1:]:
        _same(val[0], got[0][0])
        _same(val[1], got[0][1])


def test_e_fitness_is_evaluates(eng):
    from tblup_amd.engine import concat_genomes
    pn = S.panel()
    T, V = pn["splits"][129, 64]
    lst = S.cand_list(pn["genomes"][65], P, 33)
    i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    for genomes in ([pn["genomes"][k] for k in (63, 64, 127)], [pn["genomes"][k] for k in S.A_KEYS]):
        sc = eng.snp_scores(genomes, T, V, H2, lst)
        fit = eng.evaluate(genomes, T, V, H2)
        idx, off = concat_genomes(genomes)
        B = len(genomes)
        f2, u2, v2 = np.empty(B), np.empty((B, 1, len(lst))), np.empty((B, len(lst)))
        sid = eng.split_id(T, V)
        rc = eng._lib.tblup_snp_score_batch(eng._ctx, sid, lst.ctypes.data_as(i64), len(lst), idx.ctypes.data_as(i64),
                                            off.ctypes.data_as(i64), B, H2, 0, f2.ctypes.data_as(f64),
                                            u2.ctypes.data_as(f64), v2.ctypes.data_as(f64), None)
        assert rc == 0
        np.testing.assert_array_equal(f2, fit)
        np.testing.assert_array_equal(u2, sc.score)
        np.testing.assert_array_equal(v2, sc.info)


def test_e_forced_expiry_keeps_scores(gpu):
    """snp_scores on a context whose first chained solve gives up a bounded wait
    (TBLUP_CHAIN_DEBUG="1000,20000,1", the reliability tests' set-up): the score launch runs once, beside
    the first pass, and the recovery pass re-solves for the fitness only -- scores bit-equal to a clean
    context's, chain_recoveries = 1.  SNP form with three tile columns (k in 257..331 on split (257, 70))."""
    pn = S.panel()
    T, V = pn["splits"][257, 70]
    rng = np.random.default_rng(331257)
    genomes = [rng.choice(P, int(k), replace=False) for k in rng.integers(257, 332, 4)]
    lst = np.arange(P)[::-3].copy()
    with _engine(pn["geno"], pn["pheno"]) as e:
        ref = e.snp_scores(genomes, T, V, H2, lst)
        assert e.chain_recoveries() == 0
    with _engine(pn["geno"], pn["pheno"], {"TBLUP_CHAIN_DEBUG": "1000,20000,1"}) as e:
        got = e.snp_scores(genomes, T, V, H2, lst)
        rec = e.chain_recoveries()
    print("\nforced expiry in snp_scores: chain_recoveries", rec)
    _same(got, ref)
    assert np.all(np.isfinite(ref.score)) and np.all(np.isfinite(ref.info)) and np.all(np.isfinite(ref.q))
    assert rec == 1


# ---------------------------------------------------------------------------------------------
# F. degenerate inputs and errors
# ---------------------------------------------------------------------------------------------
def test_f_monomorphic_model_panel_gives_nan(gpu):
    pn = S.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    geno[:, 1] = 2
    T, V = pn["splits"][129, 64]
    with _engine(geno, pn["pheno"]) as e:
        genomes = [np.array([0]), np.array([0, 1, 0]), pn["genomes"][64]]
        for br in ("auto", "gblup"):
            sc = e.snp_scores(genomes, T, V, H2, branch=br)
            assert np.all(np.isnan(sc.score[:2])) and np.all(np.isnan(sc.info[:2])) and np.all(np.isnan(sc.q[:2]))
            w = _Worst("F")
            w.check(sc, 2, S.score_ref(genomes[2], T, geno, pn["pheno"], H2, br), br)


def test_f_monomorphic_candidate_gives_exact_zeros(gpu):
    """A column that is constant over the train rows (not over the herd): w_j = 0 under snp, so u = v = 0
    exactly in both forms, and chi2 / effect / loglik_gain are NaN there."""
    pn = S.panel()
    geno = pn["geno"].copy()
    T, V = pn["splits"][129, 64]
    geno[T, 7] = 2
    geno[T, 9] = 0
    assert len(np.unique(geno[:, 7])) > 1
    with _engine(geno, pn["pheno"]) as e:
        for genomes in ([pn["genomes"][64]], [pn["genomes"][64], pn["genomes"][200]]):     # SNP form, kernel form
            sc = e.snp_scores(genomes, T, V, H2, [5, 7, 9, 7 - P])
            for j in (1, 2, 3):
                assert np.all(sc.score[:, :, j] == 0) and np.all(sc.info[:, j] == 0)
            assert np.all(sc.info[:, 0] > 0)
            chi = sc.chi2()
            assert np.all(np.isnan(chi[:, :, 1:])) and np.all(np.isfinite(chi[:, :, 0]))
            assert np.all(np.isnan(sc.effect()[:, :, 1:])) and np.all(np.isnan(sc.loglik_gain()[:, :, 1:]))


def test_f_errors(eng):
    from tblup_amd._native import TblupError, TblupIndexError
    pn = S.panel()
    T, V = pn["splits"][129, 64]
    g = [pn["genomes"][64]]
    for bad in (P, -P - 1):
        with pytest.raises(TblupIndexError):
            eng.snp_scores(g, T, V, H2, [0, bad])
        with pytest.raises(TblupIndexError):
            eng.snp_scores(g + [np.array([3, bad, 5])], T, V, H2)
    ok = eng.snp_scores([np.array([3, -P, P - 1])], T, V, H2, [-P, P - 1, 3])      # the bounds themselves are valid
    ref = S.score_ref(np.array([3, 0, P - 1]), T, pn["geno"], pn["pheno"], H2, snps=[0, P - 1, 3])
    _Worst("F bounds").check(ok, 0, ref, "bounds")
    np.testing.assert_array_equal(ok.snps, [0, P - 1, 3])
    empty = eng.snp_scores(g * 3, T, V, H2, [])
    assert empty.score.shape == (3, 1, 0) and empty.info.shape == (3, 0) and empty.q.shape == (3, 1)
    none = eng.snp_scores([], T, V, H2, [1, 2])
    assert none.score.shape == (0, 1, 2) and none.info.shape == (0, 2)
    with pytest.raises(TblupError):
        eng.snp_scores(g, T, V, 1.0)


def test_f_needs_a_panel(gpu):
    from tblup_amd import _native
    lib = gpu
    ctx = ctypes.c_void_p()
    assert lib.tblup_ctx_create(None, 0, 0, 0, None, 0, ctypes.byref(ctx)) == 0
    try:
        one = np.zeros(1, dtype=np.int64)
        off = np.array([0, 1], dtype=np.int64)
        out, out2 = np.zeros(1), np.zeros(1)
        i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        rc = lib.tblup_snp_score_batch(ctx, 0, one.ctypes.data_as(i64), 1, one.ctypes.data_as(i64),
                                       off.ctypes.data_as(i64), 1, 0.4, 0, None, out.ctypes.data_as(f64),
                                       out2.ctypes.data_as(f64), None)
        assert rc == _native.ERR_STATE
        assert b"panel" in lib.tblup_last_error()
    finally:
        lib.tblup_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# G. evaluator level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("removed", [(), (5, 17, 301, 599)])
def test_g_evaluator_snp_scores(gpu, tmp_path, removed):
    from tblup_amd import evaluator as E
    from tests.helpers import IdxIndividual
    pn = S.panel()
    gp, pp = str(tmp_path / "g.npy"), str(tmp_path / "p.npy")
    np.save(gp, pn["geno"].astype(np.float64))
    np.save(pp, pn["pheno"])
    rng = np.random.default_rng(7)
    rem = E.SNPRemovalHandler(100, 0.0, H2, False)
    rem.removed = np.array(removed, dtype=np.float64)
    w = _Worst("G")
    with E.BlupParallelEvaluator(gp, pp, H2, snp_remover=rem) as ev:
        pop = [IdxIndividual(rng.choice(P, k, replace=False), k) for k in (40, 64, 129, 200)]
        lst = S.cand_list(pop[1].genome, P, 33)
        sc = ev.snp_scores(pop, lst)
        genomes = [rem.combine_with_removed(i.genome) for i in pop]
        train = np.concatenate((ev.training_indices, ev.validation_indices))
        _same(sc, ev.engine.snp_scores(genomes, train, ev.testing_indices, H2, lst))
        for i, g in enumerate(genomes):
            # one batch, one form: the kernel form when any model has k > n_T
            form = "snp" if max(len(x) for x in genomes) <= len(train) else "kernel"
            w.check(sc, i, S.score_ref(g, train, pn["geno"], pn["pheno"], H2, snps=lst, form=form), "model %d" % i)
        every = ev.snp_scores(pop)
        assert every.score.shape == (len(pop), 1, P)
        np.testing.assert_array_equal(every.score[:, :, S.wrap(lst, P)], sc.score)
        own = ev.snp_scores(pop, lst, final=False)
        _same(own, ev.engine.snp_scores([i.genome for i in pop], ev.training_indices, ev.validation_indices, H2, lst))
    w.show()
