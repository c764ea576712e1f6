"""Edge parity: the HIP pipeline against the oracle (or numpy) at the shapes where kernels go wrong,
not the shapes the benchmark runs.

  A  unaligned splits (n_T, n_V of 1, 2, 3, 127, 129, 257 ...), every k around the 64-SNP block and
     the 128-row tile, a panel whose size is no multiple of 4 or 64, ragged batches and single genomes
  B  pearson_abs around its 1024-thread stride; n_V = 2 and 3; constant and two-valued y_V
  C  1, 2, 3 and 4 traits under both solve kernels
  D  both sides of the int16 count store (SNP form, kernel form, shared fold counts)
  E  both sides of k_sys_tiles_st's row table
  F  the SNP-major panel layout
  G  k_decode_topk at small d, k == d, ties, signed zeros, infinities, NaN, its fallbacks, ld > d
  H  tblup_grm and tblup_snp_scan at sizes below one tile / one workgroup / one stage

Tolerances are those of tests/test_gpu_parity.py; tests/test_edge_cases_cpu.py shows the oracle
itself is good to 1e-11 on the evaluator cases of A, B, C and D1.  Each test prints the largest
error it saw (pytest -s) for PERFLOG.md; the printed figures are no thresholds.
"""
import contextlib
import functools
import math
import os

import numpy as np
import pytest

from oracle import blup_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

H2 = H.EDGE_H2
LAM = (1 - H2) / H2
EBV_RTOL = 1e-9
FIT_ATOL = 1e-9
K_RTOL = 1e-12
CHOL_RTOL = 1e-10


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
    """Largest errors seen by one test, printed at its end."""

    def __init__(self, label):
        self.label, self.v = label, {}

    def add(self, key, x):
        self.v[key] = max(self.v.get(key, 0.0), float(x))
        return x

    def show(self):
        print("\nEDGE %s: %s" % (self.label, ", ".join("max %s %.3e" % kv for kv in sorted(self.v.items()))))


def _check_vs_oracle(w, name, f, e, f_ref, e_ref):
    """NaN exactly where the oracle has NaN; elsewhere the project's tolerances."""
    assert np.isnan(f) == np.isnan(f_ref), (name, f, f_ref)
    np.testing.assert_array_equal(np.isnan(e), np.isnan(e_ref), err_msg=name)
    if not np.isnan(f_ref):
        assert w.add("fit", abs(f - f_ref)) <= FIT_ATOL, (name, f, f_ref)
    if not np.any(np.isnan(e_ref)):
        assert w.add("ebv", _relmax(e, e_ref)) <= EBV_RTOL, name


@functools.lru_cache(maxsize=None)
def _oracle(group):
    cases = {"A": H.edge_a_cases, "B": H.edge_b_cases, "C": H.edge_c_cases, "D1": H.edge_d1_cases,
             "D2": H.edge_d2_cases, "E": H.edge_e_cases}[group]()
    return {c["name"]: H.edge_oracle(c) for c in cases}


# ---------------------------------------------------------------------------------------------
# A. unaligned splits and index counts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [None, "1", "2"])
def test_a_unaligned_splits(gpu, form):
    """Every split x every genome, as one ragged batch (its largest k sets the padding) and one
    genome at a time, under the automatic form, the kernel form and the SNP form (snp-branch
    genomes only, as the forced-form tests of test_gpu_parity.py)."""
    a, ref = H.edge_a(), _oracle("A")
    names = [nm for nm in a["genomes"] if form != "2" or H.edge_a_is_snp(a, nm)]
    genomes = [a["genomes"][nm] for nm in names]
    w = _Worst("A form=%s" % form)
    with _engine(a["geno"], a["pheno"], {} if form is None else {"TBLUP_FORM": form}) as eng:
        for s, (T, V) in a["splits"].items():
            fit, ebv = eng.evaluate(genomes, T, V, H2, return_ebv=True)
            for i, nm in enumerate(names):
                name = "A-%d-%d-%s" % (s + (nm,))
                _check_vs_oracle(w, name + " (batch)", fit[i], ebv[i], *ref[name])
                f1, e1 = eng.evaluate([genomes[i]], T, V, H2, return_ebv=True)
                _check_vs_oracle(w, name + " (alone)", f1[0], e1[0], *ref[name])
                # the same system with moved padding: test_leading_padding_matches_trailing's tolerance
                np.testing.assert_allclose(f1[0], fit[i], rtol=0, atol=1e-11, err_msg=name)
                np.testing.assert_allclose(e1[0], ebv[i], rtol=1e-9, atol=1e-9, err_msg=name)
                if not np.isnan(fit[i]):
                    w.add("alone-vs-batch fit", abs(f1[0] - fit[i]))
    w.show()


def test_a_forced_branches(gpu):
    a, ref = H.edge_a(), _oracle("A")
    genomes = [a["genomes"]["k%d" % k] for k in H.EDGE_A_FORCED_KS]
    w = _Worst("A forced branch")
    with _engine(a["geno"], a["pheno"]) as eng:
        for s in H.EDGE_A_FORCED_SPLITS:
            T, V = a["splits"][s]
            for br in ("gblup", "snp"):
                fit, ebv = eng.evaluate(genomes, T, V, H2, branch=br, return_ebv=True)
                for i, k in enumerate(H.EDGE_A_FORCED_KS):
                    name = "A-%d-%d-k%d-%s" % (s + (k, br))
                    _check_vs_oracle(w, name, fit[i], ebv[i], *ref[name])
    w.show()


def _a_kref(a, s, k):
    T, V = a["splits"][s]
    Kref = O.grm_block(a["genomes"]["k%d" % k], T, V, a["geno"])
    Kref[np.arange(len(T)), np.arange(len(T))] += LAM
    return T, V, Kref


def test_a_grm_block(gpu):
    """K_{R,T} (debug_grm stage 1) at two and three tile columns with one row in the last tile.
    k_grm computes the TT lower-triangle tiles (diagonal tiles in full) and the VT block, so the TT
    block is compared on its lower triangle."""
    a = H.edge_a()
    w = _Worst("A debug_grm stage 1")
    with _engine(a["geno"], a["pheno"]) as eng:
        for s in ((129, 127), (257, 6)):
            for k in H.EDGE_A_FORCED_KS:
                T, V, Kref = _a_kref(a, s, k)
                nT = len(T)
                K, _ = eng.debug_grm(a["genomes"]["k%d" % k], T, V, H2, stage=1)
                scale = np.max(np.abs(Kref))
                assert w.add("K", np.max(np.abs(np.tril(K[:nT]) - np.tril(Kref[:nT]))) / scale) <= K_RTOL, (s, k)
                assert w.add("K", np.max(np.abs(K[nT:] - Kref[nT:])) / scale) <= K_RTOL, (s, k)
    w.show()


def test_a_factor_and_forward_solve(gpu):
    """The Cholesky factor and the forward solve (debug_grm stage 2) at the same shapes: the first
    readback of systems with more than one tile column.  It used to return NaN at L[128, 128] and
    wrong rows >= 128: the readback's "also store L_JJ" flag shared bit 16 of the launch mask with
    the k_sys_tiles ablation bit "store no off-diagonal system tile", so the factorisation of a
    multi-tile system ran on tiles that were never written (evaluations were not affected)."""
    a = H.edge_a()
    y = a["pheno"]
    w = _Worst("A debug_grm stage 2")
    bad = []
    with _engine(a["geno"], y) as eng:
        for s in ((129, 127), (257, 6)):
            for k in H.EDGE_A_FORCED_KS:
                T, V, Kref = _a_kref(a, s, k)
                nT = len(T)
                F, z = eng.debug_grm(a["genomes"]["k%d" % k], T, V, H2, stage=2)
                L = np.linalg.cholesky(Kref[:nT])
                mu = 0.0 if k > a["n"] else float(np.mean(y[T]))
                ec = w.add("chol", _relmax(np.tril(F[:nT]), L))
                ez = w.add("fwd", _relmax(z, np.linalg.solve(L, y[T] - mu)))
                print("stage 2 %s k=%d: chol %.3e fwd %.3e" % (s, k, ec, ez))
                if not (ec <= CHOL_RTOL and ez <= CHOL_RTOL):
                    bad.append((s, k, ec, ez))
    w.show()
    assert not bad, "(split, k, factor error, forward-solve error) above 1e-10: %s" % bad


# ---------------------------------------------------------------------------------------------
# B. Pearson edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pheno", ["normal", "const", "two"])
def test_b_pearson_edges(gpu, pheno):
    b, ref = H.edge_b(), _oracle("B")
    ks = sorted(b["genomes"])
    w = _Worst("B pheno=%s" % pheno)
    with _engine(b["geno"], b["pheno"][pheno]) as eng:
        for nv, V in b["V"].items():
            fit, ebv = eng.evaluate([b["genomes"][k] for k in ks], b["T"], V, H2, return_ebv=True)
            for i, k in enumerate(ks):
                name = "B-%s-nv%d-k%d" % (pheno, nv, k)
                _check_vs_oracle(w, name, fit[i], ebv[i], *ref[name])
                if pheno == "const":
                    assert np.isnan(fit[i]), name
                if nv == 2 and pheno != "const":
                    assert fit[i] == 1.0, name      # scipy rounds r when n == 2
    w.show()


# ---------------------------------------------------------------------------------------------
# C. trait counts 1, 2, 3, 4
# ---------------------------------------------------------------------------------------------
C_SETTINGS = [{"TBLUP_SOLVE_CHAIN": "0"},
              {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "0"},
              {"TBLUP_SOLVE_CHAIN": "1", "TBLUP_SOLVE_PULL": "1"}]


@pytest.mark.parametrize("setting", range(len(C_SETTINGS)))
def test_c_trait_counts(gpu, setting):
    """test_multitrait_equals_single_traits at 2, 3 and 4 traits: each trait's EBVs bit-equal to
    the single-trait engine on that column and within 1e-9 of the oracle; fitness = the mean."""
    c, ref = H.edge_c(), _oracle("C")
    env = C_SETTINGS[setting]
    T, V = c["T"], c["V"]
    w = _Worst("C %s" % env)
    single = {}
    for tr in range(4):
        with _engine(c["geno"], np.ascontiguousarray(c["Y"][:, tr]), env) as eng:
            for k, gs in c["genomes"].items():
                fit, ebv = eng.evaluate(gs, T, V, H2, return_ebv=True)
                single[tr, k] = (fit, ebv)
                for i in range(len(gs)):
                    _check_vs_oracle(w, "single", fit[i], ebv[i], *ref["C-k%d-%d-trait%d" % (k, i, tr)])
    for nt in (2, 3, 4):
        with _engine(c["geno"], np.ascontiguousarray(c["Y"][:, :nt]), env) as eng:
            assert eng.n_traits == nt
            for k, gs in c["genomes"].items():
                fit, ebv = eng.evaluate(gs, T, V, H2, return_ebv=True)
                assert ebv.shape == (len(gs), nt, len(V))
                for i in range(len(gs)):
                    for tr in range(nt):
                        np.testing.assert_array_equal(ebv[i, tr], single[tr, k][1][i], err_msg=str((nt, k, i, tr)))
                        e_ref = ref["C-k%d-%d-trait%d" % (k, i, tr)][1]
                        assert w.add("ebv", _relmax(ebv[i, tr], e_ref)) <= EBV_RTOL, (nt, k, i, tr)
                    mean = np.mean([single[tr, k][0][i] for tr in range(nt)])
                    assert w.add("fit-vs-mean", abs(fit[i] - mean)) <= 1e-15, (nt, k, i)
    w.show()


# ---------------------------------------------------------------------------------------------
# D. the int16 count limit, both sides
# ---------------------------------------------------------------------------------------------
def test_d1_snp_form_count_limit(gpu):
    d, ref = H.edge_d1(), _oracle("D1")
    w = _Worst("D1")
    got = {}
    for st in (None, "0", "1"):
        with _engine(d["geno"], d["pheno"], {} if st is None else {"TBLUP_SYS_ST": st}) as eng:
            for nT, (T, V) in d["splits"].items():
                fit, ebv = eng.evaluate(d["genomes"], T, V, H2, return_ebv=True)
                got[st, nT] = (fit, ebv)
                for i in range(len(d["genomes"])):
                    _check_vs_oracle(w, "D1 st=%s nT=%d g%d" % (st, nT, i), fit[i], ebv[i], *ref["D1-nT%d-%d" % (nT, i)])
    for j in (0, 1):
        np.testing.assert_array_equal(got["0", 8191][j], got["1", 8191][j])
    w.show()


def test_d2_kernel_form_count_limit(gpu):
    """k = 8128 takes the int16 system tiles, 8129 and 8192 the in-tile products; one genome per
    call (a batch's largest k sets the contraction length)."""
    d, ref = H.edge_d2(), _oracle("D2")
    w = _Worst("D2")
    got = {}
    for st in ("1", "0"):
        with _engine(d["geno"], d["pheno"], {"TBLUP_FORM": "1", "TBLUP_DUAL_ST": st}) as eng:
            for k, g in d["genomes"].items():
                for br in ("auto", "snp"):
                    fit, ebv = eng.evaluate([g], d["T"], d["V"], H2, branch=br, return_ebv=True)
                    got[st, k, br] = (fit, ebv)
                    _check_vs_oracle(w, "D2 st=%s k=%d %s" % (st, k, br), fit[0], ebv[0], *ref["D2-k%d-%s" % (k, br)])
    for (st, k, br), (fit, ebv) in got.items():
        np.testing.assert_array_equal(fit, got["0", k, br][0])
        np.testing.assert_array_equal(ebv, got["0", k, br][1])
    w.show()


def test_d3_shared_fold_counts(gpu):
    d = H.edge_d3()
    w = _Worst("D3")
    with _engine(d["geno"], d["pheno"]) as eng:
        got = eng.evaluate_folds(d["genomes"], d["folds"], H2)
        assert got.shape == (5, len(d["genomes"]))
        for f, (T, V) in enumerate(d["folds"]):
            assert (len(T), len(V)) == (8188, 2047)
            fit, ebv = eng.evaluate(d["genomes"], T, V, H2, return_ebv=True)
            np.testing.assert_array_equal(got[f], fit)
            if f in (0, 3):
                for i, g in enumerate(d["genomes"]):
                    f_ref, e_ref = O.snp_blup(g, T, V, d["geno"], d["pheno"], H2, return_ebv=True)
                    _check_vs_oracle(w, "D3 fold %d g%d" % (f, i), got[f, i], ebv[i], f_ref, e_ref)
    w.show()


# ---------------------------------------------------------------------------------------------
# E. the SP_ROWTAB limit
# ---------------------------------------------------------------------------------------------
def test_e_sys_tiles_row_table_limit(gpu):
    e, ref = H.edge_e(), _oracle("E")
    w = _Worst("E")
    got = {}
    for st in (None, "0", "1"):
        with _engine(e["geno"], e["pheno"], {} if st is None else {"TBLUP_SYS_ST": st}) as eng:
            for k, gs in e["genomes"].items():
                fit, ebv = eng.evaluate(gs, e["T"], e["V"], H2, return_ebv=True)
                got[st, k] = (fit, ebv)
                for i in range(len(gs)):
                    _check_vs_oracle(w, "E st=%s k=%d g%d" % (st, k, i), fit[i], ebv[i], *ref["E-k%d-%d" % (k, i)])
    for k in e["genomes"]:
        for j in (0, 1):
            np.testing.assert_array_equal(got["0", k][j], got["1", k][j])
    w.show()


# ---------------------------------------------------------------------------------------------
# F. SNP-major layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(263, 530), (64, 64), (65, 63)])
def test_f_snp_major_layout(gpu, shape):
    n, P = shape
    rng = np.random.default_rng((2610, n))
    if shape == (263, 530):
        a = H.edge_a()
        geno, pheno = a["geno"], a["pheno"]
    else:
        geno, pheno = O.synth_geno(rng, n, P), rng.standard_normal(n)
    perm = rng.permutation(n)
    T, V = perm[:n // 2 + 1], perm[n // 2 + 1:n - 3]
    genomes = [rng.choice(P, k, replace=False) for k in (1, 17, P // 2, P)] + [rng.integers(0, P, n + 5)]
    rows = np.sort(rng.integers(0, n, 2 * n))[::-1]
    yc = rng.standard_normal(len(rows))
    out = []
    for kw, data in (({}, geno), ({"snp_major": True}, np.ascontiguousarray(geno.T))):
        with _engine(data, pheno, **kw) as eng:
            assert (eng.n_animals, eng.n_snps) == (n, P)
            out.append((eng.evaluate(genomes, T, V, H2, return_ebv=True), eng.grm(), eng.grm(genomes[2]),
                        eng.snp_scan(rows, yc)))
    (ev0, g0, gi0, sc0), (ev1, g1, gi1, sc1) = out
    for x, y in zip(ev0 + (g0, gi0) + sc0, ev1 + (g1, gi1) + sc1):
        np.testing.assert_array_equal(x, y)
    assert _relmax(g0, O.make_grm(geno)) <= K_RTOL


# ---------------------------------------------------------------------------------------------
# G. decode
# ---------------------------------------------------------------------------------------------
def _stable_topk(keys, k):
    return np.argsort(keys, kind="stable")[-k:]


@pytest.fixture(scope="module")
def deng(gpu):
    rng = np.random.default_rng(2611)
    with _engine(O.synth_geno(rng, 64, 64), rng.standard_normal(64)) as eng:
        yield eng


def _decode_batch(d, kinds=None):
    """(labels, keys (B, d), lens) of one row length: every row kind at every k of that kind."""
    labels, keys, lens = [], [], []
    for kind, row, ks in H.edge_g_rows(d):
        if kinds is None or kind in kinds:
            for k in ks:
                labels.append((d, kind, k))
                keys.append(row)
                lens.append(k)
    return labels, np.array(keys), np.array(lens)


@pytest.mark.parametrize("kind", ["continuous", "rounded", "equal", "ascending", "descending", "zeros", "inf", "nan"])
def test_g_decode_small_rows(deng, kind):
    """d from 1 to 32769 (whole-row samples padded with zeros below d = 4096, k == d), bit-exact
    against a stable argsort: -0.0 ties with +0.0 by index, every NaN sorts above +inf."""
    bad = []
    for d in H.EDGE_G_D:
        labels, keys, lens = _decode_batch(d, (kind,))
        idx, off = deng.decode_randkey(keys, lens)
        for i, lab in enumerate(labels):
            if not np.array_equal(idx[off[i]:off[i + 1]], _stable_topk(keys[i], lens[i])):
                bad.append(lab)
    assert not bad, "rows (d, kind, k) that differ from np.argsort(kind='stable')[-k:]: %s" % bad


def test_g_decode_fallbacks(deng):
    """Rows whose strided sample misleads the threshold (tests/test_edge_cases_cpu.py checks they
    do): candidates overflow the 8192 slots / are fewer than k, so the row-wide radix select runs."""
    rows = H.edge_g_fallback_rows()
    keys = np.array([r[1] for r in rows])
    lens = np.array([r[2] for r in rows])
    idx, off = deng.decode_randkey(keys, lens)
    for i, (name, row, k) in enumerate(rows):
        np.testing.assert_array_equal(idx[off[i]:off[i + 1]], _stable_topk(row, k), err_msg=name)


def test_g_decode_device_entry_strided(deng):
    """tblup_decode_topk_device on a column slice of a wider matrix (ld > d) = the host entry."""
    import torch
    rng = np.random.default_rng(2612)
    for d in (65, 4097, 8193):
        labels, keys, lens = _decode_batch(d)
        wide = rng.uniform(5, 6, size=(len(keys), d + 37))          # larger keys all around the slice
        wide[:, 5:5 + d] = keys
        view = torch.from_numpy(wide).cuda()[:, 5:5 + d]
        assert view.stride(0) == d + 37 and not view.is_contiguous()
        got, off = deng.decode_randkey_tensor(view, d, lens)
        host, off_h = deng.decode_randkey(keys, lens)
        np.testing.assert_array_equal(off, off_h)
        np.testing.assert_array_equal(got, host)
        for i in range(len(labels)):
            np.testing.assert_array_equal(got[off[i]:off[i + 1]], _stable_topk(keys[i], lens[i]), err_msg=str(labels[i]))


# ---------------------------------------------------------------------------------------------
# H. GRM and scan, small
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 127, 128, 129])
def test_h_grm_small(gpu, n):
    rng = np.random.default_rng((2613, n))
    P = 70
    geno = O.synth_geno(rng, n, P, maf_lo=0.3)
    geno[0, 0], geno[1, 0] = 0, 2                     # column 0 is polymorphic at every n
    w = _Worst("H grm n=%d" % n)
    with _engine(geno, rng.standard_normal(n)) as eng:
        for k in (1, 63, 64, 65, 255, 257):
            idx = rng.integers(0, P, k)               # duplicates: k up to 257 from 70 columns
            idx[0] = 0
            G = eng.grm(idx)
            ref = O.make_grm(geno[:, idx])
            assert np.all(np.isfinite(ref))
            assert w.add("K", _relmax(G, ref)) <= K_RTOL, k
            np.testing.assert_array_equal(G, G.T)
    w.show()


@pytest.mark.parametrize("P", [1, 7, 8, 9])
def test_h_snp_scan_small(gpu, P):
    rng = np.random.default_rng((2614, P))
    n = 5000
    geno = O.synth_geno(rng, n, P)
    w = _Worst("H scan P=%d" % P)
    with _engine(geno, rng.standard_normal(n)) as eng:
        for nr in (1, 63, 64, 65, 4095, 4096, 4097, 8193):
            rows = np.sort(rng.integers(0, n, nr))[::-1].copy()
            if nr > 1:
                rows[1] = rows[0]
            yc = rng.standard_normal(nr)
            sx, sxx, sxy = eng.snp_scan(rows, yc)
            x = geno[rows].astype(np.int64)
            np.testing.assert_array_equal(sx, x.sum(axis=0))
            np.testing.assert_array_equal(sxx, (x * x).sum(axis=0))
            for s in range(P):
                terms = (x[:, s] * yc).tolist()       # x in {0, 1, 2}: the products are exact
                bound = 1e-12 * math.fsum(abs(t) for t in terms)
                err = abs(sxy[s] - math.fsum(terms))
                assert err <= bound, (nr, s, err, bound)
                w.add("sxy err / sum|x yc|", err / bound * 1e-12 if bound else 0.0)
    w.show()
