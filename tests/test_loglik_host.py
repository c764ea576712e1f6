"""The log-likelihood restatement (tests/loglik_ref.py) against the contrast likelihood it abbreviates
and against its own wider computation, and the host side of the interface (no GPU).

The GPU tests compare against loglik_ref at 1e-9 max(1, |ref|); here loglik_ref is shown to be within
1e-11 max(1, |ref|) of an np.longdouble Cholesky computation of the same quantities on every case they
use, two orders below that bound (the largest difference is printed).
"""
import ctypes
import inspect
import os
import re

import numpy as np

from tests import loglik_ref as LL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_TOL = LL.TOL / 100


def test_restricted_likelihood_is_the_contrast_likelihood():
    """snp branch: the closed form (log|V| - log lambda, centred y) equals the likelihood of the N - 1
    error contrasts with an explicit orthonormal A."""
    pn = LL.panel()
    worst = 0.0
    for s, k in (((127, 5), 63), ((127, 5), 200), ((128, 2), "dup"), ((129, 64), 129), ((129, 64), 400)):
        T = pn["splits"][s][0]
        for h2 in LL.H2S:
            ref = LL.loglik_ref(pn["genomes"][k], T, pn["geno"], pn["pheno"], h2, "snp")
            con = LL.loglik_contrast(pn["genomes"][k], T, pn["geno"], pn["pheno"], h2)
            worst = max(worst, LL.close(ref, con))
    print("\nLOGLIK host: max |ref - contrast| / max(1, |ref|) %.3e" % worst)
    assert worst <= 1e-10


def test_ref_matches_wide():
    pn = LL.panel()
    worst, lo, hi = 0.0, np.inf, -np.inf
    for name, s, k, br in LL.cases():
        for h2 in LL.H2S:
            ref = LL.case_ref(name, h2)
            assert np.all(np.isfinite(ref)), (name, h2)
            wide = LL.loglik_wide(pn["genomes"][k], pn["splits"][s][0], pn["geno"], pn["pheno"], h2, br)
            err = max(float(abs(ref[i] - wide[i]) / max(1.0, abs(float(wide[i])))) for i in (0, 1))
            worst = max(worst, err)
            assert err <= WIDE_TOL, (name, h2, err)
            lo, hi = min(lo, ref[0]), max(hi, ref[0])
    dp = LL.deep_panel()
    for h2 in LL.H2S:
        ref = LL.deep_ref(h2)
        wide = LL.loglik_wide(dp["genome"], dp["train"], dp["geno"], dp["pheno"], h2)
        err = max(float(abs(ref[i] - wide[i]) / max(1.0, abs(float(wide[i])))) for i in (0, 1))
        worst = max(worst, err)
        assert err <= WIDE_TOL, ("deep", h2, err)
    print("\nLOGLIK host: max |ref - wide| / max(1, |wide|) %.3e over loglik and sigma2_g, loglik in [%.1f, %.1f]"
          % (worst, lo, hi))


def test_traits_share_the_determinant():
    pn = LL.panel()
    T = pn["splits"][129, 64][0]
    for k, br in ((64, "auto"), (200, "gblup")):
        multi = LL.loglik_ref(pn["genomes"][k], T, pn["geno"], pn["Y"], 0.3, br)
        for t in range(4):
            one = LL.loglik_ref(pn["genomes"][k], T, pn["geno"], pn["Y"][:, t], 0.3, br)
            assert LL.close([multi[0][t], multi[1][t]], one) <= 1e-12


def test_monomorphic_panel_is_nan():
    pn = LL.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    T = pn["splits"][129, 64][0]
    assert np.all(np.isnan(LL.loglik_ref(np.array([0]), T, geno, pn["pheno"], 0.3)))
    assert np.isnan(LL.estimate_ref(np.array([0]), T, geno, pn["pheno"])["h2"])


def test_estimate_ref_finds_the_maximum():
    """The procedure on the restatement: the best point is no worse than every grid value and than its
    neighbours one final step away."""
    pn = LL.panel()
    T = pn["splits"][129, 64][0]
    g = pn["genomes"][64]
    est = LL.estimate_ref(g, T, pn["geno"], pn["pheno"])
    assert 0.02 <= est["h2"] <= 0.98 and abs(est["step"] - 0.04 / 4 ** 3) < 1e-12
    for h in list(np.linspace(0.02, 0.98, 25)) + [est["h2"] - est["step"], est["h2"] + est["step"]]:
        if 0.0 < h < 1.0:
            assert LL.loglik_ref(g, T, pn["geno"], pn["pheno"], float(h))[0] <= est["loglik"] + 1e-9
    assert est["at_bound"] == (est["h2"] in (0.02, 0.98))


def test_header_declares_the_entry():
    src = open(os.path.join(ROOT, "include", "tblup_gpu.h")).read()
    m = re.search(r"int tblup_loglik_batch\(([^;]*)\);", src)
    assert m, "include/tblup_gpu.h does not declare tblup_loglik_batch"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["tblup_ctx* ctx", "int split_id", "const int64_t* idx", "const int64_t* offsets", "int64_t batch",
                    "const double* h2", "int64_t n_h2", "int branch", "double* fitness", "double* loglik",
                    "double* sigma2_g"]


def test_library_exports_the_entry_with_the_documented_signature():
    from tblup_amd import _native
    lib = _native.load()                                   # as tests/test_abi.py loads it
    assert hasattr(lib, "tblup_loglik_batch")
    restype, argtypes = _native.SIGNATURES["tblup_loglik_batch"]
    i64p, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_int, i64p, i64p, ctypes.c_int64, dp, ctypes.c_int64, ctypes.c_int,
                        dp, dp, dp]
    assert lib.tblup_loglik_batch.argtypes == argtypes


def test_argument_errors_without_a_device():
    from tblup_amd import _native
    lib = _native.load()
    one = np.zeros(1, dtype=np.int64)
    off = np.array([0, 1], dtype=np.int64)
    h2 = np.array([0.3])
    out = np.zeros(1)
    i64, f64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    rc = lib.tblup_loglik_batch(None, 0, one.ctypes.data_as(i64), off.ctypes.data_as(i64), 1, h2.ctypes.data_as(f64), 1,
                                0, None, out.ctypes.data_as(f64), None)
    assert rc == -1                                        # a null context is an argument error, not a crash
    assert isinstance(lib.tblup_last_error(), bytes) and lib.tblup_last_error()


def test_python_surface():
    from tblup_amd.engine import GpuBlupEngine
    from tblup_amd.evaluator import BlupParallelEvaluator
    sig = inspect.signature(GpuBlupEngine.log_likelihood)
    assert list(sig.parameters)[1:] == ["genomes", "train", "valid", "h2", "branch", "return_sigma2"]
    assert sig.parameters["branch"].default == "auto" and sig.parameters["return_sigma2"].default is False
    sig = inspect.signature(GpuBlupEngine.estimate_h2)
    assert list(sig.parameters)[1:] == ["genomes", "train", "valid", "branch", "grid", "refine", "points"]
    assert sig.parameters["refine"].default == 3 and sig.parameters["points"].default == 9
    np.testing.assert_array_equal(sig.parameters["grid"].default, np.linspace(0.02, 0.98, 25))
    sig = inspect.signature(BlupParallelEvaluator.estimate_h2)
    assert list(sig.parameters)[1:5] == ["population", "final", "train", "valid"]
    sig = inspect.signature(BlupParallelEvaluator.log_likelihood)
    assert list(sig.parameters)[1:3] == ["population", "h2"]
