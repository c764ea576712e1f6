"""The reliability restatement (tests/reliability_ref.py) against its own wider computation, its two
forms against each other, and the host side of the interface (no GPU).

The GPU tests compare against rel_ref at 1e-9 absolute; here rel_ref is shown to be within 1e-11 of an
np.longdouble computation on every case they use (measured: <= 2e-15), so that bound has room.
"""
import os
import re

import numpy as np

from tests import model_ref as R
from tests import reliability_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11


def _inputs():
    pn = Q.panel()
    for name, s, k, br in Q.cases():
        yield name, pn["genomes"][k], pn["splits"][s][0], pn["geno"], br
    dp = Q.deep_panel()
    yield "deep", dp["genome"], dp["train"], dp["geno"], "auto"


def test_ref_matches_wide_and_forms_agree():
    worst = {"wide": 0.0, "forms": 0.0}
    lo, hi = 1.0, 0.0
    for name, idx, T, geno, br in _inputs():
        ref = Q.case_ref(name) if name != "deep" else Q.deep_ref()
        wide = Q.rel_wide(idx, T, geno, Q.H2, br)
        assert ref.shape == (geno.shape[0],) and np.all(np.isfinite(ref)), name
        worst["wide"] = max(worst["wide"], float(np.max(np.abs(ref - wide))))
        assert np.max(np.abs(ref - wide)) <= TOL, name
        snp = Q.rel_ref(idx, T, geno, Q.H2, br, form="snp")
        ker = Q.rel_ref(idx, T, geno, Q.H2, br, form="kernel")
        for other in (snp, ker):
            worst["forms"] = max(worst["forms"], float(np.max(np.abs(other - ref))))
            assert np.max(np.abs(other - ref)) <= TOL, name
        assert np.all(ref >= 0.0) and np.all(ref < 1.0), name
        lo, hi = min(lo, float(ref.min())), max(hi, float(ref.max()))
    print("\nRELIABILITY host: max |ref - wide| %.3e, max |form - ref| %.3e, values in [%.3f, %.3f]"
          % (worst["wide"], worst["forms"], lo, hi))


def test_train_animals_are_more_reliable():
    """A sanity check of the definition: with many SNPs an animal the model was trained on is known
    better than one it never saw."""
    pn = Q.panel()
    T, V = pn["splits"][257, 70]
    r = Q.case_ref("auto-257-70-200")
    rest = np.setdiff1d(np.arange(R.N_ANIMALS), T)
    assert r[T].mean() > r[rest].mean()


def test_monomorphic_panel_is_nan():
    pn = Q.panel()
    geno = pn["geno"].copy()
    geno[:, 0] = 0
    T = pn["splits"][129, 64][0]
    assert np.all(np.isnan(Q.rel_ref(np.array([0]), T, geno, Q.H2)))


def test_header_declares_the_entry():
    src = open(os.path.join(ROOT, "include", "tblup_gpu.h")).read()
    m = re.search(r"int tblup_reliability_batch\(([^;]*)\);", src)
    assert m, "include/tblup_gpu.h does not declare tblup_reliability_batch"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 14
    assert args[2] == "const int64_t* animals" and args[-1] == "double* reliability"


def test_native_signature_table():
    from tblup_amd import _native
    assert "tblup_reliability_batch" in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES["tblup_reliability_batch"]
    assert len(argtypes) == 14


def test_python_surface():
    import inspect
    from tblup_amd.engine import GpuBlupEngine
    from tblup_amd.evaluator import BlupParallelEvaluator
    sig = inspect.signature(GpuBlupEngine.reliability)
    assert list(sig.parameters)[1:] == ["genomes", "train", "valid", "h2", "animals", "branch"]
    assert inspect.signature(GpuBlupEngine.fit).parameters["reliability_of"].default is None
    sig = inspect.signature(BlupParallelEvaluator.reliability)
    assert list(sig.parameters)[1:] == ["population", "animals", "final", "train", "valid"]
    assert inspect.signature(BlupParallelEvaluator.fit_models).parameters["reliability_of"].default is None
