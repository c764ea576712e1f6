"""Diagonal kernel, wave count of the workgroup (TBLUP_DIAG_WAVES): the 8-wave kernel and the wide
one (16 waves, used where a diagonal launch carries no D- or E-units) run the same MFMA and fma
chains on the same operands -- only which wave takes a block, and when a finished block row of
X^T and its z leave the workgroup, differ -- so fitness, EBVs and the fitted effects (tblup_fit_batch
re-reads Dinv and z) must be bit-identical across the knob, with and without units beside the
diagonal workgroups (TBLUP_DIAG_E=1 TBLUP_DIAG_D=1: those launches keep the 8-wave kernel), in both
system forms and with 1 and 3 traits; and equal to the oracle.  (The knob is read when a context is
created.)

Batch: k = 16 (one pivot block of real rows), 100 (leading padding inside and across a block), 129,
300, 300 over a 3-tile-column system (n_T = 257), so the windows see whole padding blocks, a
partly padded block and full tiles, and the last window runs with and without X rows of real data."""
import os

import numpy as np
import pytest

from oracle import blup_oracle as O

pytestmark = pytest.mark.gpu

FIT_ATOL = 1e-9          # the parity suite's fitness bound (tests/test_gpu_parity.py)
H2 = 0.4
KS = (16, 100, 129, 300, 300)
WAVES = ("8", "16")
UNITS = ({}, {"TBLUP_DIAG_E": "1", "TBLUP_DIAG_D": "1"})


@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(77)
    n, p = 400, 2000
    geno = O.synth_geno(rng, n, p)
    pheno3 = rng.standard_normal((n, 3))
    perm = rng.permutation(n)
    T, V = perm[:257], perm[257:321]
    genomes = [rng.choice(p, k, replace=False) for k in KS]
    g64 = geno.astype(np.float64)
    # oracle fitness per trait (the engine's multi-trait fitness is the mean over traits)
    ref = np.array([[O.blup(g, T, V, g64, pheno3[:, t], H2) for t in range(3)] for g in genomes])
    return {"geno": geno, "pheno3": pheno3, "T": T, "V": V, "genomes": genomes, "ref": ref}


def _run(panel, env, traits):
    from tblup_amd.engine import GpuBlupEngine
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        pheno = panel["pheno3"][:, 0] if traits == 1 else panel["pheno3"][:, :traits]
        with GpuBlupEngine(panel["geno"], pheno, device=0) as eng:
            fit, ebv = eng.evaluate(panel["genomes"], panel["T"], panel["V"], H2, return_ebv=True)
            models = eng.fit(panel["genomes"], panel["T"], panel["V"], H2)
        return {"fit": fit, "ebv": ebv, "mfit": np.array([m.fitness for m in models]),
                "effects": [m.effects for m in models], "intercept": [m.intercept for m in models]}
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(a, b, msg):
    np.testing.assert_array_equal(a["fit"], b["fit"], err_msg=msg)
    np.testing.assert_array_equal(a["ebv"], b["ebv"], err_msg=msg)
    np.testing.assert_array_equal(a["mfit"], b["mfit"], err_msg=msg)
    for x, y in zip(a["effects"], b["effects"]):
        np.testing.assert_array_equal(x, y, err_msg=msg)
    for x, y in zip(a["intercept"], b["intercept"]):
        np.testing.assert_array_equal(x, y, err_msg=msg)


@pytest.mark.parametrize("traits", [1, 3])
@pytest.mark.parametrize("form", ["2", "1", None], ids=["snp", "kernel", "auto"])
def test_wave_counts_are_bit_identical(panel, gpu, form, traits):
    fenv = {} if form is None else {"TBLUP_FORM": form}
    first = None
    for units in UNITS:
        ref = None
        for waves in WAVES:
            env = dict(fenv, TBLUP_DIAG_WAVES=waves, **units)
            got = _run(panel, env, traits)
            assert np.all(np.isfinite(got["fit"])), env
            if ref is None:
                ref = got
            else:
                _same(got, ref, str(env))
        if first is None:
            first = ref
        else:
            _same(ref, first, f"units {units} against none, form {form}")
    want = panel["ref"][:, :traits].mean(axis=1)
    err = np.abs(first["fit"] - want)
    print("max |fitness - oracle|:", err.max())
    assert err.max() <= FIT_ATOL, err
    np.testing.assert_array_equal(first["mfit"], first["fit"])
