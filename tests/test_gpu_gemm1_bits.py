"""Off-diagonal GEMM1 stage loop (k_chol.hip gemm1_a32): the fitnesses of a small SNP-form panel are
bit-identical to those recorded from the library as it stood before the loop's B-operand prefetch
was reordered (tests/golden/gemm1_parent_bits.npz, written by tests/golden/make_gemm1_golden.py),
and equal to the oracle within the parity suite's FIT_ATOL.  The reorder moves loads and waits only:
no MFMA changes place in an accumulator chain, so any differing bit is a stale or early-read operand.

Panel 520 animals x 2000 SNPs, n_T = 400, n_V = 100: k <= n_T keeps the SNP form, up to 3 tile
columns.  The k of a genome chooses the path through the loop (leading padding pad = 128 NT - k):
  k = 129  NT 2, pad 127: three whole stages skipped, the peeled stage from k-step 7
  k = 200  pad 56: one stage skipped, the peeled stage from k-step 6
  k = 256  no padding: main loop only, nL = 1
  k = 300  NT 3, pad 84
  k = 384  NT 3, no padding, nL = 2: the loop crosses a tile boundary
Batches: B = 1 (each k) and B = 3; B = 70, which brings D- and E-units into the diagonal launch;
B = 3 under TBLUP_AHEAD=1 (P-units); one 3-trait batch (k_chol_offdiag<MAXT>)."""
import os

import numpy as np
import pytest

from oracle import blup_oracle as O

pytestmark = pytest.mark.gpu

FIT_ATOL = 1e-9          # the parity suite's fitness bound (tests/test_gpu_parity.py)
H2 = 0.4
KS = (129, 200, 256, 300, 384)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm1_parent_bits.npz")

# name -> (k of each genome, environment, traits)
CASES = {}
for _k in KS:
    CASES[f"b1_k{_k}"] = ((_k,), {}, 1)
CASES["b3_lo"] = ((129, 200, 256), {}, 1)
CASES["b3_hi"] = ((300, 384, 200), {}, 1)
CASES["b70"] = (tuple(KS[i % 5] for i in range(70)), {}, 1)
CASES["b3_lo_ahead"] = ((129, 200, 256), {"TBLUP_AHEAD": "1"}, 1)
CASES["b3_hi_ahead"] = ((300, 384, 200), {"TBLUP_AHEAD": "1"}, 1)
CASES["b5_traits3"] = (KS, {}, 3)


def make_panel():
    """The panel and every case's genomes, from fixed seeds (shared with make_gemm1_golden.py)."""
    rng = np.random.default_rng(950)
    n, p = 520, 2000
    geno = O.synth_geno(rng, n, p)
    pheno3 = rng.standard_normal((n, 3))
    perm = rng.permutation(n)
    T, V = perm[:400], perm[400:500]
    genomes = {}
    for ci, (name, (ks, _, _)) in enumerate(CASES.items()):
        grng = np.random.default_rng(9500 + ci)
        genomes[name] = [grng.choice(p, k, replace=False) for k in ks]
    return {"geno": geno, "pheno3": pheno3, "T": T, "V": V, "genomes": genomes}


def run_case(panel, name):
    """The case's fitnesses from the loaded library."""
    from tblup_amd.engine import GpuBlupEngine
    _, env, traits = CASES[name]
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        pheno = panel["pheno3"][:, 0] if traits == 1 else panel["pheno3"][:, :traits]
        with GpuBlupEngine(panel["geno"], pheno, device=0) as eng:
            return eng.evaluate(panel["genomes"][name], panel["T"], panel["V"], H2)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def panel():
    return make_panel()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(CASES))
def test_gemm1_fitness_bits(panel, golden, gpu, name):
    assert int(panel["geno"].astype(np.int64).sum()) == int(golden["geno_sum"]), "panel differs from the golden's"
    fit = np.asarray(run_case(panel, name))
    ks, _, traits = CASES[name]
    assert fit.shape == (len(ks),) and np.all(np.isfinite(fit))
    assert np.array_equal(fit, golden[name]), (name, fit - golden[name])
    g64 = panel["geno"].astype(np.float64)
    # the oracle on one genome of every k in the batch
    first = {k: i for i, k in reversed(list(enumerate(ks)))}
    for k, i in first.items():
        g = panel["genomes"][name][i]
        want = np.mean([O.blup(g, panel["T"], panel["V"], g64, panel["pheno3"][:, t], H2) for t in range(traits)])
        assert abs(fit[i] - want) <= FIT_ATOL, (name, k, fit[i], want)
