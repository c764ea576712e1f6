"""MDE_pBX's generation on the GPU (tblup_mde_draws / tblup_mde_resolve / tblup_mde_step_device_async)
against the host loop, bit for bit: children, dtypes, numpy's (key, pos), python's random state."""
import os
import random
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests.helpers import KeyIndividual, Pop, RandomKeyIndividual
from tests.test_evolver import ADAPT, MDE_META, _adaptive_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_MAX = 100
# (L, pop, pre-drawn words): block-boundary lengths, even and odd C_i
SMALL = [(1, 4, 0), (15, 12, 3), (311, 5, 1), (312, 7, 624), (313, 6, 622)]
# generation 2: p = ceil(pop / 2 * 0.98); generation 99: p == 1, the parent choice draws no word
# (pop 6: int(0.15 pop) == 0, q_best is the whole population)
GENS = (2, 99)


def _mde(L, clip, device):
    from tblup_amd.evolver import MDE_pBX
    ev = MDE_pBX(L, G_MAX, clip)
    ev.device_step = device
    return ev


def _population(L, pop, gen, tmp_path):
    rng = np.random.default_rng(L * 7 + pop)
    keys = rng.uniform(size=(pop, L)) * (L if L > 1 else 1.0) * 1.5 - 0.2   # some values outside [0, L - 1]
    inds = [KeyIndividual(keys[i].copy(), 1) for i in range(pop)]
    for ind, f in zip(inds, rng.uniform(size=pop)):
        ind.fitness = float(f)
    popn = Pop(inds, gen)
    popn.monitor = SimpleNamespace(results_file=str(tmp_path / "results.csv"))
    return popn


def one_generation(L, pop, pre, gen, clip, tmp_path, seed=0):
    """The device generation and the host loop from identical RNG states; returns the C_i the host
    resolved."""
    from tblup_amd.evolver import GpuDEStep
    got_c = []
    orig = GpuDEStep.mde_draws

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        if isinstance(out, tuple):
            got_c.append(out[3].copy())
        return out
    runs = []
    for device in (True, False):
        random.seed(L + seed)
        np.random.seed(pop + seed)
        np.random.bytes(4 * pre)
        ev = _mde(L, clip, device)
        GpuDEStep.mde_draws = spy
        try:
            kids = ev.evolve(_population(L, pop, gen, tmp_path))
        finally:
            GpuDEStep.mde_draws = orig
        runs.append(([np.asarray(k.get_internal_genome()) for k in kids], random.getstate(), np.random.get_state(),
                     (ev.cr_m, ev.f_m, ev.p, list(ev.crs), list(ev.fs))))
    (kd, pyd, npd, sd), (kh, pyh, nph, sh) = runs
    tag = (L, pop, pre, gen, clip)
    assert pyd == pyh, tag
    assert np.array_equal(npd[1], nph[1]) and npd[2] == nph[2], tag
    assert sd == sh, tag
    for a, b in zip(kd, kh):
        assert a.dtype == b.dtype and np.array_equal(a, b), tag
    return got_c


def run_shapes(shapes, tmp_path):
    for L, pop, pre in shapes:
        cs = []
        for gen in GENS:
            for clip in (True, False):
                cs += one_generation(L, pop, pre, gen, clip, tmp_path)
        assert len(cs) == 2 * len(GENS), "a generation fell back to the host loop"
        c = np.concatenate(cs)
        assert np.any(c % 2 == 0) and np.any(c % 2 == 1), (L, pop, pre)   # both parities of C_i


def _child():
    import tempfile
    from pathlib import Path
    with tempfile.TemporaryDirectory() as d:
        run_shapes(SMALL + [(64, 40, 5)], Path(d))
    print("mde child ok")


def test_mde_small_shapes_vs_host_loop(gpu, tmp_path):
    run_shapes(SMALL, tmp_path)


def test_mde_split_form_whole_blocks_skipped(gpu, tmp_path):
    """pop 700 > the CU count: the three-launch form; C_i passes 624 and 1248."""
    cs = []
    for clip in (True, False):
        cs += one_generation(64, 700, 5, 2, clip, tmp_path)
    c = np.concatenate(cs)
    assert c.max() > 1248 and np.any(c % 2 == 0) and np.any(c % 2 == 1)


def test_mde_two_mask_segments(gpu, tmp_path):
    """L = 70000: two 65536-element mask segments of the three-launch form, crossed at odd offsets."""
    for clip in (True, False):
        c = np.concatenate(one_generation(70000, 384, 5, 2, clip, tmp_path))
        assert np.any(c % 2 == 0) and np.any(c % 2 == 1), clip


@pytest.mark.parametrize("split", ["4", "100000"])
def test_mde_small_shapes_forced_launch_form(gpu, split):
    """TBLUP_DE_SPLIT is read when the library first runs a step: a fresh process, once low enough
    for the three-launch form at every shape, once high enough for the one-launch form."""
    env = dict(os.environ, TBLUP_DE_SPLIT=split)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_mde import _child; _child()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mde child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_mde_forced_overflow_falls_back_to_host_loop(gpu, tmp_path, monkeypatch):
    from tblup_amd.evolver import MDE_pBX
    monkeypatch.setenv("TBLUP_MDE_SLACK", "0")
    before = MDE_pBX.fallbacks
    assert one_generation(15, 40, 3, 2, True, tmp_path) == []
    assert MDE_pBX.fallbacks == before + 1


def test_mde_step_rejects_what_its_draws_do_not_cover(gpu):
    """The step continues one tblup_mde_draws: c_words past those draws' windows (every workgroup
    would walk c_words / 624 blocks) and a step without matching draws are argument / state errors."""
    import torch
    from tblup_amd import _native
    from tblup_amd.evolver import GpuDEStep
    step = GpuDEStep.get(0)
    pop, L = 8, 16
    np.random.seed(1)
    random.seed(1)
    parents = torch.rand(pop, L, dtype=torch.float64, device="cuda:0")
    drawn = step.mde_draws(pop, L, [1, 2, 3], [0, 4, 5, 6, 7])
    assert isinstance(drawn, tuple)
    parent, donors, fixed, c_words = drawn
    F, cr = np.full(pop, 0.5), np.full(pop, 0.5)
    bad = c_words.copy()
    bad[-1] += 10_000
    with pytest.raises(_native.TblupError, match="c_words exceeds"):
        step.step_device(1, parents, donors, fixed, F, cr, True, L - 1, mde=(parent, bad))
    bad = c_words.copy()
    bad[0] = -1
    with pytest.raises(_native.TblupError, match="non-decreasing"):
        step.step_device(1, parents, donors, fixed, F, cr, True, L - 1, mde=(parent, bad))
    kids = step.step_device(1, parents, donors, fixed, F, cr, True, L - 1, mde=(parent, c_words))   # still usable
    assert kids.shape == parents.shape
    with pytest.raises(_native.TblupError, match="no tblup_mde_draws"):   # the draws are used up
        step.step_device(1, parents, donors, fixed, F, cr, True, L - 1, mde=(parent, c_words))


@pytest.mark.parametrize("name", sorted(MDE_META))
def test_mde_goldens_through_the_gpu(gpu, name, tmp_path):
    """The reference's recorded runs (tests/golden/mde.npz), every generation on the device;
    mde_index: non-float64 parents."""
    from tblup_amd import evolver as EV

    def make(d, g, clip):
        ev = EV.MDE_pBX(d, g, clip)
        ev.device_step = True
        return ev
    before = EV.MDE_pBX.fallbacks
    z = np.load(os.path.join(ADAPT, "mde.npz"))
    resolved = []
    orig = EV.GpuDEStep.mde_draws

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        resolved.append(isinstance(out, tuple))
        return out
    EV.GpuDEStep.mde_draws = spy
    try:
        _adaptive_run(z, name, MDE_META[name], make, (900, 1000, 800), tmp_path,
                      lambda ev: [ev.cr_m, ev.f_m, ev.p, len(ev.successful_crs), len(ev.successful_fs)])
    finally:
        EV.GpuDEStep.mde_draws = orig
    assert resolved == [True] * MDE_META[name][4]   # every generation's draws resolved on the device path
    assert EV.MDE_pBX.fallbacks == before


def test_mde_generations_with_device_keystore(gpu, tmp_path):
    """evolve -> evaluate -> select for 3 generations of mde_pbx: with the device generation the
    children are decoded from their device rows; fitnesses and populations equal the host loop's."""
    from oracle import blup_oracle as O
    from tblup_amd.engine import GpuBlupEngine
    from tblup_amd.evaluator import BlupParallelEvaluator
    from tblup_amd.evolver import MDE_pBX
    from tblup_amd.keystore import DeviceKeyStore
    rng = np.random.default_rng(12)
    n, p, k, pop = 400, 3000, 150, 24
    geno = O.synth_geno(rng, n, p)
    pheno = rng.standard_normal(n)
    np.save(tmp_path / "g.npy", geno)
    np.save(tmp_path / "y.npy", pheno)
    keys0 = rng.uniform(size=(pop, p))

    def run(device):
        random.seed(6)
        np.random.seed(6)
        ev = BlupParallelEvaluator(str(tmp_path / "g.npy"), str(tmp_path / "y.npy"), 0.4)
        inds = [RandomKeyIndividual(keys0[i].copy(), k) for i in range(pop)]
        fits = []
        with ev:
            popn = Pop(inds, 0)
            popn.monitor = SimpleNamespace(results_file=str(tmp_path / ("results_%d.csv" % device)))
            ev.evaluate(popn, popn, 0)
            evo = MDE_pBX(p, 10, True)
            evo.device_step = device
            for g in range(1, 4):
                popn.generation = g
                if not device:
                    DeviceKeyStore.get(0).clear()
                kids = evo.evolve(popn)
                if device:
                    assert all(h is not None for h in DeviceKeyStore.get(0).rows(kids))
                ev.evaluate(popn, kids, g)
                popn.population = [c if c.fitness > q.fitness else q for q, c in zip(popn.population, kids)]
                fits.append([x.fitness for x in kids])
            genomes = [x.get_internal_genome().copy() for x in popn.population]
        return fits, genomes

    calls = []
    orig = GpuBlupEngine.decode_randkey_tensor

    def spy(self, *a, **kw):
        calls.append(1)
        return orig(self, *a, **kw)
    GpuBlupEngine.decode_randkey_tensor = spy
    try:
        f_dev, g_dev = run(True)
    finally:
        GpuBlupEngine.decode_randkey_tensor = orig
    assert len(calls) == 3   # the children were decoded in place from the device key store
    f_host, g_host = run(False)
    assert f_dev == f_host
    for a, b in zip(g_dev, g_host):
        assert np.array_equal(a, b)
