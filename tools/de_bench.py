"""Time the GPU DE step (tblup_de_step_device, pop x d on device) against the numpy
oracle of the reference's evolve loop on the host; prints one JSON line.

`de_bench.py mde_pbx [pop] [d] [generations]`: MDE_pBX.evolve per generation, the device
generation (draws, host resolve, step, the children's copy to the host) beside the host loop, in
one process on the same population; one JSON line with every generation's time."""
import ctypes
import json
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from tblup_amd import _native  # noqa: E402
from tblup_amd.evolver import GpuDEStep  # noqa: E402


def main(pop=256, d=50000, reps=20):
    step = GpuDEStep.get(0)
    lib = _native.load()
    rng = np.random.default_rng(0)
    par = torch.from_numpy(rng.uniform(size=(pop, d))).cuda()
    chi = torch.empty_like(par)
    donors = np.ascontiguousarray(rng.integers(0, pop, size=(pop, 3)), dtype=np.int32)
    fixed = np.ascontiguousarray(rng.integers(0, d, size=pop), dtype=np.int64)
    np.random.seed(0)
    st = np.random.get_state()
    key = np.array(st[1], dtype=np.uint32)
    pos = ctypes.c_int32(int(st[2]))
    U32 = ctypes.POINTER(ctypes.c_uint32)

    def run():
        _native.check("tblup_de_step_device", lib.tblup_de_step_device(
            step._ctx, 0, ctypes.c_void_p(par.data_ptr()), pop, d, d,
            donors.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            0.5, 0.8, 0, float(d - 1), key.ctypes.data_as(U32), ctypes.byref(pos), ctypes.c_void_p(chi.data_ptr()), d,
            None))
    t0 = time.perf_counter()
    run()
    first = time.perf_counter() - t0
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    # host path (tblup_de_step: H2D parents, D2H children)
    hp = par.cpu().numpy()
    t0 = time.perf_counter()
    step.step(0, hp, donors, fixed, 0.5, 0.8, False, d - 1)
    host_path = time.perf_counter() - t0
    # numpy oracle of the reference loop (host)
    from oracle import de_oracle as D
    genomes = [hp[i] for i in range(pop)]
    random.seed(0)
    t0 = time.perf_counter()
    D.de_generation(genomes, [0.0] * pop, 1, "de_rand_1", d, 0.8, 0.5, False)
    cpu = time.perf_counter() - t0
    print(json.dumps({"pop": pop, "d": d, "gpu_de_ms_median": 1e3 * float(np.median(ts)), "gpu_de_ms_min": 1e3 * min(ts),
                      "first_call_ms (incl. jump polynomials)": 1e3 * first, "host_pointer_path_ms": 1e3 * host_path,
                      "numpy_oracle_ms": 1e3 * cpu}))


class _Individual:
    """A RandomKey individual as the evolvers see it; deep copies take the genome along, as the
    reference's IndexIndividual.__deepcopy__ does (individual.py:110-118)."""
    _uid = 0

    def __init__(self, genome):
        _Individual._uid += 1
        self.uid = _Individual._uid
        self._genome = genome
        self.length = 100
        self.fitness = 0.0

    def get_internal_genome(self):
        return self._genome

    def set_internal_genome(self, genome):
        self._genome = genome

    def __deepcopy__(self, memo):
        cp = _Individual(None if self._genome is None else np.array(self._genome))
        cp.length, cp.fitness = self.length, self.fitness
        return cp


class _Population:
    def __init__(self, individuals, results_file):
        from types import SimpleNamespace
        self.population = individuals
        self.generation = 1
        self.monitor = SimpleNamespace(results_file=results_file)

    def __getitem__(self, i):
        return self.population[i]

    def __len__(self):
        return len(self.population)


def mde_pbx(pop=256, d=50000, gens=7):
    import os
    import tempfile
    from tblup_amd.evolver import MDE_pBX
    rng = np.random.default_rng(0)
    keys = rng.uniform(size=(pop, d))
    fit = rng.uniform(size=pop)
    out = {"mode": "mde_pbx", "pop": pop, "d": d}
    with tempfile.TemporaryDirectory() as tmp:
        for name, device in (("device", True), ("host_loop", False)):
            random.seed(0)
            np.random.seed(0)
            inds = [_Individual(keys[i].copy()) for i in range(pop)]
            for x, f in zip(inds, fit):
                x.fitness = float(f)
            popn = _Population(inds, os.path.join(tmp, name + ".csv"))
            ev = MDE_pBX(d, 1000, True)
            ev.device_step = device
            before = MDE_pBX.fallbacks
            ts = []
            for g in range(1, gens + 2):   # the first generation (polynomials, page-locking) is not timed
                popn.generation = g
                t0 = time.perf_counter()
                kids = ev.evolve(popn)
                torch.cuda.synchronize()
                if g > 1:
                    ts.append(1e3 * (time.perf_counter() - t0))
                del kids
            out[name + "_ms"] = [round(t, 3) for t in ts]
            out[name + "_ms_median"] = round(float(np.median(ts)), 3)
            out[name + "_fallbacks"] = MDE_pBX.fallbacks - before
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "mde_pbx":
        mde_pbx(*(int(a) for a in sys.argv[2:5]))
    else:
        main()
