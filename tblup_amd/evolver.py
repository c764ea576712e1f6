"""Drop-in DE evolvers whose generation step runs on the GPU.

Mirrors `tblup/evolver.py` for the two classic strategies:

* `DERandOneEvolver` (evolver.py:86-157): mutant = a + F (b - c)
* `DECurrentToBestOneEvolver` (evolver.py:160-244): mutant = x + F (best - x) + F (a - b),
  always clipped (the reference's `evolve` never passes `self.clip`, evolver.py:239-244)

with the reference's binary crossover (evolver.py:63-82) and F = 5 on every 5th
generation.  The per-individual python-`random` draws (the donors through
`exclusive_randrange`, utils.py:21-36, and the forced crossover position,
evolver.py:76) stay on the host in the reference's order; numpy's global MT19937
stream, which the reference consumes with one `np.random.rand(L)` per individual,
is jumped ahead on the GPU (k_de.hip, mt_jump.cpp) so every individual's
uniforms, mutant, crossover and clip are computed in parallel.  The children's
genomes and the numpy / python RNG states afterwards are bit-identical to the
reference's sequential loop (tests/test_evolver.py, tests/test_gpu_evolver.py).

The adaptive evolvers keep the reference's bookkeeping (AdaptiveEvolver, evolver.py:297-404) on
the host.  SaDE (evolver.py:407-547) runs its generation on the GPU too: every individual's
strategy (python's random.random() < p) and crossover rate are drawn on the host in the
reference's order and the step takes them per individual (tblup_de_step_device_async_mix; numpy's
stream still holds one np.random.rand(L) per individual).  MDE_pBX (evolver.py:550-687) draws
np.random.choice (rejection-sampled randint) between the individuals' np.random.rand(L) calls, so
each individual's numpy stream offset depends on the draws before it: the device expands the few
stream words those draws can read, native host code resolves them in order, and the GPU step
starts every individual's uniforms at its own offset (GpuDEStep.mde_draws; the reference's host
loop is kept for machines without a device and as the tests' reference, see MDE_pBX).
There is no CPU fallback for the other GPU steps: without the HIP library, `evolve` raises ImportError.
"""
import abc
import csv
import ctypes
import os
import random
from copy import deepcopy
from math import ceil

import numpy as np

from . import _native
from .distributed import shard_range, world
from .hostrows import _BLOCKS, HostRows
from .keystore import DeviceKeyStore, freeze_heap, work_stream


def get_evolver(args):
    """evolver.py:13-32 for the strategies this package runs on the GPU."""
    if args.de_strategy == "de_rand_1":
        return DERandOneEvolver(args.dimensionality, args.crossover_rate, args.mutation_intensity, args.clip)
    if args.de_strategy == "de_currenttobest_1":
        return DECurrentToBestOneEvolver(args.dimensionality, args.crossover_rate, args.mutation_intensity, args.clip)
    if args.de_strategy == "sade":
        return SaDE(args.dimensionality, args.clip)
    if args.de_strategy == "mde_pbx":
        return MDE_pBX(args.dimensionality, args.generations, args.clip)
    raise NotImplementedError("Evolver with config option {} is not implemented.".format(args.de_strategy))


def exclusive_randrange(begin, end, exclude):
    """utils.py:21-36, same python-`random` consumption (first draw before the assert)."""
    r = random.randrange(begin, end)
    exclude = set(exclude)
    assert len(exclude) < (end - begin), "Exclusion range larger than random range."
    while r in exclude:
        r = random.randrange(begin, end)
    return r


def _rand_one_draws(n, L, i):
    """Individual i's python-`random` draws of DE/rand/1 in the reference's order: the donors (a, b, c)
    of de_rand_one (evolver.py:118-121), then the crossover's forced position (evolver.py:76)."""
    a = exclusive_randrange(0, n, [i])
    b = exclusive_randrange(0, n, [i, a])
    c = exclusive_randrange(0, n, [i, a, b])
    return (a, b, c), random.randrange(0, L)


def _current_to_best_draws(n, L, i, best):
    """The same of DE/current-to-best/1: (best, a, b) (evolver.py:199-203), then the forced position.
    i: the index excluded along with best's -- the individual's own, or MDE_pBX's parent_idx."""
    a = exclusive_randrange(0, n, [i, best])
    b = exclusive_randrange(0, n, [i, best, a])
    return (best, a, b), random.randrange(0, L)


def _draw_donors(n, draws):
    """(donors, fixed) of a generation from draws(i), individual by individual."""
    donors = np.empty((n, 3), dtype=np.int32)
    fixed = np.empty(n, dtype=np.int64)
    for i in range(n):
        donors[i], fixed[i] = draws(i)
    return donors, fixed


def _best_index(population):
    best = max(population, key=lambda individual: individual.fitness)   # evolver.py:235
    return population.population.index(best)                            # evolver.py:194


def _native_donors(strategy, n, L, best=-1):
    """One generation's donor / fixed-position draws (the python loop of _draw_donors) on
    CPython's MT19937 state in native code (tblup_de_donors): the same draws and the same
    `random` state afterwards, without 4n interpreted randrange calls.  None when the loop must
    stay in python (n < 4 raises the reference's assertion there; n > 65535 or L >= 2^32)."""
    if n < 4 or n > 65535 or L >= 1 << 32:
        return None
    mt, idx = _native.py_random_state()
    donors = np.empty((n, 3), dtype=np.int32)
    fixed = np.empty(n, dtype=np.int64)
    ptr = _native.ptr
    _native.check("tblup_de_donors", _native.load().tblup_de_donors(
        strategy, n, L, best, ptr(mt), ptr(idx), ptr(donors), ptr(fixed)))
    _native.set_py_random_state(mt, idx)
    return donors, fixed


class GpuDEStep:
    """A panel-less GPU context running tblup_de_step (one per process and device)."""

    _instances = {}

    @classmethod
    def get(cls, device=None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        inst = cls._instances.get(device)
        if inst is None:
            inst = cls._instances[device] = cls(device)
        return inst

    def __init__(self, device=0):
        self._lib = _native.load()
        freeze_heap()
        ctx = ctypes.c_void_p()
        _native.check("tblup_ctx_create", self._lib.tblup_ctx_create(None, 0, 0, 0, None, int(device),
                                                                     ctypes.byref(ctx)))
        self._ctx = ctx
        self.device = int(device)

    def _rng_state(self):
        """numpy's global MT19937 state as (key, pos) buffers for the library to advance, and
        hand_back(): makes them numpy's state again (the cached gaussian is kept)."""
        st = np.random.get_state()
        if st[0] != "MT19937":
            raise RuntimeError("numpy's global RandomState is not MT19937")
        key, pos = np.array(st[1], dtype=np.uint32), ctypes.c_int32(int(st[2]))

        def hand_back():
            np.random.set_state(("MT19937", key, pos.value, st[3], st[4]))
        return key, pos, hand_back

    def step(self, strategy, parents, donors, fixed, F, cr, clip, clip_hi):
        """children (pop x L) for the current numpy global state, which is advanced
        past the generation's pop x L uniforms exactly as the reference's loop does."""
        parents = np.ascontiguousarray(parents, dtype=np.float64)
        pop, L = parents.shape
        donors = np.ascontiguousarray(donors, dtype=np.int32)
        fixed = np.ascontiguousarray(fixed, dtype=np.int64)
        key, pos, hand_back = self._rng_state()
        children = np.empty_like(parents)
        ptr = _native.ptr
        _native.check("tblup_de_step", self._lib.tblup_de_step(
            self._ctx, int(strategy), ptr(parents), pop, L, ptr(donors), ptr(fixed), float(F), float(cr),
            1 if clip else 0, float(clip_hi), ptr(key), ctypes.byref(pos), ptr(children)))
        hand_back()
        return children

    def mde_draws(self, pop, L, q_idx, p_idx, slack=-1):
        """The draws of one MDE_pBX generation for numpy's and python's current global states: the
        device expands every individual's window of numpy's stream (tblup_mde_draws), the host
        resolves the np.random.choice draws from it and makes python's (tblup_mde_resolve).  q_idx /
        p_idx: the population indices to choose the group best / the parent from.  Returns (parent,
        donors, fixed, c_words) with python's `random` state advanced, numpy's untouched (the step
        advances it).  With neither state touched: None when a rejection run left its window, False
        when the windows exceed 2^26 words (tens of thousands of individuals with choice sizes just
        above a power of two), before anything runs on the device."""
        import torch
        q_idx = np.ascontiguousarray(q_idx, dtype=np.int32)
        p_idx = np.ascontiguousarray(p_idx, dtype=np.int32)
        ptr = _native.ptr
        n_words = ctypes.c_int64()
        _native.check("tblup_mde_windows", self._lib.tblup_mde_windows(pop, len(q_idx), len(p_idx), slack, None, None,
                                                                       None, ctypes.byref(n_words)))
        if n_words.value > 1 << 26:
            return False
        words = np.empty(max(n_words.value, 1), dtype=np.uint32)
        key, pos, _ = self._rng_state()
        ws = work_stream(self.device)
        ws.wait_stream(torch.cuda.current_stream(ws.device))
        _native.check("tblup_mde_draws", self._lib.tblup_mde_draws(
            self._ctx, pop, L, len(q_idx), len(p_idx), slack, ptr(key), pos.value, ptr(words), n_words.value,
            ctypes.c_void_p(ws.cuda_stream)))
        mt, idx = _native.py_random_state()
        parent = np.empty(pop, dtype=np.int32)
        donors = np.empty((pop, 3), dtype=np.int32)
        fixed = np.empty(pop, dtype=np.int64)
        c_words = np.empty(pop, dtype=np.int64)
        overflow = ctypes.c_int32()
        _native.check("tblup_mde_resolve", self._lib.tblup_mde_resolve(
            pop, L, ptr(q_idx), len(q_idx), ptr(p_idx), len(p_idx), slack, ptr(words), n_words.value, ptr(mt),
            ptr(idx), ptr(parent), ptr(donors), ptr(fixed), ptr(c_words), ctypes.byref(overflow)))
        if overflow.value:
            return None
        _native.set_py_random_state(mt, idx)
        return parent, donors, fixed, c_words

    def step_device(self, strategy, parents, donors, fixed, F, cr, clip, clip_hi, defer=False, mde=None):
        """Same on a device tensor of parents (pop x L float64, on this device); returns the
        children as a device tensor.  Runs on torch's current stream.  defer: return
        (children, finish) without waiting for the step; finish() waits for the new MT state
        only (tblup_de_state_wait) and hands it to numpy -- call it before numpy's global RNG is
        used again.  strategy / F / cr: scalars, or one per individual (SaDE).  mde: (parent,
        c_words) of mde_draws -- the MDE_pBX step that continues those draws (F / cr per individual)."""
        import torch
        pop, L = parents.shape
        donors = np.ascontiguousarray(donors, dtype=np.int32)
        fixed = np.ascontiguousarray(fixed, dtype=np.int64)
        cur = torch.cuda.current_stream(parents.device)
        ws = work_stream(self.device)
        ws.wait_stream(cur)   # parents may come from work queued on the caller's stream
        with torch.cuda.stream(ws):
            children = torch.empty_like(parents)
        key, pos, hand_back = self._rng_state()
        ptr = _native.ptr

        def each(x, dtype):   # one value per individual
            return np.ascontiguousarray(np.broadcast_to(x, (pop,)), dtype=dtype)
        # every entry's arguments from the parents on: (..., donors, fixed) and (clip, ..., stream)
        rows = (ctypes.c_void_p(parents.data_ptr()), pop, L, parents.stride(0))
        tail = (1 if clip else 0, float(clip_hi), ptr(key), pos.value, ctypes.c_void_p(children.data_ptr()),
                children.stride(0), ctypes.c_void_p(ws.cuda_stream))
        if mde is not None:
            parent_i = np.ascontiguousarray(mde[0], dtype=np.int32)
            c_words = np.ascontiguousarray(mde[1], dtype=np.int64)
            F_i, cr_i = each(F, np.float64), each(cr, np.float64)
            _native.check("tblup_mde_step_device_async", self._lib.tblup_mde_step_device_async(
                self._ctx, ptr(F_i), ptr(cr_i), *rows, ptr(parent_i), ptr(donors), ptr(fixed), ptr(c_words), *tail))
        elif np.ndim(strategy) or np.ndim(F) or np.ndim(cr):
            strat_i, F_i, cr_i = each(strategy, np.int32), each(F, np.float64), each(cr, np.float64)
            _native.check("tblup_de_step_device_async_mix", self._lib.tblup_de_step_device_async_mix(
                self._ctx, ptr(strat_i), ptr(F_i), ptr(cr_i), *rows, ptr(donors), ptr(fixed), *tail))
        else:
            _native.check("tblup_de_step_device_async", self._lib.tblup_de_step_device_async(
                self._ctx, int(strategy), *rows, ptr(donors), ptr(fixed), float(F), float(cr), *tail))
        cur.wait_stream(ws)   # later caller work on the children is ordered behind the step

        def finish():
            _native.check("tblup_de_state_wait", self._lib.tblup_de_state_wait(self._ctx, ptr(key), ctypes.byref(pos)))
            hand_back()

        if defer:
            return children, finish
        finish()
        return children

    def gather_rows(self, out, ptrs):
        """out[i] = the device row at address ptrs[i] (this device), on torch's current stream."""
        import torch
        n, L = out.shape
        tab = np.array(ptrs, dtype=np.uint64)   # host array of n device addresses (one C conversion)
        _native.check("tblup_gather_rows", self._lib.tblup_gather_rows(
            self._ctx, ctypes.c_void_p(out.data_ptr()), n, L, out.stride(0), ctypes.c_void_p(tab.ctypes.data),
            ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)))

    def close(self):
        if self._ctx:
            self._lib.tblup_ctx_destroy(self._ctx)
            self._ctx = None
            GpuDEStep._instances.pop(self.device, None)


_F64 = np.dtype(np.float64)


def _child_dtypes(genomes, donors, strategy, mi, clip, parent_of=None):
    """Per-child dtype numpy gives the reference: np.where(mask, mutant, target) (+ np.clip);
    None when every child is float64 (the usual RandomKey case).  parent_of: child i's target is
    genome parent_of[i] (MDE_pBX), else genome i."""
    dts = [g.dtype if isinstance(g, np.ndarray) else np.asarray(g).dtype for g in genomes]
    f64 = _F64
    if all(dt is f64 or dt == f64 for dt in dts):
        return None
    out = []
    e = np.zeros(0, dtype=bool)
    for i, (x, y, z) in enumerate(donors):
        t, a, b, c = (np.zeros(0, dtype=dts[j]) for j in (i if parent_of is None else parent_of[i], x, y, z))
        st = strategy[i] if np.ndim(strategy) else strategy
        m = mi[i] if np.ndim(mi) else mi
        mutant = a + m * (b - c) if st == 0 else t + m * (a - t) + m * (b - c)
        r = np.where(e, mutant, t)
        out.append((np.clip(r, 0, 1) if clip else r).dtype)
    return out


_NO_GENOME = np.empty(0)

# diagnostics (tools/generation_bench.py): when a dict, evolve() adds its segment times (s)
PROFILE = None


def _mark(t0, name):
    import time
    t = time.perf_counter()
    if PROFILE is not None:
        PROFILE[name] = PROFILE.get(name, 0.0) + t - t0
    return t


def _assigns_genome(indv):
    """Whether set_internal_genome only stores the array (IndexIndividual's, individual.py:100-101,
    inherited by RandomKey / Nullable): then a child may be bound to its row before the row's
    transfer has landed.  CoevolutionIndividual's reads the last element (individual.py:194-208)."""
    f = getattr(type(indv), "set_internal_genome", None)
    return getattr(f, "__qualname__", "") == "IndexIndividual.set_internal_genome"


_DC_INDEX = {}


def _deepcopy_is_index(dc):
    """Whether `dc` is IndexIndividual.__deepcopy__ (the reference's, individual.py:110-118)."""
    hit = _DC_INDEX.get(dc)
    if hit is None:
        hit = _DC_INDEX[dc] = getattr(dc, "__qualname__", "") == "IndexIndividual.__deepcopy__"
    return hit


def _copy_individual(indv):
    """deepcopy(indv) as the reference's evolvers take it (evolver.py:130, 208), without
    copying the internal genome the caller replaces right after (set_internal_genome):
    the reference's IndexIndividual.__deepcopy__ (individual.py:110-118) deep-copies
    `_genome`, a 400 KB array per child at L = 50k."""
    g = getattr(indv, "_genome", None)
    if not isinstance(g, np.ndarray):
        return deepcopy(indv)
    # the class's own __deepcopy__ (individual.py:43-59, 110-118) called directly: copy.deepcopy's
    # dispatch and throwaway memo bookkeeping cost a third of the time for the same object
    dc = getattr(type(indv), "__deepcopy__", None)
    # IndexIndividual.__deepcopy__ (individual.py:110-118) only deep-copies the placeholder: None is
    # an atomic for copy.deepcopy (returned as is), where an empty array's deepcopy took ~half the
    # copy's time; other classes' __deepcopy__ may read the genome, so they get an empty array
    indv._genome = None if _deepcopy_is_index(dc) else _NO_GENOME
    try:
        return dc(indv, {}) if dc is not None else deepcopy(indv)
    finally:
        indv._genome = g


def _members(population):
    """The population's individuals and their internal genomes, one pass, and the common genome
    length (DE needs one: numpy broadcasting in evolver.py:132)."""
    inds = [population[i] for i in range(len(population))]
    genomes = [x.get_internal_genome() for x in inds]
    L = len(genomes[0]) if genomes else 0
    if any(len(g) != L for g in genomes):
        raise ValueError("DE needs internal genomes of one length (numpy broadcasting in evolver.py:132)")
    return inds, genomes, L


class Evolver(abc.ABC):
    """evolver.py:35-44."""

    @abc.abstractmethod
    def evolve(self, population):
        raise NotImplementedError()


class _GpuDEEvolver(Evolver):
    strategy = None
    device = None

    def __init__(self, dimensionality, crossover_rate, mutation_intensity, clip=True):
        self.dimensionality = dimensionality
        self.crossover_rate = crossover_rate
        self.mutation_intensity = mutation_intensity
        self.clip = clip

    def _donors(self, population, L):
        raise NotImplementedError()

    def _clip(self):
        return self.clip

    def evolve(self, population):
        import time
        t = time.perf_counter()
        mi = 5 if population.generation % 5 == 0 else self.mutation_intensity
        members = _members(population)
        donors, fixed = self._donors(population, members[2])
        return self._gpu_generation(population, t, donors, fixed, self.strategy, mi, self.crossover_rate,
                                    self._clip(), members)

    def _gpu_generation(self, population, t, donors, fixed, strategy, mi, cr, clip, members=None, mde=None):
        """The children of one generation (donors / fixed: the python-`random` draws already made;
        strategy, mi, cr: scalars or one per individual; members: _members(population) when the
        caller has it) through the GPU DE step.  mde: (parent, c_words) of GpuDEStep.mde_draws --
        child i is made from, and is a copy of, population[parent[i]] (MDE_pBX)."""
        import torch
        inds, genomes, L = members if members is not None else _members(population)
        n = len(inds)
        t = _mark(t, "ev_donors")
        step = GpuDEStep.get(self.device)
        store = DeviceKeyStore.get(step.device)
        with torch.cuda.device(step.device), torch.cuda.stream(work_stream(step.device)):
            parents = store.gather(inds, L, host_rows=lambda i: genomes[i],
                                   copy_rows=step.gather_rows)   # device-resident parents
            t = _mark(t, "ev_gather")
            children, rng_done = step.step_device(strategy, parents, donors, fixed, mi, cr, clip,
                                                  self.dimensionality - 1, defer=True, mde=mde)
            src = range(n) if mde is None else [int(j) for j in mde[0]]   # child i's base individual
            t = _mark(t, "ev_prepare_step")
            try:
                # the children's numpy dtypes (None: all float64), while the step runs
                dtypes = _child_dtypes(genomes, donors, strategy, mi, clip, None if mde is None else src)
                # the population's evaluator (tblup_amd) may start evaluating the children on the GPU
                # now, while their genomes cross to the host (BlupParallelEvaluator._speculate)
                evaluator = getattr(population, "evaluator", None)
                spec = getattr(evaluator, "_speculate", None)
                bases = inds if mde is None else [inds[j] for j in src]
                speculated = bool(spec is not None and dtypes is None and spec(bases, children, population.generation))
                t = _mark(t, "ev_speculate")
                # the copies to the host, issued behind the step: one page-locked block whose rows become
                # the genomes, a node-shared one, or chunks for an own array per child (HostRows)
                rows = HostRows(children, dtypes, n, L, shard_range(n, *world()))
            finally:
                rng_done()   # numpy's global state after the step's np.random.rand draws
        t = _mark(t, "ev_transfer_issue")
        # the candidates (new uids, the parent's other attributes) while the transfer runs
        next_pop = [_copy_individual(population[j]) for j in src]
        t = _mark(t, "ev_candidates")
        # whole-block rows: every child is bound to its row (a view: nothing reads the values),
        # recorded, and the older blocks compacted while the rows are still in flight; the
        # children are returned once their rows have landed (every rank's, for a shared block)
        early = rows.whole is not None and all(_assigns_genome(c) for c in next_pop)
        if not early:
            rows.landed()
        arrays = rows.arrays()
        t = _mark(t, "ev_arrays")
        self._bind(next_pop, arrays, inds, genomes, children, parents, store, speculated, evaluator, dtypes)
        t = _mark(t, "ev_bind_record")
        # older blocks the parents leave sparsely used, while the GPU still evaluates the children
        _BLOCKS.compact(inds, store)
        t = _mark(t, "ev_compact")
        if early:
            rows.landed()
            _mark(t, "ev_rows_landed")
        return next_pop

    @staticmethod
    def _bind(next_pop, arrays, inds, genomes, children, parents, store, speculated, evaluator, dtypes=None):
        for i in range(len(next_pop)):
            next_pop[i].set_internal_genome(arrays[i])
        if speculated:
            evaluator._spec_bind(next_pop)
        if dtypes is None:   # float64 internal genomes: the device rows are the children's exact values
            store.record(children, next_pop, arrays)
            store.record(parents, inds, genomes, adopt=True)
        store.prune([x.uid for x in inds] + [x.uid for x in next_pop])


class DERandOneEvolver(_GpuDEEvolver):
    """DE/rand/1 (evolver.py:86-157)."""

    strategy = _native.DE_STRATEGY["de_rand_1"]

    def _donors(self, population, L):
        n = len(population)
        drawn = _native_donors(self.strategy, n, L)
        return drawn if drawn is not None else _draw_donors(n, lambda i: _rand_one_draws(n, L, i))


class DECurrentToBestOneEvolver(_GpuDEEvolver):
    """DE/current-to-best/1 (evolver.py:160-244)."""

    strategy = _native.DE_STRATEGY["de_currenttobest_1"]

    def _clip(self):
        return True   # evolve() calls de_currenttobest_one without clip (default True)

    def _donors(self, population, L):
        n = len(population)
        best = _best_index(population)
        drawn = _native_donors(self.strategy, n, L, best)
        return drawn if drawn is not None else _draw_donors(n, lambda i: _current_to_best_draws(n, L, i, best))


# ---------------------------------------------------------------------------------------------
# Adaptive evolvers (evolver.py:297-687)
# ---------------------------------------------------------------------------------------------
class AdaptiveEvolver(Evolver):
    """Bookkeeping of the F / CR values whose candidates entered the population (evolver.py:297-404),
    with the reference's parameter report (a `_params` CSV beside the monitor's results file)."""

    def __init__(self):
        self.successful_fs = []
        self.successful_crs = []
        self.previous_pop_uids = None
        self.crs = []
        self.fs = []

    def should_report(self):
        return True

    def report(self, population):
        stem, ext = os.path.splitext(os.path.basename(population.monitor.results_file))
        path = os.path.join(os.path.dirname(population.monitor.results_file), stem + "_params" + ext)
        if population.generation == 1:
            with open(path, "w") as f:
                csv.writer(f).writerow(self.get_header())
        with open(path, "a") as f:
            csv.writer(f).writerow(self.get_params_row())

    @abc.abstractmethod
    def get_header(self):
        raise NotImplementedError()

    @abc.abstractmethod
    def get_params_row(self):
        raise NotImplementedError()

    def evolve(self, population):
        """The per-generation adaptation step subclasses run first (evolver.py:336-356)."""
        if self.should_report():
            self.report(population)
        if self.previous_pop_uids is None:
            self.previous_pop_uids = [x.uid for x in population]
        self.count_outcomes(population)
        if self.should_regenerate_crs(population):
            self.regenerate_crs(population)
        if self.should_regenerate_fs(population):
            self.regenerate_fs(population)
        self.previous_pop_uids = [x.uid for x in population]

    def count_outcomes(self, population):
        """A changed uid at position i: the candidate made with crs[i] / fs[i] entered the population."""
        for i, (old, cur) in enumerate(zip(self.previous_pop_uids, population)):
            if old != cur.uid:
                if i < len(self.crs):
                    self.successful_crs.append(self.crs[i])
                if i < len(self.fs):
                    self.successful_fs.append(self.fs[i])

    @abc.abstractmethod
    def should_regenerate_crs(self, population):
        raise NotImplementedError()

    @abc.abstractmethod
    def generate_cr(self):
        raise NotImplementedError()

    def regenerate_crs(self, population):
        self.crs = [self.generate_cr() for _ in range(len(population))]

    @abc.abstractmethod
    def should_regenerate_fs(self, population):
        raise NotImplementedError()

    @abc.abstractmethod
    def generate_f(self):
        raise NotImplementedError()

    def regenerate_fs(self, population):
        self.fs = [self.generate_f() for _ in range(len(population))]


class SaDE(AdaptiveEvolver, _GpuDEEvolver):
    """Self-adaptive DE (Qin & Suganthan 2005; evolver.py:407-547), its generation on the GPU.

    Per generation: cr_m re-estimated every 25 generations, the crossover rates redrawn every 5
    (N(cr_m, 0.1) clipped to [0, 1]), one F ~ N(0.5, 0.3) clipped to [0, 2], and per individual
    DE/rand/1 with probability p, else DE/current-to-best/1, p learnt from the strategies' success
    counts after a 50-generation learning period.  The host draws what the reference draws, in its
    order (numpy's normal() calls, then per individual random.random(), the donors and the forced
    crossover position); the GPU step computes every child with its own strategy and rate."""

    f_m = 0.5
    f_std = 0.3
    cr_std = 0.1
    recalculate_mean_interval = 25
    regenerate_crs_interval = 5
    initial_learning_period = 50

    def __init__(self, dimensionality, clip=True):
        AdaptiveEvolver.__init__(self)
        self.dimensionality = dimensionality
        self.clip = clip
        self.cr_m = 0.5
        self.p = 0.5
        self.strategy_one_indices = set()
        self.ns_1, self.ns_2, self.nf_1, self.nf_2 = 0, 0, 0, 0

    def get_header(self):
        return ["cr_m", "p"]

    def get_params_row(self):
        return [self.cr_m, self.p]

    def should_regenerate_crs(self, population):
        return len(self.crs) == 0 or population.generation % self.regenerate_crs_interval == 0

    def should_recalculate_cr_m(self, generation):
        return generation != 0 and generation % self.recalculate_mean_interval == 0

    def recalculate_cr_m(self):
        if self.successful_crs:
            self.cr_m = np.mean(self.successful_crs)

    def generate_f(self):
        return np.clip(np.random.normal(self.f_m, self.f_std), 0, 2)

    def generate_cr(self):
        return np.clip(np.random.normal(self.cr_m, self.cr_std), 0, 1)

    def should_regenerate_fs(self, population):
        return False

    def recalculate_p(self, population):
        if population.generation >= self.initial_learning_period and (self.ns_1 or self.ns_2):
            num = self.ns_1 * (self.ns_2 + self.nf_2)
            self.p = num / (self.ns_2 * (self.ns_1 + self.nf_1) + num)

    def count_outcomes(self, population):
        AdaptiveEvolver.count_outcomes(self, population)
        if population.generation == self.initial_learning_period:
            # learning period over: counters restart from one success each (evolver.py:479-484)
            self.ns_1, self.ns_2, self.nf_1, self.nf_2 = 1, 1, 0, 0
        for i, (old, cur) in enumerate(zip(self.previous_pop_uids, population)):
            one = i in self.strategy_one_indices
            if old == cur.uid:
                if one:
                    self.nf_1 += 1
                else:
                    self.nf_2 += 1
            elif one:
                self.ns_1 += 1
            else:
                self.ns_2 += 1

    def evolve(self, population):
        import time
        t = time.perf_counter()
        if self.should_recalculate_cr_m(population.generation):
            self.recalculate_cr_m()
        AdaptiveEvolver.evolve(self, population)
        self.recalculate_p(population)
        f = self.generate_f()
        n = len(population)
        members = _members(population)
        L = members[2]
        best_index = _best_index(population)
        strategies = np.empty(n, dtype=np.int32)
        donors = np.empty((n, 3), dtype=np.int32)
        fixed = np.empty(n, dtype=np.int64)
        self.strategy_one_indices = set()
        for i in range(n):
            if random.random() < self.p:   # DE/rand/1 (evolver.py:118-121)
                self.strategy_one_indices.add(i)
                strategies[i] = 0
                donors[i], fixed[i] = _rand_one_draws(n, L, i)
            else:                          # DE/current-to-best/1 (evolver.py:199-203)
                strategies[i] = 1
                donors[i], fixed[i] = _current_to_best_draws(n, L, i, best_index)
        crs = np.array([float(c) for c in self.crs[:n]], dtype=np.float64)
        return self._gpu_generation(population, t, donors, fixed, strategies, f, crs, self.clip, members)


class MDE_pBX(AdaptiveEvolver, _GpuDEEvolver):
    """MDE_pBX (Islam et al. 2012; evolver.py:550-687), its generation on the host or on the GPU.

    Each individual draws its group best and its parent with np.random.choice -- rejection-sampled
    integers, a data-dependent number of MT19937 words -- between the individuals' np.random.rand(L)
    calls, so individual i's uniforms start 2Li + C_i words into the generation's numpy stream, C_i
    the words the choices of individuals 0..i took.  The host loop (_host_current_to_best) is the
    reference's: the same draws in the same order, DE/current-to-best/1 with the chosen best and
    parent, binary crossover, optional clip.  The device generation (GpuDEStep.mde_draws, then
    _gpu_generation) jumps to every individual's fixed offset 2Li on the GPU, expands the few words
    past it that the choices can read, resolves the choices, C_i and python's draws sequentially in
    native host code, and runs the step with each individual's uniforms at its own offset; the
    children then live in the DeviceKeyStore like the other strategies'.  Same bits either way
    (tests/test_gpu_mde.py).

    Which one runs: `device_step` (True / False; None: the environment's TBLUP_MDE_PBX = "device" /
    "host", else DEVICE_DEFAULT).  The host loop always runs when no HIP device is visible, for
    pop < 4 (the reference's assertion is raised there), and for a generation whose rejection run
    leaves its window (MDE_pBX.fallbacks counts those; TBLUP_MDE_SLACK >= 0 sets the window slack in
    words, for tests), and for a population whose draw windows would exceed 2^26 words
    (MDE_pBX.oversize counts those generations: every one of such a run).  The device generation is the default: 5.9 against 98 ms per generation at
    pop 256, 22 against 401 ms at pop 1024 (L = 50 000, tools/de_bench.py mde_pbx; PERFLOG.md)."""

    f_scale = 0.1
    cr_std = 0.1
    group_q = 0.15
    DEVICE_DEFAULT = True
    device_step = None
    fallbacks = 0   # generations that fell back to the host loop on a window overflow
    oversize = 0    # generations kept on the host loop because their draw windows are too large

    def __init__(self, dimensionality, generations, clip=True):
        AdaptiveEvolver.__init__(self)
        self.dimensionality = dimensionality
        self.clip = clip
        self.g_max = generations
        self.cr_m = 0.6
        self.f_m = 0.5
        self.p = None

    def get_header(self):
        return ["cr_m", "f_m"]

    def get_params_row(self):
        return [self.cr_m, self.f_m]

    def should_regenerate_fs(self, population):
        return True

    def should_regenerate_crs(self, population):
        return True

    def generate_cr(self):
        """N(cr_m, 0.1), redrawn until in [0, 1]."""
        while True:
            cr = np.random.normal(self.cr_m, self.cr_std)
            if 0 <= cr <= 1:
                return cr

    def generate_f(self):
        """Cauchy(f_m, 0.1) (scipy.stats.cauchy on numpy's global RandomState), redrawn until in [0, 1]."""
        from scipy.stats import cauchy
        while True:
            f = cauchy.rvs(loc=self.f_m, scale=self.f_scale)
            if 0 <= f <= 1:
                return f

    @staticmethod
    def mean_pow(vals, n=1.5):
        """The power mean of formula (10), simplified for positive values as the reference does."""
        assert n > 0, "n must be a positive number."
        return sum(vals) / pow(1 / len(vals), -n)

    @staticmethod
    def get_weight_factor(p, q):
        return p + q * random.random()

    def recalculate_cr_m(self):
        if self.successful_crs:
            w = self.get_weight_factor(0.9, 0.1)
            self.cr_m = w * self.cr_m + (1 - w) * self.mean_pow(self.successful_crs)
            self.successful_crs = []

    def recalculate_f_m(self):
        if self.successful_fs:
            w = self.get_weight_factor(0.8, 0.2)
            self.f_m = w * self.f_m + (1 - w) * self.mean_pow(self.successful_fs)
            self.successful_fs = []

    def recalculate_p(self, population):
        self.p = ceil((len(population) / 2) * (1 - (population.generation / self.g_max)))

    _HAS_DEVICE = None

    def _on_device(self, n):
        mode = self.device_step
        if mode is None:
            env = os.environ.get("TBLUP_MDE_PBX", "")
            mode = True if env == "device" else False if env == "host" else self.DEVICE_DEFAULT
        if not mode or n < 4 or n > 65535:
            return False
        if MDE_pBX._HAS_DEVICE is None:
            try:
                MDE_pBX._HAS_DEVICE = _native.device_count() >= 1
            except (ImportError, _native.TblupError):
                MDE_pBX._HAS_DEVICE = False
        return MDE_pBX._HAS_DEVICE

    def _device_generation(self, population, t, q_best, p_best):
        """The generation through the GPU step; None (no RNG state touched) to run the host loop."""
        members = _members(population)
        n, L = len(members[0]), members[2]
        if L < 1 or L > 1 << 31:
            return None
        first = {}
        for j, x in enumerate(population.population):   # population.index(best), evolver.py:194
            first.setdefault(id(x), j)
        q_idx = [first[id(population[int(q)])] for q in q_best]
        slack = int(os.environ.get("TBLUP_MDE_SLACK", "-1"))
        drawn = GpuDEStep.get(self.device).mde_draws(n, L, q_idx, p_best, slack)
        if drawn is None:
            MDE_pBX.fallbacks += 1
            return None
        if drawn is False:
            MDE_pBX.oversize += 1
            return None
        parent, donors, fixed, c_words = drawn
        fs = np.array([float(f) for f in self.fs[:n]], dtype=np.float64)
        crs = np.array([float(c) for c in self.crs[:n]], dtype=np.float64)
        return self._gpu_generation(population, t, donors, fixed, _native.DE_STRATEGY["de_currenttobest_1"], fs, crs,
                                    self.clip, members, mde=(parent, c_words))

    def evolve(self, population):
        import time
        t = time.perf_counter()
        self.recalculate_cr_m()
        self.recalculate_f_m()
        self.recalculate_p(population)
        AdaptiveEvolver.evolve(self, population)
        order = np.argsort([x.fitness for x in population])
        q_best = order[-int(len(population) * self.group_q):]
        p_best = order[-self.p:]
        n = len(population)
        if self._on_device(n):
            out = self._device_generation(population, t, q_best, p_best)
            if out is not None:
                return out
        out = []
        for i in range(n):
            best = population[np.random.choice(q_best, 1).item()]
            parent_idx = np.random.choice(p_best, 1).item()
            out.append(_host_current_to_best(population, self.fs[i], self.crs[i], self.dimensionality, parent_idx,
                                             best, self.clip))
        return out


def _host_current_to_best(population, mi, cr, dimensionality, parent_idx, best, clip):
    """DECurrentToBestOneEvolver.de_currenttobest_one with binary crossover (evolver.py:63-82,
    179-221) on the host: the reference's draws (_current_to_best_draws, one np.random.rand(L)) and
    its float arithmetic order."""
    L = len(population[parent_idx].get_internal_genome())
    (_, a, b), fixed = _current_to_best_draws(len(population), L, parent_idx, population.population.index(best))
    ga, gb = population[a].get_internal_genome(), population[b].get_internal_genome()
    child = deepcopy(population[parent_idx])
    x = child.get_internal_genome()
    mutant = x + mi * (best.get_internal_genome() - x) + mi * (ga - gb)
    take = np.random.rand(L) < cr
    take[fixed] = True
    child.set_internal_genome(np.where(take, mutant, x))
    if clip:
        child.set_internal_genome(np.clip(child.get_internal_genome(), 0, dimensionality - 1))
    return child
