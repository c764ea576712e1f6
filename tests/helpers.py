"""Test-side stand-ins for the reference's individuals and an oracle-backed engine.

The oracle engine is TEST INFRASTRUCTURE: it lets the CPU suite exercise the
evaluator's host logic (splits, archive, SNP removal, CV folds, sharding)
without a GPU.  The product evaluator never constructs it.
"""
import itertools

import numpy as np

from oracle import blup_oracle as O

_uid = itertools.count(10_000)


class KeyIndividual:
    """RandomKeyIndividual stand-in (tblup/individual.py:132-167)."""

    def __init__(self, keys, length):
        self.uid = next(_uid)
        self._genome = np.asarray(keys)
        self.length = length
        self.fitness = float("-inf")

    @property
    def genome(self):
        return O.decode_randkeys(self._genome, self.length)

    def __len__(self):
        return int(self.length)

    def set_fitness(self, f):
        self.fitness = f


    def get_internal_genome(self):
        return self._genome

    def set_internal_genome(self, genome):
        self._genome = genome

    def __deepcopy__(self, memo):
        """individual.py:43-59 / 110-118: same class and attributes, a new uid."""
        cp = self.__class__.__new__(self.__class__)
        cp.__dict__.update(self.__dict__)
        cp.uid = next(_uid)
        return cp


class CoevoIndividual(KeyIndividual):
    """CoevolutionIndividual stand-in (tblup/individual.py:170-222): the length rides along
    as the last element of the internal genome."""

    def __init__(self, keys, length, dimensionality):
        super().__init__(keys, length)
        self.dimensionality = dimensionality

    def get_internal_genome(self):
        return np.append(self._genome, self.length)

    def set_internal_genome(self, genome):
        if len(genome) == self.dimensionality + 1:
            if genome[-1] < 1:
                self.length = 1
            elif genome[-1] > self.dimensionality:
                self.length = self.dimensionality
            else:
                self.length = genome[-1]
            self._genome = np.delete(genome, -1)
        elif len(genome) == self.dimensionality:
            self._genome = genome
        else:
            raise RuntimeError("Genome of invalid length, must be dimensionality d or d + 1.")


class Pop:
    """The slice of tblup.Population the evolvers read (.population, .generation, [], len)."""

    def __init__(self, individuals, generation):
        self.population = individuals
        self.generation = generation

    def __getitem__(self, i):
        return self.population[i]

    def __len__(self):
        return len(self.population)


class RandomKeyIndividual(KeyIndividual):
    """Same stand-in under the reference's class name: the evaluator batch-decodes
    RandomKeyIndividual / CoevolutionIndividual genomes on the GPU (by class name)."""


class IdxIndividual(KeyIndividual):
    """IndexIndividual stand-in (tblup/individual.py:73-130)."""

    @property
    def genome(self):
        return O.decode_index(self._genome)

    def __len__(self):
        return len(self._genome)


class OracleEngine:
    """Same evaluate() contract as tblup_amd.engine.GpuBlupEngine, computed by the oracle."""

    def __init__(self, data, labels):
        self.data = np.asarray(data, dtype=np.float64)
        self.labels = np.asarray(labels, dtype=np.float64)
        self.calls = 0

    def evaluate(self, genomes, train, valid, h2, branch="auto", return_ebv=False):
        self.calls += 1
        out = []
        for g in genomes:
            if branch == "auto":
                out.append(O.blup(g, train, valid, self.data, self.labels, h2))
            elif branch == "gblup":
                out.append(O.gblup(g, train, valid, self.data, self.labels, h2))
            else:
                out.append(O.snp_blup(g, train, valid, self.data, self.labels, h2))
        return np.array(out, dtype=np.float64)

    def evaluate_folds(self, genomes, splits, h2, branch="auto"):
        """GpuBlupEngine.evaluate_folds: (n_splits, B), row f = evaluate(genomes, *splits[f])."""
        return np.array([self.evaluate(genomes, t, v, h2, branch) for t, v in splits]).reshape(len(splits), -1)

    def close(self):
        pass


def shard_population(pop, n_snps, k, seed=11):
    """A population of `pop` selected-index sets where individual i comes from its own seed:
    the same individuals in every process, whatever the sharding (tests/test_gpu_shards.py)."""
    return [np.random.default_rng((seed, i)).choice(n_snps, k, replace=False) for i in range(pop)]


# ----------------------------------------------------------------------------
# Edge-parity case builders, shared by tests/test_gpu_edges.py (the HIP pipeline against the
# oracle) and tests/test_edge_cases_cpu.py (the oracle against a wider solve on the same
# inputs).  Every case is generated from a seed; the builders are cached, so callers must not
# write into what they return.
# ----------------------------------------------------------------------------
import functools  # noqa: E402

EDGE_H2 = 0.4
EDGE_A_SIZES = [(1, 2), (2, 3), (3, 2), (15, 17), (127, 2), (128, 128), (129, 127), (130, 129), (256, 7), (257, 6)]
EDGE_A_KS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 264, 530, 600]
EDGE_A_FORCED_SPLITS = [(3, 2), (129, 127), (257, 6)]
EDGE_A_FORCED_KS = [1, 17, 129, 264, 600]
EDGE_B_NV = [2, 3, 1023, 1024, 1025, 2049]
EDGE_C_KS = [200, 400, 701]


def _case(group, name, geno, pheno, T, V, idx, branch="auto"):
    return dict(group=group, name=name, geno=geno, pheno=pheno, T=T, V=V, idx=idx, branch=branch)


def edge_oracle(case):
    """The oracle's (fitness, EBV_V) of one evaluator case: the reference's own branch functions."""
    fn = {"auto": O.blup, "gblup": O.gblup, "snp": O.snp_blup}[case["branch"]]
    return fn(case["idx"], case["T"], case["V"], case["geno"], case["pheno"], EDGE_H2, return_ebv=True)


@functools.lru_cache(maxsize=None)
def edge_a():
    """263 x 530 panel: columns 0 / 1 / 2 all 0 / 2 / 1, column 3 polymorphic only on the six
    animals outside every train set; ten unsorted splits cut from one permutation; genomes of
    every k around the 64-SNP block and the 128-row tile, k > n (gblup), every column, with
    replacement, a degenerate one (columns 0-2) and one written with negative indices."""
    rng = np.random.default_rng(2601)
    n, P = 263, 530
    geno = O.synth_geno(rng, n, P)
    perm = rng.permutation(n)
    geno[:, 0], geno[:, 1], geno[:, 2], geno[:, 3] = 0, 2, 1, 0
    geno[perm[257:], 3] = [1, 2, 0, 1, 2, 1]
    pheno = rng.standard_normal(n)
    splits = {s: (perm[:s[0]].copy(), perm[s[0]:s[0] + s[1]].copy()) for s in EDGE_A_SIZES}
    genomes = {}
    for k in EDGE_A_KS:
        if k == 530:
            g = rng.permutation(P)
        elif k == 600:
            g = rng.integers(0, P, k)
        else:
            g = rng.choice(np.arange(4, P), k, replace=False)
            if k in (17, 129):
                g[k // 2] = 3
        genomes["k%d" % k] = g.astype(np.int64)
    genomes["degenerate"] = np.array([2, 0, 1], dtype=np.int64)
    neg = rng.choice(np.arange(4, P), 40, replace=False).astype(np.int64)
    neg[::2] -= P
    genomes["negative"] = neg
    return dict(n=n, P=P, geno=geno, pheno=pheno, splits=splits, genomes=genomes)


def edge_a_is_snp(a, name):
    return len(a["genomes"][name]) <= a["n"]


def edge_a_cases():
    a = edge_a()
    out = []
    for s, (T, V) in a["splits"].items():
        for name, g in a["genomes"].items():
            out.append(_case("A", "A-%d-%d-%s" % (s + (name,)), a["geno"], a["pheno"], T, V, g))
    for s in EDGE_A_FORCED_SPLITS:
        T, V = a["splits"][s]
        for k in EDGE_A_FORCED_KS:
            for br in ("gblup", "snp"):
                out.append(_case("A", "A-%d-%d-k%d-%s" % (s + (k, br)), a["geno"], a["pheno"], T, V,
                                 a["genomes"]["k%d" % k], br))
    return out


@functools.lru_cache(maxsize=None)
def edge_b():
    """2200 x 300 panel, 64 train animals, nested validation sets of the sizes around
    pearson_abs' 1024-thread stride; phenotypes standard normal, constant on V, two-valued on V."""
    rng = np.random.default_rng(2602)
    n, P, nT = 2200, 300, 64
    geno = O.synth_geno(rng, n, P)
    perm = rng.permutation(n)
    T, vall = perm[:nT].copy(), perm[nT:nT + max(EDGE_B_NV)].copy()
    y = rng.standard_normal(n)
    y_const = y.copy()
    y_const[vall] = 0.75
    two = rng.integers(0, 2, len(vall))
    two[:2] = [0, 1]
    y_two = y.copy()
    y_two[vall] = np.where(two == 0, -1.25, 0.5)
    genomes = {k: rng.choice(P, k, replace=False).astype(np.int64) for k in (40, 100)}
    return dict(geno=geno, T=T, V={nv: vall[:nv] for nv in EDGE_B_NV}, genomes=genomes,
                pheno={"normal": y, "const": y_const, "two": y_two})


def edge_b_cases():
    b = edge_b()
    return [_case("B", "B-%s-nv%d-k%d" % (pn, nv, k), b["geno"], y, b["T"], V, g)
            for pn, y in b["pheno"].items() for nv, V in b["V"].items() for k, g in b["genomes"].items()]


@functools.lru_cache(maxsize=None)
def edge_c():
    """700 x 3000 panel, n_T = 300, n_V = 90, four phenotype columns; five genomes for each k:
    200 (SNP form, 2 tile columns), 400 (kernel form, 3 tile columns), 701 (k > n: gblup)."""
    rng = np.random.default_rng(2603)
    n, P = 700, 3000
    geno = O.synth_geno(rng, n, P)
    perm = rng.permutation(n)
    Y = rng.standard_normal((n, 4))
    Y[:, 2] += 0.5 * Y[:, 0]
    Y[:, 3] = 3.0 + 0.1 * Y[:, 3]
    genomes = {k: [rng.choice(P, k, replace=False).astype(np.int64) for _ in range(5)] for k in EDGE_C_KS}
    return dict(geno=geno, Y=Y, T=perm[:300].copy(), V=perm[300:390].copy(), genomes=genomes)


def edge_c_cases():
    c = edge_c()
    return [_case("C", "C-k%d-%d-trait%d" % (k, i, tr), c["geno"], np.ascontiguousarray(c["Y"][:, tr]), c["T"],
                  c["V"], g) for k, gs in c["genomes"].items() for i, g in enumerate(gs) for tr in range(4)]


def edge_d_geno(rng, n, P):
    """binomial(2, q) with q ~ U(0.9, 0.995) and columns 0-7 all 2: raw counts reach 4 per row."""
    q = rng.uniform(0.9, 0.995, size=P)
    geno = rng.binomial(2, q, size=(n, P)).astype(np.int8)
    geno[:, :8] = 2
    return geno


def _with_all2(rng, P, k, dup=0):
    """k columns: the eight all-2 columns, `dup` of them again, the rest distinct others."""
    g = np.concatenate([np.arange(8), np.arange(dup), rng.choice(np.arange(8, P), k - 8 - dup, replace=False)])
    return rng.permutation(g).astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_d1():
    """SNP form on both sides of the int16 count store: n_T = 8191 (counts reach 32764) and 8192."""
    rng = np.random.default_rng(2604)
    n, P = 8200, 320
    geno = edge_d_geno(rng, n, P)
    perm = rng.permutation(n)
    pheno = rng.standard_normal(n)
    splits = {nT: (perm[:nT].copy(), perm[nT:].copy()) for nT in (8191, 8192)}
    genomes = [_with_all2(rng, P, 260, dup=2) for _ in range(3)]
    return dict(geno=geno, pheno=pheno, splits=splits, genomes=genomes)


def edge_d1_cases():
    d = edge_d1()
    return [_case("D1", "D1-nT%d-%d" % (nT, i), d["geno"], d["pheno"], T, V, g, "snp")
            for nT, (T, V) in d["splits"].items() for i, g in enumerate(d["genomes"])]


@functools.lru_cache(maxsize=None)
def edge_d2():
    """Kernel form on both sides of 64 * cblk = 8191: k = 8128 (int16 counts), 8129 and 8192."""
    rng = np.random.default_rng(2605)
    n, P = 300, 8200
    geno = edge_d_geno(rng, n, P)
    perm = rng.permutation(n)
    pheno = rng.standard_normal(n)
    genomes = {k: _with_all2(rng, P, k) for k in (8128, 8129, 8192)}
    return dict(geno=geno, pheno=pheno, T=perm[:257].copy(), V=perm[257:].copy(), genomes=genomes)


def edge_d2_cases():
    d = edge_d2()
    return [_case("D2", "D2-k%d-%s" % (k, br), d["geno"], d["pheno"], d["T"], d["V"], g, br)
            for k, g in d["genomes"].items() for br in ("auto", "snp")]


@functools.lru_cache(maxsize=None)
def edge_d3():
    """Five equal folds of 10235 animals: n_T = 8188, n_V = 2047 (shared fold counts, int16)."""
    from tblup_amd.evaluator import InterGCVBlupParallelEvaluator
    rng = np.random.default_rng(2606)
    n, P = 10240, 320
    geno = edge_d_geno(rng, n, P)
    perm = rng.permutation(n)
    pheno = rng.standard_normal(n)
    folds = [(np.asarray(t), np.asarray(v)) for t, v in
             InterGCVBlupParallelEvaluator.make_fold_indices(perm[:10235], 5)]
    genomes = [_with_all2(rng, P, 200, dup=2) for _ in range(3)]
    return dict(geno=geno, pheno=pheno, folds=folds, genomes=genomes)


@functools.lru_cache(maxsize=None)
def edge_e():
    """SNP-form systems of ns = 4096 (k = 4096) and ns = 4224 (k = 4097) rows, two genomes each."""
    rng = np.random.default_rng(2607)
    n, P = 4400, 6000
    geno = O.synth_geno(rng, n, P)
    perm = rng.permutation(n)
    pheno = rng.standard_normal(n)
    genomes = {k: [rng.choice(P, k, replace=False).astype(np.int64) for _ in range(2)] for k in (4096, 4097)}
    return dict(geno=geno, pheno=pheno, T=perm[:4200].copy(), V=perm[4200:].copy(), genomes=genomes)


def edge_e_cases():
    e = edge_e()
    return [_case("E", "E-k%d-%d" % (k, i), e["geno"], e["pheno"], e["T"], e["V"], g)
            for k, gs in e["genomes"].items() for i, g in enumerate(gs)]


# ---- decode rows (group G) --------------------------------------------------------------
EDGE_G_D = [1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 32769]
NEG_NAN = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]   # x86's default NaN
POS_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def edge_g_ks(d):
    return sorted({k for k in (1, d // 2, d - 1, min(d, 8192)) if 1 <= k <= min(d, 8192)})


def edge_g_rows(d, seed=2608):
    """[(kind, keys, ks)] for one row length: the key rows of the issue's list, each with the k
    values it is decoded at."""
    rng = np.random.default_rng((seed, d))
    ks = edge_g_ks(d)
    rows = [("continuous", rng.uniform(-1, 1, d), ks),
            ("rounded", np.round(rng.uniform(size=d), 2), ks),
            ("equal", np.full(d, 0.5), ks),
            ("ascending", np.arange(d, dtype=np.float64) - d / 3, ks),
            ("descending", -np.arange(d, dtype=np.float64) + d / 3, ks)]
    # signed zeros: ~30 % each of +0.0 and -0.0, fewer than 8192 positive keys, negative keys for
    # the rest; k ends inside the zero tie
    n_pz, n_nz = (3 * d + 5) // 10, (3 * d) // 10
    n_pos = min(d - n_pz - n_nz, 4000)
    z = np.concatenate([np.zeros(n_pz), -np.zeros(n_nz), rng.uniform(0.1, 1, n_pos),
                        -rng.uniform(0.1, 1, d - n_pz - n_nz - n_pos)])
    z = rng.permutation(z)
    kz = min(max(n_pos + (n_pz + n_nz) // 2, 1), d, 8192)
    rows.append(("zeros", z, sorted(set(ks + [kz]))))
    inf = rng.uniform(-1, 1, d)
    inf[rng.permutation(d)[:max(1, d // 10)]] = np.inf
    inf[rng.permutation(d)[:max(1, d // 10)]] = -np.inf
    rows.append(("inf", inf, ks))
    nan = rng.uniform(-1, 1, d)
    where = rng.permutation(d)[:max(2, d // 20)] if d >= 2 else np.array([0])
    nan[where[::2]] = NEG_NAN
    nan[where[1::2]] = POS_NAN
    if d >= 8:
        nan[np.flatnonzero(~np.isnan(nan))[:2]] = [np.inf, -np.inf]
    rows.append(("nan", nan, ks))
    return rows


def decode_sample_candidates(keys, k):
    """Host model of k_decode_topk's fast path for a row of positive finite keys: the number of
    keys at or above the threshold bucket its strided sample picks (the fast path needs
    k <= candidates <= 8192)."""
    d = len(keys)
    u = keys.view(np.uint64) | np.uint64(1 << 63)
    s = (d + 4095) // 4096
    ns = 8 * ((d + 8 * s - 1) // (8 * s))
    j = np.arange(ns)
    i = (j >> 3) * (8 * s) + (j & 7)
    samp = np.where(i < d, u[np.minimum(i, d - 1)], np.uint64(0))
    r = min((5 * k) // (4 * s) + 8, ns)
    tau = np.sort(samp)[-r] >> np.uint64(40)
    return int(np.sum((u >> np.uint64(40)) >= tau))


@functools.lru_cache(maxsize=None)
def edge_g_fallback_rows():
    """Two rows of d = 50 000 (sampling stride 13: runs of 8 keys every 104) that the sampled
    threshold misjudges: [(name, keys, k)]."""
    rng = np.random.default_rng(2609)
    d = 50_000
    i = np.arange(d)
    sampled = (i % 104) < 8
    over = rng.uniform(1e-4, 2e-4, d)
    over[sampled] = rng.uniform(1e-6, 2e-6, int(sampled.sum()))
    over[rng.permutation(np.flatnonzero(~sampled))[:9000]] = rng.uniform(1, 2, 9000)
    few = rng.uniform(0, 1, d)
    few[sampled] = rng.uniform(10, 11, int(sampled.sum()))
    return [("overflow", over, 1000), ("too_few", few, 8192)]
