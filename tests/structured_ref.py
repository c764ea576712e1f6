"""A structured genotype panel -- linkage disequilibrium, full sibs, clones, rare alleles, repeated columns --
with heritabilities up to 1, its longdouble truths and the tolerance that scales with the condition number
(TEST INFRASTRUCTURE ONLY).  Shared by tests/test_structured_host.py (CPU) and tests/test_gpu_structured.py
(GPU).  Every other accuracy test of the suite runs on oracle.synth_geno's independent binomial SNPs at
h2 = 0.4, where the solved systems have a condition number of about 20.

Panel: 301 animals (odd: the SNP-major rows are unaligned) x 640 SNPs.
  LD        40 blocks of 16 consecutive SNPs; a haplotype is one of 5 block patterns with 2 % of its alleles
            flipped; along a block a SNP's pattern column repeats its neighbour's (one bit changed half the time)
            three times out of four
  families  29 full-sib families of 10: a child takes, block by block, one haplotype of each parent (the parents
            are not in the panel) and 0.5 % new flips; 11 unrelated animals; two breeds (families alternate), the
            second with the block patterns' frequencies reversed
  clones    identical rows: a pair at train rows 4 and 5 (inside one 16-row pivot block), a pair at train rows
            127 and 128 (across the 128-row tile boundary) and a triple at rows 60, 140 and 199
  rare      20 columns that are 1 in a single animal and 0 elsewhere, each with its own carrier
  columns   one column repeated exactly (DUP) and one complemented, 2 - x (COMP)
  Y         (a) standard normal, (b) the clone contrast e_i - e_j of the pair at train rows 4 and 5 (the smallest
            eigenvector of every kernel-form system), (c) a simulated breeding value plus noise, (d) (a) + 1e6
            (the gblup branch fits no mean: the offset goes through the solve), and (ab) = (a) + (b)

Splits (n_T, n_V): (200, 60) -- two tiles, unaligned -- and (257, 40), three tiles, whose first 200 train rows are the
first split's; every clone and every carrier is a train row of both; "cf" is (200, 60) without the later members
of the clone groups (n_T = 196).  Genomes: snp160 (SNP form: nine whole LD blocks and half of two more, DUP's two
columns at positions 4 and 5, COMP's two at 127 and 128, the 20 rare columns), snp158 (snp160 without one column
of each pair), dual260 (n_T < k <= n), g400 (k > n: gblup) and g130 (forced gblup at k <= n).

kappa is the 2-norm condition number (float64 eigvalsh) of the system that is solved: W_T^T W_T + lambda d I_k in the
SNP form, K_TT + lambda I in the kernel form.  One rule bounds every quantity:

    bar = max(TOL, 16 kappa 2^-53)         the GPU tests
    host_bar = max(TOL / 8, 2 kappa 2^-53) the float64 restatements against the longdouble truth

TOL the flat tolerance of the quantity's existing GPU test (1e-9; 1e-10 for the factor), the error taken relative
to the largest |truth| of the output vector, absolute for reliabilities and for the fitness and relative to
max(1, |truth|) for log-likelihood terms.  The absolute fitness departs from the issue, which makes only reliabilities
absolute: like them the fitness lives in [0, 1], FIT_ATOL of the existing tests is absolute, and a correlation can
be as near zero as it likes -- on (257, 40) snp160 gblup h2 = 0.9999 (c) the truth is 0.0057 and the oracle's own
1.1e-12 is 1.9e-10 of it, over the host bar (tests/test_structured_host.py keeps that figure).  kappa u is the forward-error scale of a backward-stable Cholesky; the
GPU path gets 16 times that scale, 8 times what LAPACK has to meet here.

What is not compared.  Column (b) alone: rows i and j of every K are equal, so alpha = (e_i - e_j) / lambda exactly
and every EBV, effect and score of (b) is exactly zero -- there is no |truth| to be relative to.  (b) is used where
its truth is not zero (z = L^-1 y, the quadratic form q, the log-likelihood), and (ab) puts the same component of
size 1 / lambda into the solution beside values of size one.  Two more inputs are left out because the float64
restatement itself misses the host bar on them (fit_cols, z_cols): z of (d) under the snp branch, and (d) for snp160
under forced gblup.  tests/test_structured_host.py::test_inputs_left_out_do_miss_the_host_bar keeps each figure.

Fixed effects (tests/test_gpu_structured_fixed.py, sections G to K).  The class factor is the family label (groups():
30 levels, confounded with relationship), the designs "cov3" (covariates()), "fam" (the factor) and "fam+n" (the factor
and the normal covariate; the family-0 indicator of covariates() is collinear with the factor).  cond(G) of
G = F~^T V^-1 F~ is at most 2.3e5, 7.4e2 and 1.6e6 -- the last over covar_ref.COND_MAX in two cases, which stay:
STRUCT_COND_MAX = 1e7 is the cap here.  Truths: adj_truth (u_P, v_P, q_P, b, likelihood), relfix_truth (adjusted
reliability, pev_total, cov_cov / fixed_cov), fixfit_truth (the model of fit(groups=)), loo_truth.  Errors follow the
rule above; b = [cov_effects, group_effects] is one output vector, a covariance matrix is taken whole.
Left out too, for the same reason as above (stat_cols, fixfit_cols): (d) under gblup with the class factor for q_P,
sigma2_g, the log-likelihood, u_P and the SNP effects / EBVs of y* -- the level means absorb the offset and
q_P = q - |C^-1 h|^2 cancels twelve digits (the float64 restatement is 1.2e6 host bars off at kappa 17); its GLS
effects b are compared.
The LOO rule: e_loo = e_t / (1 - h_tt), so pred, eloo, PRESS and the LOO fitness are held to bar / gap,
gap = min_t (1 - h_tt) of the truth (down to 6.8e-6 at h2 = 0.999999; on (200, 60) dual260 snp it is 1.5e-5 and the
float64 restatement's eloo is 780 host bars off without that factor, 0.012 with it); the leverages are held to the plain bar.  A case is kept only if
bar / gap <= LOO_GAP_MAX = 1e-2 (the worst is 6.2e-3), and LOO runs at h2 = 0.4, 0.9999 and 0.999999.
"""
import functools

import numpy as np

from tests import covar_ref as CV
from tests import group_ref as GR
from tests import loglik_ref as LL
from tests import loo_ref as LO
from tests import model_ref as R
from tests import reliab_cov_ref as RC
from tests import reliab_group_ref as RG
from tests import reliability_ref as Q
from tests import score_cov_ref as SC
from tests import score_ref as S
from tests.test_edge_cases_cpu import _pearson_wide, blup_wide      # noqa: F401  (blup_wide: re-exported)

LD = np.longdouble
U = 2.0 ** -53
N_ANIMALS, N_SNPS, BLOCK = 301, 640, 16
N_FAM, FAM = 29, 10
SPLITS = [(200, 60), (257, 40)]
H2S = (0.4, 0.99, 0.9999, 0.999999)
COLS = ("a", "b", "c", "d", "ab")            # columns of Y; the 4-trait engines take MT_COLS
MT_COLS = (0, 4, 2, 3)                       # (a), (ab), (c), (d)
TOL = 1e-9                                   # EBVs, effects, intercept, fitness, reliability, loglik, scores, GLS
CHOL_TOL = 1e-10                             # the factor and z (tests/test_gpu_edges.py)
PAIR_ROWS, STRADDLE_ROWS, TRIPLE_ROWS = (4, 5), (127, 128), (60, 140, 199)


def bar(kappa, tol=TOL):
    return max(tol, 16.0 * kappa * U)


def host_bar(kappa, tol=TOL):
    return max(tol / 8.0, 2.0 * kappa * U)


def relerr(got, truth):
    """max |got - truth| / max |truth| in longdouble."""
    truth = np.asarray(truth, dtype=LD)
    return float(np.max(np.abs(np.asarray(got).astype(LD) - truth)) / np.max(np.abs(truth)))


# ---------------------------------------------------------------------------------------------
# The panel
# ---------------------------------------------------------------------------------------------
def _block_patterns(rng, npat=5):
    """(npat, BLOCK) 0/1 patterns of one LD block and their frequencies."""
    cols = []
    while len(cols) < BLOCK:
        if cols and rng.random() < 0.75:
            v = cols[-1].copy()
            if rng.random() < 0.5:
                v[rng.integers(npat)] ^= 1
        else:
            v = rng.integers(0, 2, npat)
        if 0 < v.sum() < npat:
            cols.append(v)
    return np.stack(cols, axis=1), rng.dirichlet(np.full(npat, 2.0))


@functools.lru_cache(maxsize=None)
def panel():
    rng = np.random.default_rng(301640)
    n, P, nb = N_ANIMALS, N_SNPS, N_SNPS // BLOCK
    n_found = 2 * N_FAM + (n - N_FAM * FAM)
    hap = np.zeros((n_found, 2, P), dtype=np.int8)              # founders: the parents, then the unrelated animals
    breed = (np.arange(n_found) // 2) % 2                       # two breeds: the pattern frequencies reversed
    for b in range(nb):
        pat, freq = _block_patterns(rng)
        pid = np.where(breed[:, None] == 0, rng.choice(len(freq), size=(n_found, 2), p=freq),
                       rng.choice(len(freq), size=(n_found, 2), p=freq[::-1]))
        hap[:, :, b * BLOCK:(b + 1) * BLOCK] = pat[pid]
    hap ^= (rng.random(hap.shape) < 0.02).astype(np.int8)
    geno = np.zeros((n, P), dtype=np.int8)
    family = np.full(n, -1)
    for f in range(N_FAM):
        for c in range(FAM):
            a = f * FAM + c
            family[a] = f
            for b in range(nb):
                sl = slice(b * BLOCK, (b + 1) * BLOCK)
                h = hap[2 * f, rng.integers(2), sl].copy(), hap[2 * f + 1, rng.integers(2), sl].copy()
                for x in h:
                    x ^= (rng.random(BLOCK) < 0.005).astype(np.int8)
                geno[a, sl] = h[0] + h[1]
    unrelated = np.arange(N_FAM * FAM, n)
    geno[unrelated] = hap[2 * N_FAM:].sum(axis=1)

    # the SNP-form genome's columns: blocks 3..11 whole, the first half of blocks 12 and 13
    base = np.concatenate([np.arange(3 * BLOCK, 12 * BLOCK), np.arange(12 * BLOCK, 12 * BLOCK + 8),
                           np.arange(13 * BLOCK, 13 * BLOCK + 8)])
    assert len(base) == 160
    dup, comp = (3 * BLOCK + 5, 8 * BLOCK + 2), (5 * BLOCK + 9, 10 * BLOCK + 4)
    rare = np.array([b * BLOCK + o for b in range(3, 12) for o in (7, 13)] + [12 * BLOCK + 3, 13 * BLOCK + 3])
    assert len(rare) == 20 and set(rare) <= set(base) and not set(rare) & set(dup + comp)

    # clones (members of families, so they have sibs) and carriers (one per rare column), all train rows
    pair, straddle, triple = (0, 1), (10, 11), (20, 21, 22)     # families 0, 1 and 2
    clones = pair + straddle + triple
    sibs = np.array([2, 3, 12, 13, 23, 24])                     # sibs of each clone group: validation animals
    order = rng.permutation(np.setdiff1d(np.arange(n), clones + tuple(sibs)))
    carriers, rest = order[:20], order[20:]
    loose = rest[np.isin(rest, unrelated)][:3]                  # unrelated validation animals
    rest = rest[~np.isin(rest, loose)]
    V60 = np.concatenate([sibs, loose, rest[:51]])
    rest = rest[51:]
    T257 = np.full(257, -1)
    for rows, an in ((PAIR_ROWS, pair), (STRADDLE_ROWS, straddle), (TRIPLE_ROWS, triple)):
        T257[list(rows)] = an
    free = np.flatnonzero(T257[:200] < 0)
    T257[rng.choice(free, 20, replace=False)] = carriers
    T257[T257 < 0] = np.concatenate([rest, V60[40:]])[:int(np.sum(T257 < 0))]
    T200, V40 = T257[:200].copy(), V60[:40].copy()

    geno[:, dup[1]] = geno[:, dup[0]]
    geno[:, comp[1]] = 2 - geno[:, comp[0]]
    geno[:, rare] = 0
    geno[carriers, rare] = 1
    for grp in (pair, straddle, triple):
        geno[list(grp[1:])] = geno[grp[0]]
    later = np.array(pair[1:] + straddle[1:] + triple[1:])
    Tcf = T200[~np.isin(T200, later)].copy()
    splits = {(200, 60): (T200, V60), (257, 40): (T257, V40), "cf": (Tcf, V60)}

    # genomes
    others = np.setdiff1d(base, dup + comp)
    g160 = np.full(160, -1)
    g160[[4, 5]], g160[[127, 128]] = dup, comp
    g160[g160 < 0] = rng.permutation(others)
    g158 = g160[~np.isin(g160, (dup[1], comp[1]))]
    outside = np.setdiff1d(np.arange(P), base)
    genomes = {"snp160": g160, "snp158": g158,
               "dual260": rng.permutation(np.concatenate([base, rng.choice(outside, 100, replace=False)])),
               "g400": rng.choice(P, 400, replace=False), "g130": rng.choice(outside, 130, replace=False)}

    # phenotypes
    Y = np.zeros((n, 5))
    Y[:, 0] = rng.standard_normal(n)
    Y[pair[0], 1], Y[pair[1], 1] = 1.0, -1.0
    w = geno.astype(np.float64) - geno.mean(axis=0)
    g = w @ (rng.standard_normal(P) * (rng.random(P) < 0.1))
    bv = g / g.std()
    Y[:, 2] = bv + rng.standard_normal(n)
    Y[:, 3] = Y[:, 0] + 1e6
    Y[:, 4] = Y[:, 0] + Y[:, 1]
    for arr in (geno, Y, family):
        arr.setflags(write=False)
    return {"geno": geno, "Y": Y, "family": family, "splits": splits, "genomes": genomes, "dup": dup, "comp": comp,
            "rare": rare, "carriers": carriers, "clones": {"pair": pair, "straddle": straddle, "triple": triple},
            "sibs": sibs, "unrelated": unrelated, "base": base, "bv": bv}


def pheno(cols):
    """The phenotype argument of an engine: one column (n,) or several (n, t) of Y, by index."""
    Y = panel()["Y"]
    return np.ascontiguousarray(Y[:, cols[0]] if len(cols) == 1 else Y[:, list(cols)])


def cand_snps():
    """Candidates of the score test: DUP's second column (the duplicate of a SNP of snp160 and of dual260), DUP's
    first, COMP's two, two rare columns, two columns of block 12's other half (outside snp160, inside one of its LD
    blocks), three columns far from every model block, one negative index, and the first again."""
    pn = panel()
    P = N_SNPS
    out = [pn["dup"][1], pn["dup"][0], pn["comp"][1], pn["comp"][0], pn["rare"][0], pn["rare"][-1],
           12 * BLOCK + 8, 12 * BLOCK + 15, 0, 30 * BLOCK + 1, P - 1, 12 * BLOCK + 9 - P, pn["dup"][1]]
    return np.array(out, dtype=np.int64)


def rel_animals():
    """Animals of the reliability test: every clone, the sibs of each clone group, three unrelated validation
    animals, two carriers and two ordinary train animals."""
    pn = panel()
    c = pn["clones"]
    T = pn["splits"][200, 60][0]
    return np.concatenate([c["pair"], c["straddle"], c["triple"], pn["sibs"], pn["splits"][200, 60][1][6:9],
                           pn["carriers"][:2], T[[0, 199]]]).astype(np.int64)


def covariates():
    """Q (n, 3): the indicator of family 0 (the in-block clone pair's: nearly in the span of the genotypes), the
    breeding-value phenotype's rank scaled to [0, 1), and a standard normal column."""
    pn = panel()
    rng = np.random.default_rng(3016403)
    q = np.stack([(pn["family"] == 0).astype(np.float64), np.argsort(np.argsort(pn["Y"][:, 2])) / float(N_ANIMALS),
                  rng.standard_normal(N_ANIMALS)], axis=1)
    return np.ascontiguousarray(q)


# ---------------------------------------------------------------------------------------------
# Cases: (split, genome, branch).  MODELS are the distinct fitted models; `auto` maps onto them.
# ---------------------------------------------------------------------------------------------
GENOMES = ("snp160", "dual260", "g400", "g130")
MODELS = [(g, br) for g in GENOMES for br in ("snp", "gblup")]
AUX_MODELS = [("snp160", "snp"), ("dual260", "snp"), ("g400", "gblup"), ("g130", "gblup")]


def fit_cols(branch, gkey=None):
    """The columns of Y whose solution is compared: (a), (ab), (c) and (d).  Not (b), whose solution is zero, and not
    (d) for snp160 under forced gblup, where the oracle's own K_VT alpha is 4.4 kappa u from the truth on the
    three-tile split (tests/test_structured_host.py asks for 2 and keeps the figure)."""
    return (0, 4, 2) if branch == "gblup" and gkey == "snp160" else (0, 4, 2, 3)


FITNESS_COLS = (0, 4, 2, 3)                  # every compared column (the fitness is held to the bar absolutely)


def z_cols(branch):
    """The columns whose z = L^-1 (y_T - mu) is compared: all five under gblup, all but (d) under snp, where mu is
    mean(y_T) in float64: at 1e6 it is rounded at 1e-10, the shift lies along K_TT's null vector 1 and reaches z
    over sqrt(lambda) (numpy's own z is 4.7e-11 off at h2 = 0.4, host bar 1.25e-11); the EBVs do not see it."""
    return (0, 1, 2, 3, 4) if branch == "gblup" else (0, 1, 2, 4)


# evaluate / fit / predict: every model, split and h2
FIT_CASES = [(s, g, br, h) for s in SPLITS for g, br in MODELS for h in H2S]
# the factor readback (kernel form): the SNP-form genome, the gblup genome, and the forced gblup genome at k < n_T
# whose offset column is the open finding of tests/test_gpu_structured.py's section F
FACTOR_MODELS = (("snp160", "snp"), ("g400", "gblup"), ("g130", "gblup"))
FACTOR_CASES = [(s, g, br, h) for s in SPLITS for g, br in FACTOR_MODELS for h in H2S]
# reliability, SNP scores, covariates: both ends of the h2 range on two tiles, the stressed end on three
AUX_CASES = ([((200, 60), g, br, h) for g, br in AUX_MODELS for h in (0.4, 0.999999)]
             + [((257, 40), g, br, 0.999999) for g, br in AUX_MODELS])
# log-likelihood: every h2 on two tiles, the stressed end on three
LL_CASES = ([((200, 60), g, br, h) for g, br in AUX_MODELS for h in H2S]
            + [((257, 40), g, br, 0.999999) for g, br in AUX_MODELS])


def own_form(split, gkey, branch):
    """The form the float64 restatements solve a model in (sklearn's rule: model_ref.fit_ref, score_ref, the
    oracle): the SNP form for the snp branch at k <= n_T.  (The library's rule counts tiles: form_of.)"""
    pn = panel()
    small = len(pn["genomes"][gkey]) <= len(pn["splits"][split][0])
    return "snp" if fitted_branch(gkey, branch) == "snp" and small else "kernel"


def fitted_branch(gkey, branch):
    return R._branch(len(panel()["genomes"][gkey]), N_ANIMALS, branch)


def form_of(gkeys, split, branch):
    """The form tblup's automatic choice gives a batch: the SNP form when every model takes the snp branch and the
    largest k gives no more 128-row tiles than n_T."""
    pn = panel()
    nT = len(pn["splits"][split][0])
    kmax = max(len(pn["genomes"][g]) for g in gkeys)
    all_snp = all(fitted_branch(g, branch) == "snp" for g in gkeys)
    return "snp" if all_snp and -(-kmax // 128) <= -(-nT // 128) else "kernel"


def _system(split, gkey, branch, h2, form, dtype=np.float64):
    """The solved matrix (scaled as K_TT + lambda I; the SNP form's is W_T^T W_T / d + lambda I_k) in dtype."""
    pn = panel()
    _, wt, d, lam = Q._setup(pn["genomes"][gkey], pn["splits"][split][0], pn["geno"], h2, branch, dtype)
    A = (wt.T @ wt if form == "snp" else wt @ wt.T) / d
    A[np.diag_indices_from(A)] += lam
    return A


@functools.lru_cache(maxsize=None)
def _spectrum(split, gkey, branch, form):
    e = np.linalg.eigvalsh(_system(split, gkey, fitted_branch(gkey, branch), 1.0, form))
    return float(e[0]), float(e[-1])


def kappa(split, gkey, branch, h2, form):
    """cond_2 of the solved system from the float64 spectrum of its lambda = 0 part; inf when that is not positive."""
    lo, hi = _spectrum(split, gkey, fitted_branch(gkey, branch), form)
    lam = (1.0 - h2) / h2
    lo = max(lo, 0.0) + lam if lam > 0 else lo
    return (hi + lam) / lo if lo > 0 else np.inf


def block_kappa(split, gkey, branch, h2, lo=0, hi=16):
    """cond_2 of one diagonal block of the kernel-form system: what an explicit inverse of that block is
    sensitive to."""
    A = _system(split, gkey, fitted_branch(gkey, branch), h2, "kernel")[lo:hi, lo:hi]
    return float(np.linalg.cond(A))


# ---------------------------------------------------------------------------------------------
# Truths (longdouble), once per case
# ---------------------------------------------------------------------------------------------
def _args(split, gkey):
    pn = panel()
    T, V = pn["splits"][split]
    return pn["genomes"][gkey], T, V, pn["geno"]


@functools.lru_cache(maxsize=None)
def fit_truth(split, gkey, branch, h2):
    """{effects (5, k), intercept (5,), ebv (5, n) of every animal, fitness (5,)} of the five columns of Y from
    model_ref.fit_wide (one longdouble factor), or None where its Cholesky meets a pivot that is not positive."""
    pn = panel()
    idx, T, V, geno = _args(split, gkey)
    br = fitted_branch(gkey, branch)
    eff = R.fit_wide(idx, T, geno, pn["Y"], h2, br)
    if eff is None or not np.all(np.isfinite(eff)):
        return None
    Y = pn["Y"].astype(LD)
    ref = np.arange(N_ANIMALS) if br == "gblup" else T
    a = geno[:, idx].astype(np.int64)
    w = a.astype(LD) - a[ref].sum(axis=0).astype(LD) / LD(len(ref))
    mu = np.zeros(Y.shape[1], dtype=LD) if br == "gblup" else Y[T].sum(axis=0) / LD(len(T))
    ebv = (w @ eff + mu).T
    fit = np.array([_pearson_wide(ebv[t][V], Y[V, t])[0] for t in range(Y.shape[1])])
    out = {"effects": np.ascontiguousarray(eff.T), "intercept": mu, "ebv": np.ascontiguousarray(ebv), "fitness": fit}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def k_truth(split, gkey, branch):
    """K_{R,T}, R the train rows then the validation rows, without the lambda shift, in longdouble from the exact
    integer N^2 W_R W_T^T (as loglik_ref.loglik_wide builds V): what debug_grm stage 1 reads back."""
    idx, T, Vr, geno = _args(split, gkey)
    br = fitted_branch(gkey, branch)
    a = geno[:, idx].astype(np.int64)
    ref = np.arange(N_ANIMALS) if br == "gblup" else T
    N = len(ref)
    m = a[ref].sum(axis=0)
    sm, qq = int(m.sum()), int(np.sum(m * m))
    d = LD(2 * N * sm - qq) / LD(2 * N * N)
    rows = np.concatenate([T, Vr])
    u = a @ m
    M = (N * N) * (a[rows] @ a[T].T) - N * (u[rows][:, None] + u[T][None, :]) + qq
    K = M.astype(LD) / (LD(N * N) * d)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def factor_truth(split, gkey, branch, h2):
    """(L, z): the lower Cholesky factor of the kernel-form K_TT + lambda I (k_truth's exact K_TT) and
    z = L^-1 (y_T - mu) of the five columns of Y, in longdouble."""
    pn = panel()
    T = pn["splits"][split][0]
    br = fitted_branch(gkey, branch)
    V = k_truth(split, gkey, br)[:len(T)].copy()
    V[np.diag_indices_from(V)] += (LD(1) - LD(h2)) / LD(h2)
    L = Q._chol(V)
    y = pn["Y"].astype(LD)[T]
    if br == "snp":
        y = y - y.sum(axis=0) / LD(len(T))
    z = Q._forward(L, y)
    L.setflags(write=False)
    z.setflags(write=False)
    return L, z


@functools.lru_cache(maxsize=None)
def rel_truth(split, gkey, branch, h2):
    idx, T, _, geno = _args(split, gkey)
    r = Q.rel_wide(idx, T, geno, h2, fitted_branch(gkey, branch))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def loglik_truth(split, gkey, branch, h2):
    """(loglik (5,), sigma2_g (5,)) of the five columns of Y."""
    idx, T, _, geno = _args(split, gkey)
    return LL.loglik_wide(idx, T, geno, panel()["Y"], h2, fitted_branch(gkey, branch))


@functools.lru_cache(maxsize=None)
def score_truth(split, gkey, branch, h2):
    """(u (5, m), v (m,), q (5,)) of cand_snps() for the five columns of Y."""
    idx, T, _, geno = _args(split, gkey)
    return S.score_wide(idx, T, geno, panel()["Y"], h2, fitted_branch(gkey, branch), cand_snps())


@functools.lru_cache(maxsize=None)
def gls_truth(split, gkey, branch, h2):
    """covar_ref.gls_wide of covariates() for the five columns of Y, with `cond` of G and the model of the adjusted
    phenotype y* = y - Q~ b: `effects` (5, k) and `ebv` (5, n).  The fit is linear in the phenotype, so they are
    fit_wide's effects of Y less those of Q times b, with no rounding of y* to float64 in between."""
    idx, T, _, geno = _args(split, gkey)
    br = fitted_branch(gkey, branch)
    Qm = covariates()
    g = CV.gls_wide(idx, T, geno, panel()["Y"], Qm, h2, br)
    g["cond"] = float(np.linalg.cond(g["G"].astype(np.float64)))
    e = R.fit_wide(idx, T, geno, np.hstack([panel()["Y"], Qm]), h2, br)
    nt = panel()["Y"].shape[1]
    eff = e[:, :nt] - e[:, nt:] @ g["b"].T
    ref = np.arange(N_ANIMALS) if br == "gblup" else T
    a = geno[:, idx].astype(np.int64)
    w = a.astype(LD) - a[ref].sum(axis=0).astype(LD) / LD(len(ref))
    mu = LD(0) if br == "gblup" else g["ystar"][T].sum(axis=0) / LD(len(T))
    g["effects"], g["ebv"] = np.ascontiguousarray(eff.T), np.ascontiguousarray((w @ eff + mu).T)
    return g


# ---------------------------------------------------------------------------------------------
# Fixed effects on the panel: the designs, and the truths of the entries that adjust for them
# ---------------------------------------------------------------------------------------------
DESIGNS = ("cov3", "fam", "fam+n")
STRUCT_COND_MAX = 1e7                        # cond(F~^T V^-1 F~) of every structured case (covar_ref.COND_MAX is 1e6)
LOO_H2S = (0.4, 0.9999, 0.999999)
LOO_GAP_MAX = 1e-2                           # a LOO case is kept only if bar / gap stays below this


def groups():
    """The class factor: the family label, 29 families of 10 and -1 for the 11 unrelated animals (30 levels).  It is
    confounded with relationship: nearly in the span of the genotypes."""
    return panel()["family"]


def design(name):
    """(covariates or None, groups or None) of a design.  "fam+n" takes the normal column only: the first column of
    covariates() is the indicator of family 0, collinear with the factor."""
    return {"cov3": (covariates(), None), "fam": (None, groups()),
            "fam+n": (np.ascontiguousarray(covariates()[:, 2:]), groups())}[name]


def design_matrix(name, split, gkey, branch):
    """The dense fixed design F (n, C) of a model under its fitted branch (tests/group_ref.py::expand) and the
    number of covariate columns in front of the levels' columns."""
    cov, grp = design(name)
    if grp is None:
        return cov, cov.shape[1]
    F, _ = GR.expand(cov, grp, panel()["splits"][split][0], fitted_branch(gkey, branch))
    return F, 0 if cov is None else cov.shape[1]


def stat_cols(name, branch, cols=(0, 1, 2, 3, 4)):
    """The columns of Y whose q_P, log-likelihood, sigma2_g and u_P are compared under a design: not (d) under gblup
    with the class factor, where the level means absorb the offset and q_P = q - |C^-1 h|^2 cancels twelve digits
    (tests/test_structured_host.py keeps the float64 restatement's figure)."""
    return tuple(t for t in cols if not (t == 3 and branch == "gblup" and name != "cov3"))


def fixfit_cols(name, branch, gkey=None):
    """The columns of Y whose SNP effects, EBVs and fitness under a design are compared: fit_cols', and -- as for
    stat_cols -- not (d) under gblup with the class factor: y* = y - F~ b is 1e6 less 1e6, the float64 restatement
    rounds it at 1e-10 and its effects are 9.6 host bars off at kappa 17 (tests/test_structured_host.py keeps the
    figure).  The GLS effects b of (d) are compared everywhere (fit_cols)."""
    return stat_cols(name, branch, fit_cols(branch, gkey))


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def adj_truth(name, split, gkey, branch, h2):
    """score_cov_ref.adj_wide of a design for the five columns of Y and cand_snps(), with `cond` of G."""
    idx, T, _, geno = _args(split, gkey)
    br = fitted_branch(gkey, branch)
    F, _ = design_matrix(name, split, gkey, br)
    out = SC.adj_wide(idx, T, geno, panel()["Y"], F, h2, br, cand_snps())
    out["cond"] = float(np.linalg.cond(out["G"].astype(np.float64)))
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def relfix_truth(name, split, gkey, branch, h2):
    """reliab_cov_ref.vform_wide ("cov3") / reliab_group_ref.vform_wide of a design over all animals: rel, pev and
    cov_cov, which for the class factor is `fixed_cov` too (covariates then levels, zeros at the snp reference level)."""
    idx, T, _, geno = _args(split, gkey)
    br = fitted_branch(gkey, branch)
    cov, grp = design(name)
    if grp is None:
        return _frozen(RC.vform_wide(idx, T, geno, cov, h2, br))
    out = RG.vform_wide(idx, T, geno, cov, grp, h2, br)
    keep = np.flatnonzero(np.any(out["fixed_cov"] != 0, axis=0))
    fc = np.zeros(out["fixed_cov"].shape, dtype=LD)             # (_widen fills a float64 array: refill it in longdouble)
    fc[np.ix_(keep, keep)] = out["cov_cov"]
    out["fixed_cov"] = fc
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def fixfit_truth(name, split, gkey, branch, h2):
    """The model that fit(covariates=) / fit(groups=) returns under a design, as gls_truth builds it: covar_ref.gls_wide
    of the expanded design, and fit_wide on [Y, F] -- the effects are those of Y less those of F times b, with nothing
    rounded to float64 in between.  {b (5, C), m (C,), cov_effects (5, c), group_effects (5, L), group_center (L,),
    effects (5, k), ebv (5, n) of y*, total (5, n) = ebv + F~ b, fitness (5,) of y*, cond}."""
    idx, T, V, geno = _args(split, gkey)
    br = fitted_branch(gkey, branch)
    F, nc = design_matrix(name, split, gkey, br)
    Y = panel()["Y"]
    g = CV.gls_wide(idx, T, geno, Y, F, h2, br)
    g["cond"] = float(np.linalg.cond(g["G"].astype(np.float64)))
    e = R.fit_wide(idx, T, geno, np.hstack([Y, F]), h2, br)
    nt = Y.shape[1]
    eff = e[:, :nt] - e[:, nt:] @ g["b"].T
    ref = np.arange(N_ANIMALS) if br == "gblup" else T
    a = geno[:, idx].astype(np.int64)
    w = a.astype(LD) - a[ref].sum(axis=0).astype(LD) / LD(len(ref))
    mu = LD(0) if br == "gblup" else g["ystar"][T].sum(axis=0) / LD(len(T))
    ebv = (w @ eff + mu).T
    g["effects"], g["ebv"] = np.ascontiguousarray(eff.T), np.ascontiguousarray(ebv)
    g["total"] = np.ascontiguousarray(ebv + ((F.astype(LD) - g["m"]) @ g["b"].T).T)
    g["fitness"] = np.array([_pearson_wide(ebv[t][V], g["ystar"][V, t])[0] for t in range(nt)])
    g["cov_effects"] = g["b"][:, :nc]
    if design(name)[1] is not None:
        L = F.shape[1] - nc + (br == "snp")
        ge, gc = np.zeros((nt, L), dtype=LD), np.zeros(L, dtype=LD)
        ge[:, L - (F.shape[1] - nc):] = g["b"][:, nc:]
        if br == "snp":
            gc[1:] = g["m"][nc:]
            gc[0] = LD(1) - np.sum(g["m"][nc:])
        g["group_effects"], g["group_center"] = ge, gc
    return _frozen(g)


# Leave-one-out: (split, genome, branch, form, h2).  snp160 in both forms, the others in the kernel form; both splits at
# the top tier, (200, 60) below it.
LOO_MODELS = (("snp160", "snp", "snp"), ("snp160", "snp", "kernel"), ("dual260", "snp", "kernel"),
              ("g400", "gblup", "kernel"), ("g130", "gblup", "kernel"))
LOO_CASES = [(s, g, br, f, h) for h in LOO_H2S for s in SPLITS if s == (200, 60) or h == LOO_H2S[-1]
             for g, br, f in LOO_MODELS]


@functools.lru_cache(maxsize=None)
def loo_truth(split, gkey, branch, h2, form):
    """loo_ref.loo_wide of the five columns of Y: pred / eloo (5, n_T), leverage (n_T,), press / fitness (5,) and
    gap = min_t (1 - h_tt)."""
    idx, T, _, geno = _args(split, gkey)
    return _frozen(LO.loo_wide(idx, T, geno, panel()["Y"], h2, fitted_branch(gkey, branch), form))


def loo_bar(kap, gap, tol=TOL, host=False):
    """The LOO rule: pred, eloo, PRESS and fitness are e_t / (1 - h_tt), so they are held to bar / gap."""
    return (host_bar(kap, tol) if host else bar(kap, tol)) / gap


# ---------------------------------------------------------------------------------------------
# h2 = 1: lambda = 0
# ---------------------------------------------------------------------------------------------
# positive definite: (split, genome, branch, form)
PD_CASES = [("cf", "g400", "gblup", "kernel"),          # k = 400 columns on the clone-free train rows
            ((200, 60), "snp158", "snp", "snp"),        # the SNP form without DUP's and COMP's second columns
            ((200, 60), "g130", "snp", "snp"),
            ("cf", "dual260", "gblup", "kernel")]
# singular: (name, split, branch, form, batch, position of the singular individual); its batch-mates are of PD_CASES
SINGULAR_CASES = [("dup-columns", (200, 60), "snp", "snp", ("snp158", "snp160", "g130"), 1),
                  ("rank-130", "cf", "gblup", "kernel", ("g400", "g130", "dual260"), 1)]
# singular through the train rows (clones), which every batch-mate shares: evaluated alone
SINGULAR_ALONE = [("clones", (200, 60), "g400", "gblup", "kernel")]
