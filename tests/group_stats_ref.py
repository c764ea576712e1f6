"""Dense restatement of the score statistics and the restricted likelihood of h2 under a class fixed effect (TEST
INFRASTRUCTURE ONLY), and the inputs shared by tests/test_group_stats_host.py (CPU) and
tests/test_gpu_group_stats.py (GPU).

Nothing is restated: (Q, groups) is expanded by tests/group_ref.py::expand to the dense fixed design F = [Q, Z] that
tblup_fit_group_batch documents, under the branch the model is fitted with, and handed to tests/score_cov_ref.py,
whose adj_ref / adj_wide / contrast_ref / estimate_ref take any column count.  dof = N - r - C_m follows from the
expanded design's own width.
"""
import functools

import numpy as np

from tests import group_ref as G
from tests import model_ref as R
from tests import score_cov_ref as A

H2 = A.H2
H2S = A.H2S
TOL = A.TOL                      # the GPU tests' bound: |got - ref| <= TOL max(1, max |ref|)
LL_TOL = A.LL_TOL
HOST_TOL = A.HOST_TOL
SPAN_MIN = A.SPAN_MIN
COND_MAX = G.COND_MAX
close = A.close
panel = G.panel
deep_panel = G.deep_panel
big_panel = A.big_panel
cand_list = A.cand_list
LIST_LENGTHS = A.LIST_LENGTHS
DESIGNS = G.DESIGNS
DESIGN_SPLITS = G.DESIGN_SPLITS
AUTO_KEYS = G.AUTO_KEYS
GBLUP_KEYS = G.GBLUP_KEYS
snp_keys = G.snp_keys
design_inputs = G.design_inputs
deep_inputs = G.deep_inputs
make_groups = G.make_groups
HOST_KEYS = (64, 127, 200, 332)   # the host sweep's genomes


def fitted_branch(idx, geno, branch="auto"):
    return R._branch(len(np.asarray(idx)), np.asarray(geno).shape[0], branch)


def design(idx, train, geno, cov, groups, branch="auto"):
    """The expanded design of the model (under its fitted branch) and the levels."""
    return G.expand(cov, groups, train, fitted_branch(idx, geno, branch))


def adj_ref(idx, train, geno, pheno, cov, groups, h2, branch="auto", snps=None):
    """score_cov_ref.adj_ref on the expanded design: {u, v, q, loglik, sigma2_g, b (nt, C_m), dof, G, v_plain}."""
    X, _ = design(idx, train, geno, cov, groups, branch)
    return A.adj_ref(idx, train, geno, pheno, X, h2, branch, snps)


def adj_wide(idx, train, geno, pheno, cov, groups, h2, branch="auto", snps=None):
    X, _ = design(idx, train, geno, cov, groups, branch)
    return A.adj_wide(idx, train, geno, pheno, X, h2, branch, snps)


def contrast_ref(idx, train, geno, pheno, cov, groups, h2, branch="auto"):
    X, _ = design(idx, train, geno, cov, groups, branch)
    return A.contrast_ref(idx, train, geno, pheno, X, h2, branch)


def estimate_ref(idx, train, geno, pheno, cov, groups, branch="auto", **kw):
    X, _ = design(idx, train, geno, cov, groups, branch)
    return A.estimate_ref(idx, train, geno, pheno, X, branch, **kw)


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name, split, key, branch, h2=H2, all_snps=True):
    """adj_ref of (design, split, genome key, branch) on the 331 x 600 panel at h2, over all columns or none (the
    likelihood alone), computed once (read-only)."""
    pn = panel()
    T, _ = pn["splits"][split]
    cov, groups = design_inputs(name, split)
    snps = None if all_snps else np.zeros(0, dtype=np.int64)
    return _freeze(adj_ref(pn["genomes"][key], T, pn["geno"], pn["pheno"], cov, groups, h2, branch, snps))


@functools.lru_cache(maxsize=None)
def deep_ref(h2=H2, all_snps=True):
    dp = deep_panel()
    cov, groups = deep_inputs()
    snps = None if all_snps else np.zeros(0, dtype=np.int64)
    return _freeze(adj_ref(dp["genome"], dp["train"], dp["geno"], dp["pheno"], cov, groups, h2, "auto", snps))


# The 1200 x 1100 panel of the LDS-limit tests (score_cov_ref.big_panel) with a design of more than 16 columns:
# 24 levels and 3 covariates, 26 columns under snp and 27 under gblup (two slabs, the second partial).
BIG_L, BIG_C = 24, 3


@functools.lru_cache(maxsize=None)
def big_inputs(train_key):
    bp = big_panel()
    cov = np.ascontiguousarray(bp["cov_snp"][:, :BIG_C])
    groups = make_groups(A.BIG_N, BIG_L, bp[train_key], seed=7)
    groups.setflags(write=False)
    return cov, groups


@functools.lru_cache(maxsize=None)
def big_ref(name):
    bp = big_panel()
    _, g, t, v, _, br, _, _ = next(x for x in A.big_cases() if x[0] == name)
    cov, groups = big_inputs(t)
    return _freeze(adj_ref(bp[g], bp[t], bp["geno"], bp["pheno"], cov, groups, H2, br, snps=bp["snps"]))


# estimate_h2 under a class factor: a phenotype with strong level effects on the 331 x 600 panel
EST_L = 20


@functools.lru_cache(maxsize=None)
def est_inputs():
    e = A.est_inputs()
    rng = np.random.default_rng(5151)
    groups = make_groups(R.N_ANIMALS, EST_L, e["T"], seed=3)
    y = e["pheno"] + 2.0 * rng.standard_normal(EST_L)[groups]
    return _freeze({"geno": e["geno"], "pheno": y, "cov": e["cov"], "groups": groups, "genome": e["genome"],
                    "T": e["T"], "V": e["V"]})
