"""Dense restatement of the fitted model with a class fixed effect (TEST INFRASTRUCTURE ONLY), and the inputs
shared by tests/test_group_host.py (CPU) and tests/test_gpu_group.py (GPU).

Nothing new is restated: (Q, groups) is expanded to the dense fixed design F = [Q, Z] that
tblup_fit_group_batch documents (include/tblup_gpu.h) and handed to tests/covar_ref.py, whose cov_ref / gls_ref /
gls_wide take any column count:

  gblup : Z has one 0/1 column per level, in ascending label order; nothing is centred
  snp   : Z drops the lowest level (the reference); cov_ref centres every column by its train mean, which for
          a level's column is the level's share n_l / n_T of the train rows

The levels are np.unique of the train rows' labels; an animal with any other label has a row of zeros in Z.
"""
import functools

import numpy as np

from tests import covar_ref as C
from tests import model_ref as R

H2 = C.H2
TOL = C.TOL
HOST_TOL = C.HOST_TOL
COND_MAX = C.COND_MAX
MAX_FIXED = 128
close = C.close
panel = C.panel
deep_panel = C.deep_panel


def make_groups(n, L, train, seed=0):
    """(n,) integer labels drawn uniformly over L levels; the first L train animals get levels 0 .. L-1, so
    every level has a train record."""
    rng = np.random.default_rng(5100 + 10 * L + seed)
    g = rng.integers(0, L, n).astype(np.int64)
    g[np.asarray(train)[:L]] = np.arange(L)
    return g


def levels_of(groups, train):
    return np.unique(np.asarray(groups)[np.asarray(train)])


def expand(cov, groups, train, branch):
    """The dense (n, c + L) design under "gblup", (n, c + L - 1) under "snp", and the levels."""
    g = np.asarray(groups)
    lev = levels_of(g, train)
    Z = (g[:, None] == lev[None, :]).astype(np.float64)
    if branch == "snp":
        Z = Z[:, 1:]
    elif branch != "gblup":
        raise ValueError("branch must be the fitted one: gblup or snp")
    parts = [] if cov is None else [np.asarray(cov, dtype=np.float64).reshape(len(g), -1)]
    return np.ascontiguousarray(np.hstack(parts + [Z])), lev


def _split_effects(b, m, nc, L, br):
    """(cov_effects, cov_center, group_effects, group_center) out of the expanded design's b (nt, C), m (C,)."""
    nt = b.shape[0]
    ge, gc = np.zeros((nt, L)), np.zeros(L)
    dead = not np.all(np.isfinite(b)) or not np.all(np.isfinite(m))
    if br == "snp":
        ge[:, 1:], gc[1:] = b[:, nc:], m[nc:]
        gc[0] = 1.0 - np.sum(m[nc:], dtype=np.longdouble)
    else:
        ge[:] = b[:, nc:]
    if dead:
        ge[:], gc[:] = np.nan, np.nan
    return b[:, :nc], m[:nc], ge, gc


def group_ref(idx, train, valid, geno, pheno, cov, groups, h2, branch="auto"):
    """Everything tblup_fit_group_batch returns for one model, in float64: covar_ref.cov_ref of the expanded design
    with its cov_effects / cov_center split into the covariates' and the levels' (group_effects (nt, L), zero at
    the reference level under snp; group_center (L,), the train shares under snp), plus group_levels and cond."""
    br = R._branch(len(np.asarray(idx)), np.asarray(geno).shape[0], branch)
    X, lev = expand(cov, groups, train, br)
    nc = X.shape[1] - (len(lev) - (br == "snp"))
    out = dict(C.cov_ref(idx, train, valid, geno, pheno, X, h2, branch))
    ce, cc, ge, gc = _split_effects(out["cov_effects"], out["cov_center"], nc, len(lev), br)
    out.update(cov_effects=ce, cov_center=cc, group_effects=ge, group_center=gc, group_levels=lev, columns=X.shape[1])
    return out


def gls_pair(idx, train, geno, pheno, cov, groups, h2, branch="auto"):
    """(float64, longdouble) GLS of the expanded design: covar_ref.gls_ref and gls_wide."""
    br = R._branch(len(np.asarray(idx)), np.asarray(geno).shape[0], branch)
    X, _ = expand(cov, groups, train, br)
    return C.gls_ref(idx, train, geno, pheno, X, h2, branch), C.gls_wide(idx, train, geno, pheno, X, h2, branch)


# ---------------------------------------------------------------------------------------------
# Designs (levels, covariates) and where they run.  18 levels without covariates is the first wide case under
# snp (17 columns: one in the second slab); 40 levels with 3 covariates is three slabs, the last partial;
# 113 levels with 15 covariates is 127 columns under snp and 128, the limit, under gblup.
# ---------------------------------------------------------------------------------------------
DESIGNS = {"L18": (18, 0), "L40c3": (40, 3), "L113c15": (113, 15)}
DESIGN_SPLITS = {"L18": [(127, 5), (129, 64)], "L40c3": [(128, 2), (257, 70)], "L113c15": [(257, 70)]}
AUTO_KEYS = [64, 127, 200, 332, 400]       # 332 and 400 exceed n = 331: gblup models in the ragged batch
GBLUP_KEYS = [64, 200]
DEEP_DESIGN = (40, 0)


def snp_keys(nT):
    """forced snp at k > n_T: the kernel form"""
    return [k for k in (200, 332, 400) if k > nT][:2]


def design_inputs(name, split):
    """(cov or None, groups) of a design on the 331 x 600 panel for a split."""
    L, c = DESIGNS[name]
    T, _ = panel()["splits"][split]
    return (C.make_cov(R.N_ANIMALS, c) if c else None), make_groups(R.N_ANIMALS, L, T)


@functools.lru_cache(maxsize=None)
def case_ref(name, split, key, branch):
    """group_ref of (design, split, genome key, branch), computed once (read-only)."""
    pn = panel()
    T, V = pn["splits"][split]
    cov, groups = design_inputs(name, split)
    out = group_ref(pn["genomes"][key], T, V, pn["geno"], pn["pheno"], cov, groups, H2, branch)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def deep_inputs():
    dp = deep_panel()
    L, c = DEEP_DESIGN
    return (C.make_cov(len(dp["pheno"]), c) if c else None), make_groups(len(dp["pheno"]), L, dp["train"])


@functools.lru_cache(maxsize=None)
def deep_ref():
    dp = deep_panel()
    cov, groups = deep_inputs()
    out = group_ref(dp["genome"], dp["train"], dp["valid"], dp["geno"], dp["pheno"], cov, groups, H2)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
