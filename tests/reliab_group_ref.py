"""Dense restatement of the uncertainty under the model with a class fixed effect (TEST INFRASTRUCTURE ONLY), and the
inputs shared by tests/test_reliab_group_host.py (CPU) and tests/test_gpu_reliab_group.py (GPU).

Nothing new is restated: (Q, groups) is expanded by tests/group_ref.py::expand to the dense fixed design F = [Q, Z] that
tblup_fit_group_batch documents, under the branch the model is fitted with, and handed to tests/reliab_cov_ref.py,
whose mixed-model-equation route in SNP space (mme_ref) and V-form (vform_ref / vform_wide) take any column count.
On top of that route come the two things the class factor adds to tblup_reliability_group_batch's outputs:

  fixed_cov  (c + L, c + L), covariates then levels: the expanded design's cov_cov with, under snp, a row and a column
             of zeros at the reference level (the lowest), whose effect is 0 by construction
  pev        NaN for a listed animal whose label no train animal has (PanelModel.predict's rule); its reliability
             needs no design row and stays defined
"""
import functools

import numpy as np

from tests import group_ref as G
from tests import group_stats_ref as GS
from tests import model_ref as R
from tests import reliab_cov_ref as Q

H2 = Q.H2
TOL = Q.TOL                      # the GPU tests' bound: |got - ref| <= TOL max(1, max |ref|)
HOST_TOL = Q.HOST_TOL
COND_MAX = Q.COND_MAX
close = Q.close
panel = G.panel
deep_panel = G.deep_panel
big_panel = GS.big_panel
DESIGNS = G.DESIGNS
DESIGN_SPLITS = G.DESIGN_SPLITS
AUTO_KEYS = G.AUTO_KEYS
GBLUP_KEYS = G.GBLUP_KEYS
snp_keys = G.snp_keys
design_inputs = G.design_inputs
deep_inputs = G.deep_inputs
make_groups = G.make_groups
big_inputs = GS.big_inputs
BIG_L, BIG_C = GS.BIG_L, GS.BIG_C
animal_list = Q.animal_list
LIST_LENGTHS = (1, 15, 16, 17, 33)
HOST_KEYS = GS.HOST_KEYS
fitted_branch = GS.fitted_branch
design = GS.design


def _widen(out, nc, L, groups, train, animals, n):
    """reliab_cov_ref's result of the expanded design as the class-factor entry returns it."""
    snp = out["branch"] == "snp"
    cc = out["cov_cov"]
    fc = np.zeros((nc + L, nc + L))
    keep = np.array([j for j in range(nc + L) if not (snp and j == nc)])
    fc[np.ix_(keep, keep)] = cc
    g = np.asarray(groups)
    an = np.arange(n) if animals is None else np.asarray(animals, dtype=np.int64)
    unseen = ~np.isin(g[an], G.levels_of(g, train))
    res = dict(out)
    res["pev"] = np.where(unseen, np.nan, out["pev"])
    res["fixed_cov"] = fc
    res["unseen"] = unseen
    return res


def _route(fn, idx, train, geno, cov, groups, h2, branch, animals, **kw):
    X, lev = design(idx, train, geno, cov, groups, branch)
    nc = X.shape[1] - (len(lev) - (fitted_branch(idx, geno, branch) == "snp"))
    out = fn(idx, train, geno, X, h2, branch, animals, **kw)
    return _widen(out, nc, len(lev), groups, train, animals, np.asarray(geno).shape[0])


def mme_ref(idx, train, geno, cov, groups, h2, branch="auto", animals=None, check=True):
    """{rel (m,), pev (m,), cov_cov (C_m, C_m), fixed_cov (c + L, c + L), kaa (m,), unseen (m,), branch} for the listed
    animals (None: all) from the mixed-model equations in SNP space on the expanded design, float64.  check:
    reliab_cov_ref.mme_ref's -- cond(G) <= COND_MAX and K_aa > 0 for every listed animal."""
    return _route(Q.mme_ref, idx, train, geno, cov, groups, h2, branch, animals, check=check)


def vform_ref(idx, train, geno, cov, groups, h2, branch="auto", animals=None):
    """The definitions as the header writes them (dense V, one column Cholesky), float64."""
    return _route(Q.vform_ref, idx, train, geno, cov, groups, h2, branch, animals)


def vform_wide(idx, train, geno, cov, groups, h2, branch="auto", animals=None):
    """The same in np.longdouble."""
    return _route(Q.vform_wide, idx, train, geno, cov, groups, h2, branch, animals)


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name, split, key, branch):
    """mme_ref of (design, split, genome key, branch) over all animals of the 331 x 600 panel, once (read-only)."""
    pn = panel()
    T, _ = pn["splits"][split]
    cov, groups = design_inputs(name, split)
    return _freeze(mme_ref(pn["genomes"][key], T, pn["geno"], cov, groups, H2, branch))


@functools.lru_cache(maxsize=None)
def deep_ref():
    dp = deep_panel()
    cov, groups = deep_inputs()
    return _freeze(mme_ref(dp["genome"], dp["train"], dp["geno"], cov, groups, H2))


@functools.lru_cache(maxsize=None)
def big_ref(name):
    """mme_ref of a case of score_cov_ref.big_cases() with group_stats_ref's 24 levels + 3 covariates, all animals."""
    from tests import score_cov_ref as A
    bp = big_panel()
    _, g, t, v, _, br, _, _ = next(x for x in A.big_cases() if x[0] == name)
    cov, groups = big_inputs(t)
    return _freeze(mme_ref(bp[g], bp[t], bp["geno"], cov, groups, H2, br))
