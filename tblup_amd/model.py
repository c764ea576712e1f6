"""PanelModel: the fitted model of one selected SNP panel, as a breeder deploys it.

The reference ends a blup() call with |pearson| and drops what it fitted on the way
(tblup/evaluator.py:284-286, 311-314).  `GpuBlupEngine.fit` / `tblup_fit_batch` return it: for the
selected columns idx[0..k) (duplicates kept, each occurrence its own column, as
data[:, indices]),

    EBV_t(a) = intercept[t] + sum_j (x[a, idx_j] - center[j]) * effects[t][j]

`predict` below is that formula in plain numpy, so a saved model needs neither the GPU nor the
library to be applied to a genotype matrix.

A model fitted with fixed-effect covariates (`GpuBlupEngine.fit(..., covariates=Q)`,
tblup_fit_cov_batch) also carries their GLS effects and centre; the value of an animal with
covariates q is then the genomic value above plus sum_i (q_i - cov_center[i]) * cov_effects[t][i].
A model fitted with a class factor (`fit(..., groups=labels)`, tblup_fit_group_batch) carries the fitted
levels, their effects and centres as well: an animal of level g adds
sum_l ([g == group_levels[l]] - group_center[l]) * group_effects[t][l], and NaN if g is not a fitted level.
"""
import numpy as np


class PanelModel:
    """indices (k,) wrapped to [0, P); center (k,) = 2p of each column over the branch's reference
    rows; effects (nt, k); intercept (nt,); h2, branch ("gblup" / "snp": the branch that was fitted)
    and the fit's validation fitness.  cov_effects (nt, c) and cov_center (c,): the fitted fixed-effect
    covariates, or None for a model without any.  group_levels (L,) the sorted labels of a fitted class factor,
    group_effects (nt, L) and group_center (L,): their effects (0 at the reference level under snp) and centres
    (the levels' shares of the train rows under snp, zero under gblup), or None for a model without one."""

    __slots__ = ("indices", "center", "effects", "intercept", "h2", "branch", "fitness", "cov_effects", "cov_center",
                 "group_levels", "group_effects", "group_center")

    def __init__(self, indices, center, effects, intercept, h2=float("nan"), branch="snp", fitness=float("nan"),
                 cov_effects=None, cov_center=None, group_levels=None, group_effects=None, group_center=None):
        idx = np.asarray(indices)
        if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("indices must be a non-empty 1-D integer array")
        if int(idx.min()) < 0:
            raise ValueError("indices must be non-negative (wrap negative indices by the panel width first)")
        self.indices = np.ascontiguousarray(idx, dtype=np.int64)
        k = self.indices.shape[0]
        self.center = np.ascontiguousarray(center, dtype=np.float64)
        if self.center.shape != (k,):
            raise ValueError(f"center must have shape ({k},), got {self.center.shape}")
        eff = np.asarray(effects, dtype=np.float64)
        if eff.ndim == 1:
            eff = eff[None, :]
        if eff.ndim != 2 or eff.shape[1] != k or eff.shape[0] < 1:
            raise ValueError(f"effects must have shape (n_traits, {k}), got {eff.shape}")
        self.effects = np.ascontiguousarray(eff)
        self.intercept = np.ascontiguousarray(np.atleast_1d(np.asarray(intercept, dtype=np.float64)))
        if self.intercept.shape != (eff.shape[0],):
            raise ValueError(f"intercept must have shape ({eff.shape[0]},), got {self.intercept.shape}")
        if branch not in ("gblup", "snp"):
            raise ValueError("branch must be 'gblup' or 'snp'")
        self.h2 = float(h2)
        self.branch = branch
        self.fitness = float(fitness)
        if (cov_effects is None) != (cov_center is None):
            raise ValueError("cov_effects and cov_center are given together or not at all")
        self.cov_effects = self.cov_center = None
        if cov_effects is not None:
            ce = np.asarray(cov_effects, dtype=np.float64)
            if ce.ndim == 1:
                ce = ce[None, :]
            cc = np.ascontiguousarray(np.atleast_1d(np.asarray(cov_center, dtype=np.float64)))
            if ce.ndim != 2 or ce.shape[0] != eff.shape[0] or ce.shape[1] < 1 or cc.shape != (ce.shape[1],):
                raise ValueError(f"cov_effects must have shape ({eff.shape[0]}, c) and cov_center (c,), got "
                                 f"{ce.shape} and {cc.shape}")
            self.cov_effects, self.cov_center = np.ascontiguousarray(ce), cc
        given = [a is not None for a in (group_levels, group_effects, group_center)]
        if any(given) and not all(given):
            raise ValueError("group_levels, group_effects and group_center are given together or not at all")
        self.group_levels = self.group_effects = self.group_center = None
        if all(given):
            gl = np.asarray(group_levels)
            ge = np.asarray(group_effects, dtype=np.float64)
            if ge.ndim == 1:
                ge = ge[None, :]
            gc = np.ascontiguousarray(np.atleast_1d(np.asarray(group_center, dtype=np.float64)))
            if gl.ndim != 1 or gl.size < 1 or ge.shape != (eff.shape[0], gl.size) or gc.shape != (gl.size,):
                raise ValueError(f"group_levels must be (L,), group_effects ({eff.shape[0]}, L) and group_center (L,), "
                                 f"got {gl.shape}, {ge.shape} and {gc.shape}")
            if gl.size > 1 and not np.all(gl[1:] > gl[:-1]):
                raise ValueError("group_levels must be sorted and distinct (np.unique's order)")
            self.group_levels, self.group_effects, self.group_center = gl, np.ascontiguousarray(ge), gc

    @property
    def n_covariates(self):
        return 0 if self.cov_effects is None else self.cov_effects.shape[1]

    @property
    def n_levels(self):
        return 0 if self.group_levels is None else self.group_levels.shape[0]

    @property
    def n_traits(self):
        return self.effects.shape[0]

    def _cov_part(self, covariates, rows):
        """(Q - cov_center) cov_effects^T as (n_traits, animals)."""
        if self.cov_effects is None:
            raise ValueError("the model was fitted without covariates")
        q = np.asarray(covariates, dtype=np.float64)
        if q.ndim == 1:
            q = q[:, None]
        if q.shape != (rows, self.n_covariates):
            raise ValueError(f"covariates must have shape ({rows}, {self.n_covariates}), got {q.shape}")
        return self.cov_effects @ (q - self.cov_center).T

    def _group_part(self, groups, rows):
        """(Z - group_center) group_effects^T as (n_traits, animals); NaN for a label that is not a fitted level."""
        if self.group_levels is None:
            raise ValueError("the model was fitted without groups")
        g = np.asarray(groups)
        if g.dtype.kind == "O":
            g = g.astype(str)
        if g.shape != (rows,):
            raise ValueError(f"groups must have shape ({rows},), got {g.shape}")
        if (g.dtype.kind in "US") != (self.group_levels.dtype.kind in "US"):
            raise ValueError("groups must be labels of the kind the model was fitted with (%s)" % self.group_levels.dtype)
        at = np.minimum(np.searchsorted(self.group_levels, g), self.n_levels - 1)
        known = self.group_levels[at] == g
        out = self.group_effects[:, at] - (self.group_effects @ self.group_center)[:, None]
        out[:, ~known] = np.nan
        return out

    def _fixed_part(self, covariates, groups, rows):
        part = np.zeros((self.n_traits, rows))
        if covariates is not None:
            part = part + self._cov_part(covariates, rows)
        if groups is not None:
            part = part + self._group_part(groups, rows)
        return part

    def adjust(self, y, covariates=None, groups=None):
        """The phenotype adjusted for the fitted fixed effects, y* = y - (Q - cov_center) cov_effects
        - (Z - group_center) group_effects: y is (animals,) for one trait, else (animals, n_traits); covariates
        (animals, c) and groups (animals,) labels, each for a model fitted with it (an animal whose label is not a
        fitted level gets NaN).  Host numpy."""
        y = np.asarray(y, dtype=np.float64)
        part = self._fixed_part(covariates, groups, y.shape[0])
        if y.ndim == 1:
            if self.n_traits != 1:
                raise ValueError("y must be (animals, n_traits)")
            return y - part[0]
        if y.ndim != 2 or y.shape[1] != self.n_traits:
            raise ValueError("y must be (animals, n_traits)")
        return y - part.T

    def predict(self, genotypes, covariates=None, groups=None):
        """EBVs of the rows of an (animals x P) {0,1,2} genotype matrix: (animals,) for one trait,
        else (n_traits, animals) -- the shapes GpuBlupEngine.predict gives per model.  Host numpy.
        covariates (animals, c): the fitted fixed effects (Q - cov_center) cov_effects are added (a model
        fitted with covariates; without the argument it returns the genomic value and intercept alone).
        groups (animals,) labels: the fitted class effects (Z - group_center) group_effects are added in the same
        way; an animal whose label is not a fitted level gets NaN."""
        g = np.asarray(genotypes)
        if g.ndim != 2:
            raise ValueError("genotypes must be 2-D (animals x SNPs)")
        if int(self.indices.max()) >= g.shape[1]:
            raise IndexError(f"index {int(self.indices.max())} is out of bounds for axis 1 with size {g.shape[1]}")
        xc = g[:, self.indices].astype(np.float64) - self.center
        out = self.effects @ xc.T + self.intercept[:, None]
        if covariates is not None or groups is not None:
            out = out + self._fixed_part(covariates, groups, g.shape[0])
        return out[0] if self.n_traits == 1 else out

    def save(self, path):
        """Write the model as an .npz (numpy appends the suffix when it is missing)."""
        extra = {} if self.cov_effects is None else {"cov_effects": self.cov_effects, "cov_center": self.cov_center}
        if self.group_levels is not None:
            extra.update(group_levels=self.group_levels, group_effects=self.group_effects,
                         group_center=self.group_center)
        np.savez(path, indices=self.indices, center=self.center, effects=self.effects, intercept=self.intercept,
                 h2=np.float64(self.h2), branch=np.array(self.branch), fitness=np.float64(self.fitness), **extra)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            # (files without them: no covariates, no class factor)
            cov = {k: z[k] for k in ("cov_effects", "cov_center", "group_levels", "group_effects", "group_center")
                   if k in z.files}
            return cls(z["indices"], z["center"], z["effects"], z["intercept"], float(z["h2"]), str(z["branch"]),
                       float(z["fitness"]), **cov)


class SnpScores:
    """Mixed-model score statistics of listed SNPs against fitted panels (GpuBlupEngine.snp_scores,
    tblup_snp_score_batch; include/tblup_gpu.h has the definitions).  For B models, nt traits and
    n_cand listed SNPs:

        score (B, nt, n_cand)  u = w_j' V^-1 r_t
        info  (B, n_cand)      v = w_j' V^-1 w_j
        q     (B, nt)          r_t' V^-1 r_t
        dof   (B,)             N - r: the train animals, minus one under snp (the fitted intercept)
        snps  (n_cand,)        the listed columns, wrapped to [0, P)

    With fixed-effect covariates Q (snp_scores(covariates=), tblup_snp_score_cov_batch) the same fields hold
    the statistics adjusted for them -- u_P = w_j' P r_t, v_P = w_j' P w_j, q_P = r_t' P r_t with
    P = V^-1 - V^-1 Q~ (Q~' V^-1 Q~)^-1 Q~' V^-1, dof = N - r - c -- and `cov_effects` (B, nt, c) the GLS
    effects of the covariates in the model without the SNP (fit(covariates=)'s); it is None otherwise.
    With a class factor (snp_scores_group, tblup_snp_score_group_batch) the adjustment is for the fixed design
    [Q, Z], dof = N - r - C_m with C_m the model's column count, and `group_levels` (L,) / `group_effects` (B, nt, L)
    are fit(groups=)'s levels and level effects; both are None otherwise.

    The derived statistics are plain numpy and need neither the GPU nor the library; all three give NaN
    where v == 0 (a column that is constant over the reference rows, or in the span of the covariates)."""

    __slots__ = ("score", "info", "q", "dof", "snps", "cov_effects", "group_effects", "group_levels")

    def __init__(self, score, info, q, dof, snps, cov_effects=None, group_effects=None, group_levels=None):
        self.score = np.asarray(score, dtype=np.float64)
        self.info = np.asarray(info, dtype=np.float64)
        self.q = np.asarray(q, dtype=np.float64)
        self.dof = np.asarray(dof, dtype=np.float64)
        self.snps = np.asarray(snps, dtype=np.int64)
        self.cov_effects = None if cov_effects is None else np.asarray(cov_effects, dtype=np.float64)
        if self.score.ndim != 3:
            raise ValueError("score must have shape (models, n_traits, n_cand)")
        B, nt, m = self.score.shape
        if self.info.shape != (B, m) or self.q.shape != (B, nt) or self.dof.shape != (B,) or self.snps.shape != (m,):
            raise ValueError("info (B, n_cand), q (B, n_traits), dof (B,) and snps (n_cand,) must match score %s"
                             % (self.score.shape,))
        if self.cov_effects is not None and (self.cov_effects.ndim != 3 or self.cov_effects.shape[:2] != (B, nt)):
            raise ValueError("cov_effects must have shape (models, n_traits, n_cov)")
        self.group_effects = None if group_effects is None else np.asarray(group_effects, dtype=np.float64)
        self.group_levels = None if group_levels is None else np.asarray(group_levels)
        if (self.group_effects is None) != (self.group_levels is None):
            raise ValueError("group_effects and group_levels are given together")
        if self.group_effects is not None and self.group_effects.shape != (B, nt, len(self.group_levels)):
            raise ValueError("group_effects must have shape (models, n_traits, n_levels)")

    def _uv(self):
        v = np.where(self.info == 0, np.nan, self.info)[:, None, :]
        return self.score, v

    def effect(self):
        """u / v: the GLS effect of the SNP fitted as a covariate beside the panel, (B, nt, n_cand)."""
        u, v = self._uv()
        with np.errstate(all="ignore"):
            return u / v

    def chi2(self):
        """u^2 / (v q / dof): the score test's statistic (1 degree of freedom), (B, nt, n_cand)."""
        u, v = self._uv()
        with np.errstate(all="ignore"):
            return u * u / (v * (self.q / self.dof[:, None])[:, :, None])

    def loglik_gain(self):
        """dof / 2 * log(q / (q - u^2 / v)): the rise of the profile log-likelihood when the SNP is
        fitted as a covariate at the same h2, (B, nt, n_cand)."""
        u, v = self._uv()
        q = self.q[:, :, None]
        with np.errstate(all="ignore"):
            return self.dof[:, None, None] / 2 * np.log(q / (q - u * u / v))


class CovReliability:
    """Uncertainty under the model with fixed-effect covariates (GpuBlupEngine.reliability_cov(covariates=),
    tblup_reliability_cov_batch; include/tblup_gpu.h has the definitions).  For B models, n_pred listed animals and
    c covariates:

        reliability (B, n_pred)  1 - PEV(g^_a - g_a) / (sigma2_g K_aa) with the covariates' effects estimated
        pev_total   (B, n_pred)  error variance of (q_a - cov_center) cov_effects + g_a, in units of sigma2_g
                                 (None unless return_pev)
        cov_cov     (B, c, c)    (Q~' V^-1 Q~)^-1: Var(cov_effects[t]) = sigma2_g[t] * cov_cov (None unless
                                 return_cov_cov)
        models      B PanelModels, fit(covariates=)'s bit for bit (None unless return_models)

    No phenotype enters the first three: with several traits they are one value per (model, animal)."""

    __slots__ = ("reliability", "pev_total", "cov_cov", "models")

    def __init__(self, reliability, pev_total=None, cov_cov=None, models=None):
        self.reliability = np.asarray(reliability, dtype=np.float64)
        if self.reliability.ndim != 2:
            raise ValueError("reliability must have shape (models, n_pred)")
        B = self.reliability.shape[0]
        self.pev_total = None if pev_total is None else np.asarray(pev_total, dtype=np.float64)
        if self.pev_total is not None and self.pev_total.shape != self.reliability.shape:
            raise ValueError("pev_total must have reliability's shape %s" % (self.reliability.shape,))
        self.cov_cov = None if cov_cov is None else np.asarray(cov_cov, dtype=np.float64)
        if self.cov_cov is not None and (self.cov_cov.ndim != 3 or self.cov_cov.shape[0] != B
                                         or self.cov_cov.shape[1] != self.cov_cov.shape[2]):
            raise ValueError("cov_cov must have shape (models, c, c)")
        self.models = None if models is None else list(models)
        if self.models is not None and len(self.models) != B:
            raise ValueError("models must hold one model per row of reliability")

    def cov_stderr(self, sigma2_g):
        """sqrt(sigma2_g * diag cov_cov): the standard errors of cov_effects, (B, nt, c).  sigma2_g: (B,) for one
        trait or (B, nt), as log_likelihood_cov(return_sigma2=True) gives it at one h2.  Host numpy."""
        if self.cov_cov is None:
            raise ValueError("cov_cov was not asked for (return_cov_cov=True)")
        B = self.cov_cov.shape[0]
        s2 = np.asarray(sigma2_g, dtype=np.float64)
        if s2.ndim == 1:
            s2 = s2[:, None]
        if s2.ndim != 2 or s2.shape[0] != B:
            raise ValueError("sigma2_g must have shape (models,) or (models, n_traits), got %s" % (s2.shape,))
        diag = np.einsum("bii->bi", self.cov_cov)
        with np.errstate(invalid="ignore"):
            return np.sqrt(s2[:, :, None] * diag[:, None, :])


class GroupReliability:
    """Uncertainty under the model with a class fixed effect (GpuBlupEngine.reliability_group(groups=),
    tblup_reliability_group_batch; include/tblup_gpu.h has the definitions).  For B models, n_pred listed animals,
    c covariates and L levels:

        reliability  (B, n_pred)         1 - PEV(g^_a - g_a) / (sigma2_g K_aa) with the covariates' and the levels'
                                         effects estimated
        pev_total    (B, n_pred)         error variance of a predicted record of the animal in its own level, in
                                         units of sigma2_g; NaN for an animal whose label is not a fitted level (None
                                         unless return_pev)
        fixed_cov    (B, c + L, c + L)   (F~' V^-1 F~)^-1, covariates then levels: Var of [cov_effects[t],
                                         group_effects[t]] = sigma2_g[t] * fixed_cov; under snp the reference level's
                                         row and column are zero (None unless return_fixed_cov)
        models       B PanelModels, fit(groups=)'s bit for bit (None unless return_models)
        group_levels (L,)                the fitted levels, np.unique of the train rows' labels
        n_cov        c

    No phenotype enters the first three: with several traits they are one value per (model, animal)."""

    __slots__ = ("reliability", "pev_total", "fixed_cov", "models", "group_levels", "n_cov")

    def __init__(self, reliability, group_levels, n_cov=0, pev_total=None, fixed_cov=None, models=None):
        self.reliability = np.asarray(reliability, dtype=np.float64)
        if self.reliability.ndim != 2:
            raise ValueError("reliability must have shape (models, n_pred)")
        B = self.reliability.shape[0]
        self.group_levels = np.asarray(group_levels)
        if self.group_levels.ndim != 1 or self.group_levels.size < 1:
            raise ValueError("group_levels must be a non-empty 1-D array")
        self.n_cov = int(n_cov)
        if self.n_cov < 0:
            raise ValueError("n_cov must not be negative")
        C = self.n_cov + self.group_levels.size
        self.pev_total = None if pev_total is None else np.asarray(pev_total, dtype=np.float64)
        if self.pev_total is not None and self.pev_total.shape != self.reliability.shape:
            raise ValueError("pev_total must have reliability's shape %s" % (self.reliability.shape,))
        self.fixed_cov = None if fixed_cov is None else np.asarray(fixed_cov, dtype=np.float64)
        if self.fixed_cov is not None and self.fixed_cov.shape != (B, C, C):
            raise ValueError("fixed_cov must have shape (models, n_cov + levels, n_cov + levels) = %s"
                             % ((B, C, C),))
        self.models = None if models is None else list(models)
        if self.models is not None and len(self.models) != B:
            raise ValueError("models must hold one model per row of reliability")

    def _stderr(self, sigma2_g, lo, hi):
        if self.fixed_cov is None:
            raise ValueError("fixed_cov was not asked for (return_fixed_cov=True)")
        B = self.fixed_cov.shape[0]
        s2 = np.asarray(sigma2_g, dtype=np.float64)
        if s2.ndim == 1:
            s2 = s2[:, None]
        if s2.ndim != 2 or s2.shape[0] != B:
            raise ValueError("sigma2_g must have shape (models,) or (models, n_traits), got %s" % (s2.shape,))
        diag = np.einsum("bii->bi", self.fixed_cov)[:, lo:hi]
        with np.errstate(invalid="ignore"):
            return np.sqrt(s2[:, :, None] * diag[:, None, :])

    def cov_stderr(self, sigma2_g):
        """sqrt(sigma2_g * diag fixed_cov) over the covariates: the standard errors of cov_effects, (B, nt, c).
        sigma2_g: (B,) for one trait or (B, nt), as log_likelihood_group(return_sigma2=True) gives it at one h2.
        Host numpy."""
        return self._stderr(sigma2_g, 0, self.n_cov)

    def group_stderr(self, sigma2_g):
        """The same over the levels: the standard errors of group_effects, (B, nt, L) -- 0 at the reference level
        under snp, whose effect is 0 by construction (the others are then errors of contrasts with it)."""
        return self._stderr(sigma2_g, self.n_cov, self.n_cov + self.group_levels.size)


class LooResult:
    """Leave-one-out cross-validation of fitted models (GpuBlupEngine.loo, tblup_loo_batch; include/tblup_gpu.h has
    the definitions).  For B models, n_T training animals in `train` order and t traits:

        fitness      (B,)                   |pearson(pred, y_T)|, the mean over traits for several traits
        pred         (B, n_T) / (B, t, n_T) every training animal predicted by the model fitted without it
        press        (B,) / (B, t)          sum over the animals of (y_T - pred)^2
        leverage     (B, n_T)               h_tt, the diagonal of the smoother (None unless return_leverage); no
                                            phenotype enters: one value per (model, animal) for any number of traits
        eval_fitness (B,)                   the same pass's validation fitness, evaluate()'s bit for bit
        train        (n_T,)                 the animals' row ids, the order of pred's and leverage's last axis"""

    __slots__ = ("fitness", "pred", "press", "leverage", "eval_fitness", "train")

    def __init__(self, fitness, pred, press, leverage, eval_fitness, train):
        self.fitness = np.asarray(fitness, dtype=np.float64)
        self.pred = np.asarray(pred, dtype=np.float64)
        self.train = np.asarray(train, dtype=np.int64)
        if self.fitness.ndim != 1 or self.train.ndim != 1:
            raise ValueError("fitness must have shape (models,) and train (n_train,)")
        B, nT = self.fitness.shape[0], self.train.shape[0]
        if self.pred.ndim not in (2, 3) or self.pred.shape[0] != B or self.pred.shape[-1] != nT:
            raise ValueError("pred must have shape (models, n_train) or (models, n_traits, n_train)")
        self.press = np.asarray(press, dtype=np.float64)
        if self.press.shape != self.pred.shape[:-1]:
            raise ValueError("press must have shape %s" % (self.pred.shape[:-1],))
        self.leverage = None if leverage is None else np.asarray(leverage, dtype=np.float64)
        if self.leverage is not None and self.leverage.shape != (B, nT):
            raise ValueError("leverage must have shape (models, n_train)")
        self.eval_fitness = np.asarray(eval_fitness, dtype=np.float64)
        if self.eval_fitness.shape != (B,):
            raise ValueError("eval_fitness must have shape (models,)")

    def residuals(self, y):
        """y_T - pred, the leave-one-out errors, in pred's shape.  y: the phenotypes of every animal of the panel,
        (n,) or (n, t) as the engine took them.  Host numpy."""
        y = np.asarray(y, dtype=np.float64)
        if y.ndim == 2 and y.shape[1] == 1:
            y = y[:, 0]
        yT = y[self.train]
        if self.pred.ndim == 2:
            if yT.ndim != 1:
                raise ValueError("one trait was fitted: y must be (n,)")
            return yT[None, :] - self.pred
        if yT.ndim != 2 or yT.shape[1] != self.pred.shape[1]:
            raise ValueError("y must be (n, %d)" % self.pred.shape[1])
        return yT.T[None, :, :] - self.pred
