"""PanelModel: the fitted model of one selected SNP panel, as a breeder deploys it.

The reference ends a blup() call with |pearson| and drops what it fitted on the way
(tblup/evaluator.py:284-286, 311-314).  `GpuBlupEngine.fit` / `tblup_fit_batch` return it: for the
selected columns idx[0..k) (duplicates kept, each occurrence its own column, as
data[:, indices]),

    EBV_t(a) = intercept[t] + sum_j (x[a, idx_j] - center[j]) * effects[t][j]

`predict` below is that formula in plain numpy, so a saved model needs neither the GPU nor the
library to be applied to a genotype matrix.
"""
import numpy as np


class PanelModel:
    """indices (k,) wrapped to [0, P); center (k,) = 2p of each column over the branch's reference
    rows; effects (nt, k); intercept (nt,); h2, branch ("gblup" / "snp": the branch that was fitted)
    and the fit's validation fitness."""

    __slots__ = ("indices", "center", "effects", "intercept", "h2", "branch", "fitness")

    def __init__(self, indices, center, effects, intercept, h2=float("nan"), branch="snp", fitness=float("nan")):
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

    @property
    def n_traits(self):
        return self.effects.shape[0]

    def predict(self, genotypes):
        """EBVs of the rows of an (animals x P) {0,1,2} genotype matrix: (animals,) for one trait,
        else (n_traits, animals) -- the shapes GpuBlupEngine.predict gives per model.  Host numpy."""
        g = np.asarray(genotypes)
        if g.ndim != 2:
            raise ValueError("genotypes must be 2-D (animals x SNPs)")
        if int(self.indices.max()) >= g.shape[1]:
            raise IndexError(f"index {int(self.indices.max())} is out of bounds for axis 1 with size {g.shape[1]}")
        xc = g[:, self.indices].astype(np.float64) - self.center
        out = self.effects @ xc.T + self.intercept[:, None]
        return out[0] if self.n_traits == 1 else out

    def save(self, path):
        """Write the model as an .npz (numpy appends the suffix when it is missing)."""
        np.savez(path, indices=self.indices, center=self.center, effects=self.effects, intercept=self.intercept,
                 h2=np.float64(self.h2), branch=np.array(self.branch), fitness=np.float64(self.fitness))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["indices"], z["center"], z["effects"], z["intercept"], float(z["h2"]), str(z["branch"]),
                       float(z["fitness"]))


class SnpScores:
    """Mixed-model score statistics of listed SNPs against fitted panels (GpuBlupEngine.snp_scores,
    tblup_snp_score_batch; include/tblup_gpu.h has the definitions).  For B models, nt traits and
    n_cand listed SNPs:

        score (B, nt, n_cand)  u = w_j' V^-1 r_t
        info  (B, n_cand)      v = w_j' V^-1 w_j
        q     (B, nt)          r_t' V^-1 r_t
        dof   (B,)             N - r: the train animals, minus one under snp (the fitted intercept)
        snps  (n_cand,)        the listed columns, wrapped to [0, P)

    The derived statistics are plain numpy and need neither the GPU nor the library; all three give NaN
    where v == 0 (a column that is constant over the reference rows)."""

    __slots__ = ("score", "info", "q", "dof", "snps")

    def __init__(self, score, info, q, dof, snps):
        self.score = np.asarray(score, dtype=np.float64)
        self.info = np.asarray(info, dtype=np.float64)
        self.q = np.asarray(q, dtype=np.float64)
        self.dof = np.asarray(dof, dtype=np.float64)
        self.snps = np.asarray(snps, dtype=np.int64)
        if self.score.ndim != 3:
            raise ValueError("score must have shape (models, n_traits, n_cand)")
        B, nt, m = self.score.shape
        if self.info.shape != (B, m) or self.q.shape != (B, nt) or self.dof.shape != (B,) or self.snps.shape != (m,):
            raise ValueError("info (B, n_cand), q (B, n_traits), dof (B,) and snps (n_cand,) must match score %s"
                             % (self.score.shape,))

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
