"""GpuBlupEngine: one MI355X context holding the genotype panel in HBM.

This is the compute leg that replaces the reference's worker pool
(tblup/evaluator.py:205-241): instead of pickling one `blup` job per
individual onto an mp.Queue, a whole batch of selected-index sets goes to
`tblup_eval_batch` in one call.  Splits (train/validation animal lists) are
registered once and cached by content, so InterGCV folds, the testing split
and Monte-Carlo splits each pay the split build only when they change.
"""
import ctypes
import hashlib
from collections import OrderedDict

import numpy as np

from . import _native
from ._native import ptr as _ptr


def _as_int64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64))


def validate_genotypes(data):
    """The GPU path stores genotypes as int8 {0,1,2} (SURVEY.md section 8a data contract).

    Raises ValueError for anything else (e.g. imputed dosages), instead of
    silently changing the arithmetic.
    """
    from .panel import convert_rows
    g = data if isinstance(data, np.ndarray) else np.asarray(data)
    if g.ndim != 2:
        raise ValueError("genotype matrix must be 2-D (animals x SNPs)")
    if g.dtype == np.int8:
        if g.size and (int(g.min()) < 0 or int(g.max()) > 2):
            raise ValueError("genotypes must take values in {0, 1, 2} for the MI355X evaluator")
        return np.ascontiguousarray(g)
    # converted by blocks of rows (tblup_amd.panel): no full-size boolean or float temporaries
    return convert_rows(g)


def concat_genomes(genomes):
    """Concatenate ragged index arrays -> (idx int64, offsets int64[B+1])."""
    lens = np.fromiter((len(g) for g in genomes), dtype=np.int64, count=len(genomes))
    offsets = np.zeros(len(genomes) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    if len(genomes):
        idx = np.concatenate([np.asarray(g, dtype=np.int64).ravel() for g in genomes])
    else:
        idx = np.zeros(0, dtype=np.int64)
    return np.ascontiguousarray(idx), offsets


class GpuBlupEngine:
    """Genotypes + phenotypes resident on one GPU; batched BLUP fitness."""

    MAX_SPLITS = 16   # a cached split is ~100 MB at config 2; IntraGCV holds k of them

    def __init__(self, data, labels, device=0, snp_major=False):
        """labels: (n,) phenotypes, or (n, t) for multi-trait evaluation (t <= 4, BASELINE
        config 5): one Cholesky per individual serves every trait, fitness = mean |r|."""
        self._lib = _native.load()
        geno = validate_genotypes(data)
        labels = np.asarray(labels, dtype=np.float64)
        if labels.ndim == 2 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if labels.ndim not in (1, 2) or (labels.ndim == 2 and not 1 <= labels.shape[1] <= _native.MAX_TRAITS):
            raise ValueError(f"phenotypes must be (n,) or (n, t) with t <= {_native.MAX_TRAITS}")
        self.n_traits = 1 if labels.ndim == 1 else labels.shape[1]
        pheno = np.ascontiguousarray(labels[:, 0] if labels.ndim == 2 else labels)
        if snp_major:
            n_snps, n = geno.shape
            layout = _native.LAYOUT_SNP_MAJOR
        else:
            n, n_snps = geno.shape
            layout = _native.LAYOUT_ANIMAL_MAJOR
        if pheno.shape[0] != n:
            raise ValueError(f"phenotype length {pheno.shape[0]} != number of animals {n}")
        self.n_animals, self.n_snps, self.device = n, n_snps, int(device)
        ctx = ctypes.c_void_p()
        _native.check("tblup_ctx_create", self._lib.tblup_ctx_create(
            geno.ctypes.data_as(ctypes.c_void_p), n, n_snps, layout, _ptr(pheno), self.device, ctypes.byref(ctx)))
        self._ctx = ctx
        if self.n_traits > 1:
            mt = np.ascontiguousarray(labels)
            _native.check("tblup_set_traits", self._lib.tblup_set_traits(
                self._ctx, _ptr(mt), self.n_traits))
        self._splits = OrderedDict()   # key -> (split_id, n_valid)
        self._next_split = 0
        self._pending = None           # (event, keep-alive) of asynchronous work using the workspace
        self._spec_stream = None

    def _settle(self):
        """Wait for asynchronous work (eval_keys_async) that uses the context's workspace; every
        other entry point (the device-pointer ones included) calls this first, so calls stay
        serialised on the context whatever stream they are enqueued on."""
        p = self._pending
        if p is not None:
            self._pending = None
            p[0].synchronize()

    # ------------------------------------------------------------------ splits
    def split_id(self, train, valid, pinned=()):
        """Device id of the (train, valid) split, registered on first use; the cache keeps the
        MAX_SPLITS most recently used splits, never evicting the keys in `pinned` (the other
        splits of the same call: evaluate_folds)."""
        self._settle()
        t = _as_int64(train)
        v = _as_int64(valid)
        key = self._split_key(t, v)
        hit = self._splits.get(key)
        if hit is not None:
            self._splits.move_to_end(key)
            return hit[0]
        while len(self._splits) >= self.MAX_SPLITS:
            victim = next((k for k in self._splits if k not in pinned), None)
            if victim is None:   # every cached split belongs to this call: let the cache grow
                break
            old_id, _ = self._splits.pop(victim)
            _native.check("tblup_drop_split", self._lib.tblup_drop_split(self._ctx, old_id))
        sid = self._next_split
        self._next_split += 1
        _native.check("tblup_set_split", self._lib.tblup_set_split(
            self._ctx, sid, _ptr(t), len(t), _ptr(v), len(v)))
        self._splits[key] = (sid, len(v))
        return sid

    @staticmethod
    def _split_key(train, valid):
        return hashlib.sha1(_as_int64(train).tobytes() + b"|" + _as_int64(valid).tobytes()).hexdigest()

    def split_ids(self, splits):
        """split_id for every (train, valid) pair of one call; none of them evicts another, however
        many there are (the cache shrinks back to MAX_SPLITS on later registrations)."""
        pinned = {self._split_key(t, v) for t, v in splits}
        return [self.split_id(t, v, pinned) for t, v in splits]

    # -------------------------------------------------------------- evaluation
    def evaluate(self, genomes, train, valid, h2, branch="auto", return_ebv=False, groups=None):
        """Fitness |pearson(EBV_V, y_V)| for each selected-index set (evaluator.py:244-314);
        multi-trait: the mean over traits, EBVs (B, t, n_valid)."""
        self._no_groups(groups, "evaluate()")
        self._settle()
        sid = self.split_id(train, valid)
        idx, offsets = concat_genomes(genomes)
        B = len(genomes)
        fit = np.empty(B, dtype=np.float64)
        n_valid = len(valid)
        shape = (B, n_valid) if self.n_traits == 1 else (B, self.n_traits, n_valid)
        ebv = np.empty(shape, dtype=np.float64) if return_ebv else None
        if B:
            _native.check("tblup_eval_batch", self._lib.tblup_eval_batch(
                self._ctx, sid, _ptr(idx), _ptr(offsets), B, float(h2), _native.BRANCH[branch], _ptr(fit),
                _ptr(ebv) if return_ebv else None))
        return (fit, ebv) if return_ebv else fit

    # ------------------------------------------------------- taking the model out
    def fit(self, genomes, train, valid, h2, branch="auto", reliability_of=None, covariates=None, return_ebv=False,
            groups=None):
        """evaluate() plus what it fitted: one PanelModel per selected-index set (tblup_fit_batch),
        whose `fitness` is evaluate()'s value bit for bit.  Out-of-range indices raise
        TblupIndexError; a degenerate panel gives NaN effects, not an error.
        reliability_of: a list of animals (row ids of the panel) -- the return value is then
        (models, reliabilities) from one pass (tblup_reliability_batch), the models bit-identical to
        fit()'s and the (len(genomes), len(animals)) array to reliability()'s.
        covariates: an (n_animals, c) float matrix Q of fixed-effect covariates, 1 <= c <= 16, one row per
        animal of the panel (a 1-D array is one column) -- they are fitted beside the genomic effects by
        GLS (tblup_fit_cov_batch; include/tblup_gpu.h has the model) and every model carries `cov_effects`
        (nt, c) and `cov_center` (c,): the column means over the train rows under snp, zero under gblup,
        where a mean is fitted only by a column of ones.  The models' effects, intercept and `fitness` are
        then those of the adjusted phenotype y* = y - (Q - cov_center) cov_effects (PanelModel.adjust);
        return_ebv=True also returns the validation EBVs of y*, (B, n_valid) or (B, nt, n_valid), as
        (models, ebv).  Collinear covariates give a NaN model, not an error; NaN / Inf in Q is a ValueError.
        Not combined with reliability_of: reliability_cov(covariates=Q, return_models=True) gives the reliabilities
        under the covariate model and these models from one pass.
        groups: an (n_animals,) array of integer or string labels of one class factor (herd, batch, pen ..), with
        or without covariates -- its levels, np.unique of the train rows' labels, are fitted as fixed effects
        beside them (tblup_fit_group_batch; include/tblup_gpu.h has the model).  Under gblup every level has a
        column and the level effects are the model's group means (a column of ones in Q is then collinear: a NaN
        model); under snp the columns are centred, the lowest level is the reference with effect 0 and the
        intercept stays mean(y_T).  A model has at most 128 columns, covariates and levels together (one level
        less under snp).  Every model carries `group_levels` (L,), `group_effects` (nt, L) and `group_center`
        (L,), and y* = PanelModel.adjust(y, covariates, groups).  A validation animal whose label no train animal
        has is a ValueError that names the label; elsewhere such an animal is simply not used.  The h2 of this
        model is estimate_h2_group()'s; snp_scores_group() tests SNPs against it.  Not combined with
        reliability_of: reliability_group(groups=, return_models=True) gives the reliabilities under this model and
        these models from one pass."""
        self._settle()
        if groups is not None:
            if reliability_of is not None:
                raise ValueError("reliability_of is not supported together with groups: "
                                 "reliability_group(return_models=True) gives both from one pass")
            return self._fit_group(genomes, train, valid, h2, branch, covariates, groups, return_ebv)
        if covariates is not None:
            if reliability_of is not None:
                raise ValueError("reliability_of is not supported together with covariates")
            return self._fit_cov(genomes, train, valid, h2, branch, covariates, return_ebv)
        if return_ebv:
            raise ValueError("return_ebv needs covariates (evaluate(return_ebv=True) gives the plain model's EBVs)")
        an = None
        if reliability_of is not None:
            an = _as_int64(reliability_of)
            if an.ndim != 1:
                raise ValueError("reliability_of must be a 1-D list of row ids")
        B = len(genomes)
        rel = None if an is None else np.empty((B, len(an)), dtype=np.float64)
        if an is not None and len(an):
            def call(sid, idx, offsets, *outs):
                _native.check("tblup_reliability_batch", self._lib.tblup_reliability_batch(
                    self._ctx, sid, _ptr(an), len(an), idx, offsets, B, float(h2), _native.BRANCH[branch], *outs,
                    _ptr(rel)))
        else:
            def call(sid, idx, offsets, *outs):
                _native.check("tblup_fit_batch", self._lib.tblup_fit_batch(
                    self._ctx, sid, idx, offsets, B, float(h2), _native.BRANCH[branch], *outs))
        models = self._fit_models(genomes, train, valid, h2, branch, call)
        return models if an is None else (models, rel)

    def _fitted_branch(self, k, branch):
        """The branch a model of k SNPs is fitted under (evaluator.py:257)."""
        return branch if branch != "auto" else ("gblup" if k > self.n_animals else "snp")

    def _fit_models(self, genomes, train, valid, h2, branch, call, **cov):
        """The fitted-model entries' frame: the outputs allocated, call(sid, idx, offsets, fitness, intercept,
        center, effects) made for a non-empty batch (all but sid as pointers), one PanelModel per index set.
        cov: the cov_effects / cov_center arrays that the call fills, a row per model."""
        from .model import PanelModel
        sid = self.split_id(train, valid)
        idx, offsets = concat_genomes(genomes)
        B, nt, total = len(genomes), self.n_traits, int(offsets[-1])
        fit, intercept = np.empty(B, dtype=np.float64), np.empty((B, nt), dtype=np.float64)
        center, effects = np.empty(total, dtype=np.float64), np.empty((nt, total), dtype=np.float64)
        if B:
            call(sid, *map(_ptr, (idx, offsets, fit, intercept, center, effects)))
        wrapped = np.where(idx < 0, idx + self.n_snps, idx)
        models = []
        for b in range(B):
            lo, hi = int(offsets[b]), int(offsets[b + 1])
            models.append(PanelModel(wrapped[lo:hi], center[lo:hi], effects[:, lo:hi], intercept[b], h2,
                                     self._fitted_branch(hi - lo, branch), fit[b], **{k: v[b] for k, v in cov.items()}))
        return models

    def _covariates(self, covariates):
        """The (n_animals, c) float64 matrix of a `covariates` argument, validated."""
        q = np.asarray(covariates, dtype=np.float64)
        if q.ndim == 1:
            q = q[:, None]
        if q.ndim != 2 or q.shape[0] != self.n_animals:
            raise ValueError(f"covariates must have one row per animal ({self.n_animals}), got shape {q.shape}")
        if not 1 <= q.shape[1] <= _native.MAX_COV:
            raise ValueError(f"need 1 <= covariates <= {_native.MAX_COV}, got {q.shape[1]}")
        if not np.all(np.isfinite(q)):
            raise ValueError("covariates must be finite")
        return np.ascontiguousarray(q)

    def _fit_cov(self, genomes, train, valid, h2, branch, covariates, return_ebv):
        q = self._covariates(covariates)
        B, nt, nc, n_valid = len(genomes), self.n_traits, q.shape[1], len(valid)
        cov_eff = np.empty((B, nt, nc), dtype=np.float64)
        cov_cen = np.empty((B, nc), dtype=np.float64)
        ebv = np.empty((B, n_valid) if nt == 1 else (B, nt, n_valid), dtype=np.float64) if return_ebv else None

        def call(sid, idx, offsets, fit, *model):
            _native.check("tblup_fit_cov_batch", self._lib.tblup_fit_cov_batch(
                self._ctx, sid, _ptr(q), nc, idx, offsets, B, float(h2), _native.BRANCH[branch], fit,
                _ptr(ebv) if return_ebv else None, _ptr(cov_eff), _ptr(cov_cen), *model))
        models = self._fit_models(genomes, train, valid, h2, branch, call, cov_effects=cov_eff, cov_center=cov_cen)
        return (models, ebv) if return_ebv else models

    _GROUP_FORMS = {"snp_scores()": "snp_scores_group()", "log_likelihood_cov()": "log_likelihood_group()",
                    "estimate_h2_cov()": "estimate_h2_group()", "reliability_cov()": "reliability_group()"}

    @classmethod
    def _no_groups(cls, groups, what):
        if groups is not None:
            own = cls._GROUP_FORMS.get(what)
            raise ValueError(f"{what} does not take groups: " + (f"the class factor's form is {own}" if own else
                             "the class factor is known to fit(groups=), snp_scores_group(), log_likelihood_group(), "
                             "estimate_h2_group() and reliability_group() only"))

    def _groups(self, groups, train, valid):
        """(levels, codes) of a `groups` argument: the sorted distinct labels of the train rows and every
        animal's level code as int64, -1 for a label that is not among them."""
        g = np.asarray(groups)
        if g.dtype.kind == "O":
            g = g.astype(str)
        if g.ndim != 1 or g.shape[0] != self.n_animals:
            raise ValueError(f"groups must have one label per animal ({self.n_animals}), got shape {g.shape}")
        if g.dtype.kind not in "iuUS":
            raise ValueError(f"groups must be integer or string labels, got dtype {g.dtype}")
        T, V = _as_int64(train), _as_int64(valid)
        levels = np.unique(g[T])
        if not len(levels):
            raise ValueError("groups needs at least one train animal")
        at = np.minimum(np.searchsorted(levels, g), len(levels) - 1)
        codes = np.where(levels[at] == g, at, -1).astype(np.int64)
        unseen = codes[V] < 0
        if np.any(unseen):
            raise ValueError("validation animal %d has the label %r, which no train animal has"
                             % (int(V[unseen][0]), g[V][unseen][0].item()))
        return levels, np.ascontiguousarray(codes)

    def _group_design(self, genomes, train, valid, branch, covariates, groups):
        """(levels, codes, Q or None, columns (B,)) of a class-factor call, validated: _groups' labels, the
        covariates and every model's column count (covariates + levels, one less under snp) against the limit."""
        levels, codes = self._groups(groups, train, valid)
        q = None if covariates is None else self._covariates(covariates)
        nc, L = 0 if q is None else q.shape[1], len(levels)
        cols = np.array([nc + L - (self._fitted_branch(len(g), branch) == "snp") for g in genomes], dtype=np.int64)
        if len(cols) and cols.max() > _native.MAX_FIXED:
            raise ValueError(f"a model would have {cols.max()} fixed columns ({nc} covariates, {L} levels); the limit "
                             f"is {_native.MAX_FIXED}")
        return levels, codes, q, cols

    def _fit_group(self, genomes, train, valid, h2, branch, covariates, groups, return_ebv):
        levels, codes, q, _ = self._group_design(genomes, train, valid, branch, covariates, groups)
        B, nt, nc, L, n_valid = len(genomes), self.n_traits, 0 if q is None else q.shape[1], len(levels), len(valid)
        cov_eff = np.empty((B, nt, nc), dtype=np.float64)
        cov_cen = np.empty((B, nc), dtype=np.float64)
        grp_eff = np.empty((B, nt, L), dtype=np.float64)
        grp_cen = np.empty((B, L), dtype=np.float64)
        ebv = np.empty((B, n_valid) if nt == 1 else (B, nt, n_valid), dtype=np.float64) if return_ebv else None

        def call(sid, idx, offsets, fit, *model):
            _native.check("tblup_fit_group_batch", self._lib.tblup_fit_group_batch(
                self._ctx, sid, _ptr(q) if nc else None, nc, _ptr(codes), L, idx, offsets, B, float(h2),
                _native.BRANCH[branch], fit, _ptr(ebv) if return_ebv else None, _ptr(cov_eff) if nc else None,
                _ptr(cov_cen) if nc else None, _ptr(grp_eff), _ptr(grp_cen), *model))
        extra = dict(group_levels=np.broadcast_to(levels, (B, L)), group_effects=grp_eff, group_center=grp_cen)
        if nc:
            extra.update(cov_effects=cov_eff, cov_center=cov_cen)
        models = self._fit_models(genomes, train, valid, h2, branch, call, **extra)
        return (models, ebv) if return_ebv else models

    def reliability(self, genomes, train, valid, h2, animals, branch="auto"):
        """Reliability (squared accuracy, 1 - PEV / (sigma_g^2 K_aa)) of the genomic value of each of
        `animals` (row ids of this engine's panel: any order, repeats allowed, any or no split role)
        under the model each selected-index set fits on (train, valid): an ndarray
        (len(genomes), len(animals)) from tblup_reliability_batch (include/tblup_gpu.h has the
        definition).  It needs no phenotype: with several traits it is still one number per (model,
        animal).  The snp branch's intercept is taken as known.  The factor behind it is not kept, so
        candidates must be rows of this engine's panel.  A degenerate panel gives NaN; an animal's
        value does not depend on the list it comes in.  With fixed-effect covariates: reliability_cov."""
        self._settle()
        an = _as_int64(animals)
        if an.ndim != 1:
            raise ValueError("animals must be a 1-D list of row ids")
        sid = self.split_id(train, valid)
        idx, offsets = concat_genomes(genomes)
        B = len(genomes)
        rel = np.empty((B, len(an)), dtype=np.float64)
        if B and len(an):
            _native.check("tblup_reliability_batch", self._lib.tblup_reliability_batch(
                self._ctx, sid, _ptr(an), len(an), _ptr(idx), _ptr(offsets), B, float(h2), _native.BRANCH[branch], None,
                None, None, None, _ptr(rel)))
        return rel

    def loo(self, genomes, train, valid, h2, branch="auto", return_leverage=False, covariates=None, groups=None):
        """Leave-one-out cross-validation of the model each selected-index set fits on (train, valid): every
        training animal predicted by the model fitted without it, in closed form from the factor one evaluation
        leaves behind (tblup_loo_batch; include/tblup_gpu.h has the definitions) -- the k -> n_T limit of IntraGCV
        at the cost of one pass.  Returns a tblup_amd.model.LooResult: `fitness` (B,) = |pearson(pred, y_T)| (the
        mean over traits), `pred` (B, n_T) or (B, t, n_T) in `train` order, `press`, `eval_fitness` (evaluate()'s
        value bit for bit) and, with return_leverage, `leverage` (B, n_T), the h_tt that mark influential records.
        gblup branch: pred is the reference's gblup prediction of animal t from a model trained on T without t.
        snp branch: ridge regression with the fitted model's own penalty lambda d kept -- d and the centre come from
        the full training set, the intercept and the centring are refitted without t.  That is not the reference
        pipeline re-run with t removed, which would also change p and d.  A degenerate panel gives NaN; an
        animal's values do not depend on the batch.  The closed form loses digits as 1 / (1 - h_tt), so towards
        h2 = 1.  LOO under fixed effects (covariates=, groups=) is not built: ValueError."""
        if covariates is not None or groups is not None:
            raise ValueError("LOO under fixed effects (covariates= / groups=) is not built: loo() cross-validates the "
                             "plain model only")
        from .model import LooResult
        self._settle()
        T = _as_int64(train)
        sid = self.split_id(T, valid)
        idx, offsets = concat_genomes(genomes)
        B, nt, nT = len(genomes), self.n_traits, len(T)
        fit, efit = np.empty(B, dtype=np.float64), np.empty(B, dtype=np.float64)
        pred = np.empty((B, nt, nT), dtype=np.float64)
        press = np.empty((B, nt), dtype=np.float64)
        lev = np.empty((B, nT), dtype=np.float64) if return_leverage else None
        if B:
            _native.check("tblup_loo_batch", self._lib.tblup_loo_batch(
                self._ctx, sid, _ptr(idx), _ptr(offsets), B, float(h2), _native.BRANCH[branch], _ptr(fit), _ptr(pred),
                _ptr(lev) if return_leverage else None, _ptr(press), _ptr(efit)))
        if nt == 1:
            pred, press = pred[:, 0, :], press[:, 0]
        return LooResult(fit, pred, press, lev, efit, T)

    def reliability_cov(self, genomes, train, valid, h2, animals, covariates, branch="auto", return_pev=False,
                        return_cov_cov=False, return_models=False, groups=None):
        """reliability() under the model with fixed-effect covariates that fit(covariates=) fits (a method of
        its own, as log_likelihood_cov and estimate_h2_cov are: reliability()'s parameters stay what they were).
        covariates: an (n_animals, c) matrix Q as fit(covariates=) takes it.  Returns a
        tblup_amd.model.CovReliability from tblup_reliability_cov_batch (include/tblup_gpu.h has the
        definitions): `reliability` (B, n_pred) with the covariates' effects estimated, not known (never above
        the plain value); with return_pev `pev_total` (B, n_pred), the error variance of the predicted value
        (q_a - cov_center) cov_effects + g_a in units of sigma2_g; with return_cov_cov `cov_cov` (B, c, c) =
        (Q~' V^-1 Q~)^-1, whose cov_stderr(sigma2_g) gives the standard errors of cov_effects (sigma2_g from
        log_likelihood_cov(return_sigma2=True)); with return_models `models`, bit-identical to
        fit(covariates=Q)'s, from the same pass.  Collinear covariates give NaN for the model, K_aa = 0 NaN for
        the animal; NaN / Inf in Q is a ValueError."""
        self._no_groups(groups, "reliability_cov()")
        self._settle()
        an = _as_int64(animals)
        if an.ndim != 1:
            raise ValueError("animals must be a 1-D list of row ids")
        want_pev, want_cc, want_models = bool(return_pev), bool(return_cov_cov), bool(return_models)
        from .model import CovReliability
        q = self._covariates(covariates)
        B, nt, nc, m = len(genomes), self.n_traits, q.shape[1], len(an)
        rel = np.empty((B, m), dtype=np.float64)
        pev = np.empty((B, m), dtype=np.float64) if want_pev else None
        cc = np.empty((B, nc, nc), dtype=np.float64) if want_cc else None
        outs = (_ptr(an) if m else None, m), (_ptr(rel), _ptr(pev) if want_pev else None, _ptr(cc) if want_cc else None)

        def entry(sid, idx, offsets, *model):
            _native.check("tblup_reliability_cov_batch", self._lib.tblup_reliability_cov_batch(
                self._ctx, sid, _ptr(q), nc, *outs[0], idx, offsets, B, float(h2), _native.BRANCH[branch], *model,
                *outs[1]))
        models = None
        if want_models:
            cov_eff = np.empty((B, nt, nc), dtype=np.float64)
            cov_cen = np.empty((B, nc), dtype=np.float64)

            def call(sid, idx, offsets, fit, *model):
                entry(sid, idx, offsets, fit, _ptr(cov_eff), _ptr(cov_cen), *model)
            models = self._fit_models(genomes, train, valid, h2, branch, call, cov_effects=cov_eff, cov_center=cov_cen)
        elif B:
            idx, offsets = concat_genomes(genomes)
            entry(self.split_id(train, valid), _ptr(idx), _ptr(offsets), None, None, None, None, None, None)
        return CovReliability(rel, pev, cc, models)

    def reliability_group(self, genomes, train, valid, h2, animals, groups, covariates=None, branch="auto",
                          return_pev=False, return_fixed_cov=False, return_models=False):
        """reliability() under the model with a class fixed effect that fit(groups=) fits (a method of its own, as
        snp_scores_group and log_likelihood_group are: reliability_cov(groups=) keeps raising).  groups and the
        optional covariates are fit()'s: (n_animals,) integer or string labels of one factor, an (n_animals, c) matrix
        Q.  Returns a tblup_amd.model.GroupReliability from tblup_reliability_group_batch (include/tblup_gpu.h has the
        definitions): `reliability` (B, n_pred) with the level effects (and the covariates') estimated, not known --
        never above reliability_cov's on Q alone; with return_pev
        `pev_total` (B, n_pred), the error variance of a predicted record of the animal in its own level in units of
        sigma2_g; with return_fixed_cov `fixed_cov` (B, c + L, c + L) = (F~' V^-1 F~)^-1, covariates then levels, whose
        cov_stderr(sigma2_g) / group_stderr(sigma2_g) give the standard errors of cov_effects / group_effects
        (sigma2_g from log_likelihood_group(return_sigma2=True)); with return_models `models`, bit-identical to
        fit(groups=)'s, from the same pass.  A listed animal whose label no train animal has keeps its reliability
        and gets a NaN pev_total (PanelModel.predict's rule); on a validation row such a label stays a ValueError.
        A design that is collinear over the train rows gives NaN for the model, K_aa = 0 NaN for the animal."""
        self._settle()
        an = _as_int64(animals)
        if an.ndim != 1:
            raise ValueError("animals must be a 1-D list of row ids")
        want_pev, want_fc, want_models = bool(return_pev), bool(return_fixed_cov), bool(return_models)
        from .model import GroupReliability
        levels, codes, q, _ = self._group_design(genomes, train, valid, branch, covariates, groups)
        B, nt, nc, L, m = len(genomes), self.n_traits, 0 if q is None else q.shape[1], len(levels), len(an)
        rel = np.empty((B, m), dtype=np.float64)
        pev = np.empty((B, m), dtype=np.float64) if want_pev else None
        fc = np.empty((B, nc + L, nc + L), dtype=np.float64) if want_fc else None
        head = (_ptr(q) if nc else None, nc, _ptr(codes), L, _ptr(an) if m else None, m)
        tail = (_ptr(rel), _ptr(pev) if want_pev else None, _ptr(fc) if want_fc else None)

        def entry(sid, idx, offsets, *model):
            _native.check("tblup_reliability_group_batch", self._lib.tblup_reliability_group_batch(
                self._ctx, sid, *head, idx, offsets, B, float(h2), _native.BRANCH[branch], *model, *tail))
        models = None
        if want_models:
            cov_eff = np.empty((B, nt, nc), dtype=np.float64)
            cov_cen = np.empty((B, nc), dtype=np.float64)
            grp_eff = np.empty((B, nt, L), dtype=np.float64)
            grp_cen = np.empty((B, L), dtype=np.float64)

            def call(sid, idx, offsets, fit, *model):
                entry(sid, idx, offsets, fit, _ptr(cov_eff) if nc else None, _ptr(cov_cen) if nc else None,
                      _ptr(grp_eff), _ptr(grp_cen), *model)
            extra = dict(group_levels=np.broadcast_to(levels, (B, L)), group_effects=grp_eff, group_center=grp_cen)
            if nc:
                extra.update(cov_effects=cov_eff, cov_center=cov_cen)
            models = self._fit_models(genomes, train, valid, h2, branch, call, **extra)
        elif B:
            idx, offsets = concat_genomes(genomes)
            entry(self.split_id(train, valid), _ptr(idx), _ptr(offsets), *([None] * 8))
        return GroupReliability(rel, levels, nc, pev, fc, models)

    def snp_scores(self, genomes, train, valid, h2, snps=None, branch="auto", covariates=None, groups=None):
        """Mixed-model score statistics of the panel's SNPs `snps` (column ids: any order, repeats
        allowed, negatives wrap, in or out of the models; None: every column) against the model each
        selected-index set fits on (train, valid): a tblup_amd.model.SnpScores from
        tblup_snp_score_batch (include/tblup_gpu.h has the definitions) -- score u = w_j' V^-1 r_t
        (B, nt, n_cand), info v = w_j' V^-1 w_j (B, n_cand), q = r_t' V^-1 r_t (B, nt) and dof = N - r.
        u / d is the SNP's back-solved BLUP effect to first order (fit()'s effect for a SNP of the
        model).  h2 in (0, 1).  A degenerate model panel gives NaN; a (model, SNP) value does not
        depend on the list it comes in.  An empty list runs nothing: q is then NaN.
        covariates: an (n_animals, c) matrix Q as fit(covariates=) takes it -- the statistics are then those of
        the model with Q fitted beside the panel (tblup_snp_score_cov_batch): u_P, v_P, q_P with V^-1 replaced
        by P = V^-1 - V^-1 Q~ (Q~' V^-1 Q~)^-1 Q~' V^-1, dof = N - r - c, and `cov_effects` (B, nt, c)
        bit-identical to fit(covariates=Q)'s.  u_P / v_P is the GLS effect of the SNP fitted as one more
        covariate.  Collinear covariates give NaN for the model; a listed SNP in the span of the covariates
        gives u_P = v_P = 0, so NaN statistics."""
        self._no_groups(groups, "snp_scores()")
        from .model import SnpScores
        self._settle()
        cand = _as_int64(np.arange(self.n_snps) if snps is None else snps)
        if cand.ndim != 1:
            raise ValueError("snps must be a 1-D list of column ids")
        qc = None if covariates is None else self._covariates(covariates)
        sid = self.split_id(train, valid)
        idx, offsets = concat_genomes(genomes)
        B, nt, m = len(genomes), self.n_traits, len(cand)
        score = np.empty((B, nt, m), dtype=np.float64)
        info = np.empty((B, m), dtype=np.float64)
        q = np.full((B, nt), np.nan)
        snp = np.array([self._fitted_branch(k, branch) == "snp" for k in np.diff(offsets)], dtype=bool)
        dof = len(_as_int64(train)) - snp.astype(np.float64)
        wrapped = np.where(cand < 0, cand + self.n_snps, cand)
        if qc is not None:
            nc = qc.shape[1]
            cov_eff = np.full((B, nt, nc), np.nan)
            _native.check("tblup_snp_score_cov_batch", self._lib.tblup_snp_score_cov_batch(
                self._ctx, sid, _ptr(qc), nc, _ptr(cand) if m else None, m, _ptr(idx), _ptr(offsets), B, float(h2),
                _native.BRANCH[branch], None, _ptr(score), _ptr(info), _ptr(q), _ptr(cov_eff)))
            return SnpScores(score, info, q, (dof - nc).reshape(B), wrapped, cov_effects=cov_eff)
        _native.check("tblup_snp_score_batch", self._lib.tblup_snp_score_batch(
            self._ctx, sid, _ptr(cand) if m else None, m, _ptr(idx), _ptr(offsets), B, float(h2),
            _native.BRANCH[branch], None, _ptr(score), _ptr(info), _ptr(q)))
        return SnpScores(score, info, q, dof.reshape(B), wrapped)

    def snp_scores_group(self, genomes, train, valid, h2, groups, snps=None, branch="auto", covariates=None):
        """snp_scores() under the model with a class fixed effect that fit(groups=) fits (a method of its own, as
        log_likelihood_cov and estimate_h2_cov are: snp_scores(groups=) keeps raising).  groups and the optional
        covariates are fit()'s: (n_animals,) integer or string labels of one factor, an (n_animals, c) matrix Q.
        Returns a tblup_amd.model.SnpScores from tblup_snp_score_group_batch (include/tblup_gpu.h has the
        definitions): u_P, v_P, q_P with the fixed design F = [Q, Z] in place of Q, dof = N - r - C_m per model
        (C_m its column count: covariates + levels, one less under snp), `group_levels` (L,) and `group_effects`
        (B, nt, L) bit-identical to fit(groups=)'s, and `cov_effects` when there are covariates.  u_P / v_P is the GLS
        effect of the SNP fitted as one more covariate beside the factor.  A design that is collinear over the train
        rows, or C_m >= N - r, gives NaN for the model; a listed SNP in the span of the design gives u_P = v_P = 0."""
        from .model import SnpScores
        self._settle()
        cand = _as_int64(np.arange(self.n_snps) if snps is None else snps)
        if cand.ndim != 1:
            raise ValueError("snps must be a 1-D list of column ids")
        levels, codes, qc, cols = self._group_design(genomes, train, valid, branch, covariates, groups)
        sid = self.split_id(train, valid)
        idx, offsets = concat_genomes(genomes)
        B, nt, m, nc, L = len(genomes), self.n_traits, len(cand), 0 if qc is None else qc.shape[1], len(levels)
        score = np.empty((B, nt, m), dtype=np.float64)
        info = np.empty((B, m), dtype=np.float64)
        q = np.full((B, nt), np.nan)
        cov_eff = np.full((B, nt, nc), np.nan)
        grp_eff = np.full((B, nt, L), np.nan)
        snp = np.array([self._fitted_branch(k, branch) == "snp" for k in np.diff(offsets)], dtype=bool)
        dof = len(_as_int64(train)) - snp.astype(np.float64) - cols
        _native.check("tblup_snp_score_group_batch", self._lib.tblup_snp_score_group_batch(
            self._ctx, sid, _ptr(qc) if nc else None, nc, _ptr(codes), L, _ptr(cand) if m else None, m, _ptr(idx),
            _ptr(offsets), B, float(h2), _native.BRANCH[branch], None, _ptr(score), _ptr(info), _ptr(q),
            _ptr(cov_eff) if nc else None, _ptr(grp_eff)))
        return SnpScores(score, info, q, dof.reshape(B), np.where(cand < 0, cand + self.n_snps, cand),
                         cov_effects=cov_eff if nc else None, group_effects=grp_eff, group_levels=levels)

    # ------------------------------------------------- variance ratio by (RE)ML
    def log_likelihood(self, genomes, train, valid, h2, branch="auto", return_sigma2=False):
        """Profile (restricted) log-likelihood of h2 for the model each selected-index set fits on
        (train, valid) (tblup_loglik_batch; include/tblup_gpu.h has the definition: the gblup branch's
        likelihood with no mean fitted, the snp branch's restricted likelihood with its intercept).
        h2: a scalar, a (G,) grid shared by all models, or a (G, B) matrix of per-model values, each in
        (0, 1).  Returns (G, B) -- (B,) for a scalar -- with the trait axis appended for several traits,
        as evaluate(return_ebv=True) shapes its output; return_sigma2=True: (loglik, sigma2_g), the
        profiled genetic variance in the same shape (sigma2_e = (1 - h2) / h2 * sigma2_g).  A degenerate
        panel gives NaN, not an error; a model's value does not depend on the batch it comes in.
        With fixed-effect covariates: log_likelihood_cov."""
        ll, s2, _ = self._loglik(genomes, train, valid, h2, branch, False)
        return (ll, s2) if return_sigma2 else ll

    def log_likelihood_cov(self, genomes, train, valid, h2, covariates, branch="auto", return_sigma2=False,
                           groups=None):
        """log_likelihood for the model that fit(covariates=) fits (this method's signature is that one's with
        `covariates` added; log_likelihood's own stays as it is): covariates is the (n_animals, c) matrix Q as
        fit takes it, and the value is the restricted likelihood of the N - r - c error contrasts of the model
        with Q fitted beside the panel (tblup_loglik_cov_batch; include/tblup_gpu.h has the definition), with
        sigma2_g = q_P / (N - r - c).  Under gblup a mean is fitted only if Q carries a column of ones.
        Collinear covariates, or c >= N - r, give NaN; NaN / Inf in Q is a ValueError."""
        self._no_groups(groups, "log_likelihood_cov()")
        ll, s2, _ = self._loglik(genomes, train, valid, h2, branch, False, covariates)
        return (ll, s2) if return_sigma2 else ll

    def log_likelihood_group(self, genomes, train, valid, h2, groups, covariates=None, branch="auto",
                             return_sigma2=False):
        """log_likelihood for the model that fit(groups=) fits (a method of its own: log_likelihood_cov(groups=)
        keeps raising): groups and the optional covariates as fit() takes them, and the value is the restricted
        likelihood of the N - r - C_m error contrasts of the model with the fixed design [Q, Z] fitted beside the panel
        (tblup_loglik_group_batch; include/tblup_gpu.h has the definition), with sigma2_g = q_P / (N - r - C_m).
        h2 as log_likelihood takes it.  A design that is collinear over the train rows, or C_m >= N - r, gives NaN."""
        ll, s2, _ = self._loglik(genomes, train, valid, h2, branch, False, covariates, groups)
        return (ll, s2) if return_sigma2 else ll

    def _loglik(self, genomes, train, valid, h2, branch, want_fitness, covariates=None, groups=None):
        self._settle()
        if groups is not None:
            levels, codes, qc, _ = self._group_design(genomes, train, valid, branch, covariates, groups)
        else:
            qc = None if covariates is None else self._covariates(covariates)
        idx, offsets = concat_genomes(genomes)
        B, nt = len(genomes), self.n_traits
        h = np.asarray(h2, dtype=np.float64)
        scalar = h.ndim == 0
        if h.ndim == 0:
            h = h.reshape(1, 1)
        if h.ndim == 1:
            h = h[:, None]
        if h.ndim != 2 or h.shape[1] not in (1, B):
            raise ValueError("h2 must be a scalar, a (G,) grid or a (G, %d) matrix" % B)
        G = h.shape[0]
        hm = np.ascontiguousarray(np.broadcast_to(h, (G, B)))
        ll = np.empty((G, B, nt), dtype=np.float64)
        s2 = np.empty((G, B, nt), dtype=np.float64)
        fit = np.empty((G, B), dtype=np.float64) if want_fitness else None
        if B and G and groups is not None:
            sid = self.split_id(train, valid)
            nc = 0 if qc is None else qc.shape[1]
            _native.check("tblup_loglik_group_batch", self._lib.tblup_loglik_group_batch(
                self._ctx, sid, _ptr(qc) if nc else None, nc, _ptr(codes), len(levels), _ptr(idx), _ptr(offsets), B,
                _ptr(hm), G, _native.BRANCH[branch], _ptr(fit) if want_fitness else None, _ptr(ll), _ptr(s2), None, None))
        elif B and G and qc is not None:
            sid = self.split_id(train, valid)
            _native.check("tblup_loglik_cov_batch", self._lib.tblup_loglik_cov_batch(
                self._ctx, sid, _ptr(qc), qc.shape[1], _ptr(idx), _ptr(offsets), B, _ptr(hm), G, _native.BRANCH[branch],
                _ptr(fit) if want_fitness else None, _ptr(ll), _ptr(s2), None))
        elif B and G:
            sid = self.split_id(train, valid)
            _native.check("tblup_loglik_batch", self._lib.tblup_loglik_batch(
                self._ctx, sid, _ptr(idx), _ptr(offsets), B, _ptr(hm), G, _native.BRANCH[branch],
                _ptr(fit) if want_fitness else None, _ptr(ll), _ptr(s2)))
        if nt == 1:
            ll, s2 = ll[:, :, 0], s2[:, :, 0]
        if scalar:
            ll, s2, fit = ll[0], s2[0], (fit[0] if want_fitness else None)
        return ll, s2, fit

    def estimate_h2(self, genomes, train, valid, branch="auto", grid=np.linspace(0.02, 0.98, 25), refine=3,
                    points=9):
        """h2 of each model by maximising log_likelihood(): one pass over `grid` (ascending, shared by
        all models), then `refine` rounds in which every model gets its own `points` evenly spaced
        values between the neighbours of its current argmax, endpoints included (at an end of the
        current values the bracket is that end and its one neighbour; ties take the first argmax);
        each round is one call with a (points, B) matrix.  With several traits the grid pass is shared
        and the refinement runs once per trait.
        Returns a dict of arrays shaped (B,) -- (B, n_traits) for several traits: `h2`, `loglik` and
        `sigma2_g` at the best point, `sigma2_e` = (1 - h2) / h2 * sigma2_g, `at_bound` (the best point
        is an end of `grid`: the maximum lies outside it or at its edge) and `step`, the spacing of the
        last round's values.  A model whose likelihood is NaN everywhere stays NaN.
        The profile is not guaranteed to be unimodal: the answer is the best point seen, a local
        maximum when the grid is too coarse to separate two.
        With fixed-effect covariates: estimate_h2_cov."""
        return self._estimate_h2(genomes, train, valid, branch, grid, refine, points, None)

    def estimate_h2_cov(self, genomes, train, valid, covariates, branch="auto", grid=np.linspace(0.02, 0.98, 25),
                        refine=3, points=9, groups=None):
        """estimate_h2 on log_likelihood_cov: the h2 of the model that fit(covariates=) fits -- the value to
        pass to fit(covariates=) and snp_scores(covariates=).  The same search, the same returned fields."""
        self._no_groups(groups, "estimate_h2_cov()")
        return self._estimate_h2(genomes, train, valid, branch, grid, refine, points, covariates)

    def estimate_h2_group(self, genomes, train, valid, groups, covariates=None, branch="auto",
                          grid=np.linspace(0.02, 0.98, 25), refine=3, points=9):
        """estimate_h2 on log_likelihood_group: the h2 of the model that fit(groups=) fits -- the value to pass to
        fit(groups=) and snp_scores_group().  The same search, the same returned fields."""
        return self._estimate_h2(genomes, train, valid, branch, grid, refine, points, covariates, groups)

    def _estimate_h2(self, genomes, train, valid, branch, grid, refine, points, covariates, groups=None):
        grid = np.asarray(grid, dtype=np.float64)
        if grid.ndim != 1 or len(grid) < 2 or not np.all(np.diff(grid) > 0):
            raise ValueError("grid must be 1-D, ascending, with at least two values")
        if points < 3:
            raise ValueError("points must be at least 3")
        B, nt = len(genomes), self.n_traits
        ll0, s20, _ = self._loglik(genomes, train, valid, grid, branch, False, covariates, groups)
        ll0, s20 = ll0.reshape(len(grid), B, nt), s20.reshape(len(grid), B, nt)
        out = {k: np.full((B, nt), np.nan) for k in ("h2", "loglik", "sigma2_g", "sigma2_e", "step")}
        out["at_bound"] = np.zeros((B, nt), dtype=bool)
        cols = np.arange(B)
        for t in range(nt):
            h = np.repeat(grid[:, None], B, axis=1)
            ll, s2 = ll0[:, :, t], s20[:, :, t]
            best = None
            for rnd in range(refine + 1):
                i = np.argmax(np.where(np.isnan(ll), -np.inf, ll), axis=0)   # first maximum
                cur = (h[i, cols], ll[i, cols], s2[i, cols])
                if best is None:
                    best = cur
                else:
                    up = cur[1] > best[1]
                    best = tuple(np.where(up, c, b) for c, b in zip(cur, best))
                step = h[1] - h[0]
                if rnd == refine or B == 0:
                    break
                lo, hi = h[np.maximum(i - 1, 0), cols], h[np.minimum(i + 1, len(h) - 1), cols]
                h = np.linspace(lo, hi, points)      # (points, B), both ends exact
                ll, s2, _ = self._loglik(genomes, train, valid, h, branch, False, covariates, groups)
                ll, s2 = ll.reshape(points, B, nt)[:, :, t], s2.reshape(points, B, nt)[:, :, t]
            dead = np.isnan(best[1])
            hb = np.where(dead, np.nan, best[0])
            out["h2"][:, t], out["loglik"][:, t], out["sigma2_g"][:, t] = hb, best[1], np.where(dead, np.nan, best[2])
            out["sigma2_e"][:, t] = (1.0 - hb) / hb * out["sigma2_g"][:, t]
            out["step"][:, t] = np.where(dead, np.nan, step)
            out["at_bound"][:, t] = ~dead & ((hb == grid[0]) | (hb == grid[-1]))
        return {k: v[:, 0] for k, v in out.items()} if nt == 1 else out

    def predict(self, models, animals):
        """EBVs of `animals` (row ids of this engine's panel: any order, repeats allowed, no split
        needed) under each PanelModel (tblup_predict_batch): (len(models), n_traits, len(animals)),
        the trait axis dropped for one trait as evaluate(return_ebv=True) shapes its output.  An
        animal's EBV does not depend on its position in the list."""
        self._settle()
        models = list(models)
        an = _as_int64(animals)
        if an.ndim != 1:
            raise ValueError("animals must be a 1-D list of row ids")
        nt = models[0].n_traits if models else self.n_traits
        if any(m.n_traits != nt for m in models):
            raise ValueError("models of one call must have the same number of traits")
        idx, offsets = concat_genomes([m.indices for m in models])
        B, total = len(models), int(offsets[-1])
        out = np.empty((B, nt, len(an)), dtype=np.float64)
        if B and len(an):
            intercept = np.ascontiguousarray(np.stack([m.intercept for m in models]))
            center = np.ascontiguousarray(np.concatenate([m.center for m in models]))
            effects = np.ascontiguousarray(np.concatenate([m.effects for m in models], axis=1))
            assert effects.shape == (nt, total)
            _native.check("tblup_predict_batch", self._lib.tblup_predict_batch(
                self._ctx, _ptr(an), len(an), _ptr(idx), _ptr(offsets), B, _ptr(intercept), _ptr(center), _ptr(effects),
                nt, _ptr(out)))
        return out[:, 0, :] if nt == 1 else out

    def evaluate_folds(self, genomes, splits, h2, branch="auto"):
        """Every genome against each (train, valid) split in one call (tblup_eval_folds: the
        splits' evaluations back to back on the GPU, one round trip): (n_splits, B) fitness, row f
        bit-identical to evaluate(genomes, *splits[f]).  IntraGCV's k folds (evaluator.py:509-537)."""
        self._settle()
        sids = np.array(self.split_ids(splits), dtype=np.int32)
        idx, offsets = concat_genomes(genomes)
        B = len(genomes)
        fit = np.empty((len(sids), B), dtype=np.float64)
        if B:
            _native.check("tblup_eval_folds", self._lib.tblup_eval_folds(
                self._ctx, _ptr(sids), len(sids), _ptr(idx), _ptr(offsets), B, float(h2), _native.BRANCH[branch],
                _ptr(fit)))
        return fit

    def evaluate_folds_device(self, split_ids, d_idx_ptr, d_off_ptr, h_offsets, h2, d_fit_ptr, stream_ptr=None,
                              branch="auto", groups=None):
        """Asynchronous evaluate_folds on device-resident buffers (d_fit: n_splits x B)."""
        self._no_groups(groups, "evaluate_folds_device()")
        self._settle()
        sids = np.ascontiguousarray(split_ids, dtype=np.int32)
        h_off = _as_int64(h_offsets)
        _native.check("tblup_eval_folds_device", self._lib.tblup_eval_folds_device(
            self._ctx, _ptr(sids), len(sids), ctypes.c_void_p(d_idx_ptr), ctypes.c_void_p(d_off_ptr), _ptr(h_off),
            len(h_off) - 1, float(h2), _native.BRANCH[branch], ctypes.c_void_p(d_fit_ptr),
            ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def evaluate_device(self, split_id, d_idx_ptr, d_off_ptr, h_offsets, h2, d_fit_ptr, d_ebv_ptr=None,
                        stream_ptr=None, branch="auto", groups=None):
        """Asynchronous evaluation on device-resident buffers (raw device pointers)."""
        self._no_groups(groups, "evaluate_device()")
        self._settle()
        h_off = _as_int64(h_offsets)
        B = len(h_off) - 1
        _native.check("tblup_eval_batch_device", self._lib.tblup_eval_batch_device(
            self._ctx, split_id, ctypes.c_void_p(d_idx_ptr), ctypes.c_void_p(d_off_ptr), _ptr(h_off), B, float(h2),
            _native.BRANCH[branch], ctypes.c_void_p(d_fit_ptr), ctypes.c_void_p(d_ebv_ptr) if d_ebv_ptr else None,
            ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def index_error(self, stream_ptr=None):
        """True if an individual evaluated through evaluate_device since the last call had an
        index outside [-P, P) (its fitness is NaN); synchronises the stream, clears the flag."""
        self._settle()
        flag = ctypes.c_int(0)
        _native.check("tblup_index_error", self._lib.tblup_index_error(
            self._ctx, ctypes.c_void_p(stream_ptr) if stream_ptr else None, ctypes.byref(flag)))
        return bool(flag.value)

    def solve_error(self, stream_ptr=None):
        """True if a chained-solve hand-off wait expired in a device-entry evaluation since the
        last call (those fitnesses are invalid); synchronises the stream, clears the flag."""
        self._settle()
        flag = ctypes.c_int(0)
        _native.check("tblup_solve_error", self._lib.tblup_solve_error(
            self._ctx, ctypes.c_void_p(stream_ptr) if stream_ptr else None, ctypes.byref(flag)))
        return bool(flag.value)

    def check_device_status(self, stream_ptr=None):
        """Raise for a device-entry evaluation that failed: TblupIndexError for an index outside
        [-P, P) (numpy's IndexError), TblupError for an expired chained-solve wait."""
        if self.index_error(stream_ptr):
            raise _native.TblupIndexError("tblup_eval_batch_device", _native.ERR_INDEX,
                                          "an index is out of bounds for axis 1 with size %d" % self.n_snps)
        if self.solve_error(stream_ptr):
            raise _native.TblupError("tblup_eval_batch_device", _native.ERR_STATE, _native.CHAIN_EXPIRED)

    def status_async(self, host_status, stream_ptr=None):
        """Enqueue the copy of the device status words {index error, solve error} into the
        page-locked int32 tensor `host_status` (and clear them); read it after the stream's event."""
        _native.check("tblup_status_async", self._lib.tblup_status_async(
            self._ctx, ctypes.c_void_p(stream_ptr) if stream_ptr else None, ctypes.c_void_p(host_status.data_ptr())))

    def chain_recoveries(self):
        """Chunks the synchronous entries re-solved through k_solve after a chained-solve wait
        expired (tblup_chain_recoveries); the speculative path's fallbacks are counted by the
        evaluator (BlupParallelEvaluator.spec_fallbacks)."""
        v = ctypes.c_int64(0)
        _native.check("tblup_chain_recoveries", self._lib.tblup_chain_recoveries(self._ctx, ctypes.byref(v)))
        return v.value

    @staticmethod
    def raise_status(status, fn="tblup_eval_batch_device", n_snps=None):
        """Raise for nonzero status words read through status_async."""
        if int(status[0]):
            raise _native.TblupIndexError(fn, _native.ERR_INDEX, "an index is out of bounds for axis 1"
                                          + ("" if n_snps is None else " with size %d" % n_snps))
        if int(status[1]):
            raise _native.TblupError(fn, _native.ERR_STATE, _native.CHAIN_EXPIRED)

    def decode_randkey(self, keys, lengths):
        """RandomKeyIndividual.genome for a batch (individual.py:154-156) on the GPU:
        row i -> np.argsort(keys[i])[-int(lengths[i]):] (ascending key order; equal keys
        ordered by index, as a stable argsort).  Returns (idx, offsets) for evaluate_concat."""
        self._settle()
        kk = np.ascontiguousarray(np.asarray(keys, dtype=np.float64))
        if kk.ndim != 2:
            raise ValueError("keys must be (batch, d)")
        B, d = kk.shape
        lens = np.broadcast_to(np.asarray(lengths), (B,)).astype(np.int64)
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        idx = np.empty(int(offsets[-1]), dtype=np.int64)
        if B:
            _native.check("tblup_decode_topk", self._lib.tblup_decode_topk(
                self._ctx, _ptr(kk), B, d, _ptr(offsets), _ptr(idx)))
        return idx, offsets

    def decode_randkey_device(self, d_keys_ptr, B, d, ld, d_off_ptr, h_offsets, d_idx_ptr, stream_ptr=None):
        """Device-resident decode: keys (B x ld doubles) -> idx at offsets (device pointers)."""
        self._settle()
        h_off = _as_int64(h_offsets)
        _native.check("tblup_decode_topk_device", self._lib.tblup_decode_topk_device(
            self._ctx, ctypes.c_void_p(d_keys_ptr), B, d, ld, ctypes.c_void_p(d_off_ptr), _ptr(h_off),
            ctypes.c_void_p(d_idx_ptr), ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def grm(self, indices=None):
        """make_grm(data[:, indices]) over all animals (tblup/utils.py:7-18) on the GPU:
        n x n float64.  indices=None: every SNP of the panel."""
        self._settle()
        idx = _as_int64(np.arange(self.n_snps) if indices is None else indices)
        G = np.empty((self.n_animals, self.n_animals), dtype=np.float64)
        _native.check("tblup_grm", self._lib.tblup_grm(self._ctx, _ptr(idx), len(idx),
                                                       _ptr(G)))
        return G

    def snp_scan(self, rows, yc):
        """Per-SNP (sum x, sum x^2, sum x*yc) over animal `rows` (k_snp_scan)."""
        self._settle()
        r = _as_int64(rows)
        y = np.ascontiguousarray(yc, dtype=np.float64)
        if y.shape != r.shape:
            raise ValueError("yc must have one value per row")
        sx = np.empty(self.n_snps, dtype=np.int64)
        sxx = np.empty(self.n_snps, dtype=np.int64)
        sxy = np.empty(self.n_snps, dtype=np.float64)
        _native.check("tblup_snp_scan", self._lib.tblup_snp_scan(
            self._ctx, _ptr(r), len(r), _ptr(y), _ptr(sx), _ptr(sxx), _ptr(sxy)))
        return sx, sxx, sxy

    def decode_randkey_tensor(self, keys, d, lengths):
        """decode_randkey on a device tensor of key rows (B x ld float64, ld >= d, on this
        context's device) on torch's current stream; returns host (idx, offsets)."""
        self._settle()
        import torch
        from .keystore import work_stream
        B, ld = keys.shape
        lens = np.broadcast_to(np.asarray(lengths), (B,)).astype(np.int64)
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        ws = work_stream(keys.device.index)
        ws.wait_stream(torch.cuda.current_stream(keys.device))
        with torch.cuda.stream(ws):   # one stream for the copies and the library's kernel
            d_off = torch.from_numpy(offsets).to(keys.device)
            d_idx = torch.empty(int(offsets[-1]), dtype=torch.int64, device=keys.device)
            if B:
                self.decode_randkey_device(keys.data_ptr(), B, d, keys.stride(0), d_off.data_ptr(), offsets,
                                           d_idx.data_ptr(), ws.cuda_stream)
            out = d_idx.cpu().numpy()
        return out, offsets

    def evaluate_concat(self, idx, offsets, train, valid, h2, branch="auto"):
        """evaluate() on an already-concatenated (idx, offsets) batch."""
        self._settle()
        sid = self.split_id(train, valid)
        idx = _as_int64(idx)
        offsets = _as_int64(offsets)
        B = len(offsets) - 1
        fit = np.empty(B, dtype=np.float64)
        if B:
            _native.check("tblup_eval_batch", self._lib.tblup_eval_batch(
                self._ctx, sid, _ptr(idx), _ptr(offsets), B, float(h2), _native.BRANCH[branch], _ptr(fit), None))
        return fit

    def debug_grm(self, indices, train, valid, h2, branch="auto", stage=1):
        """K_{R,T} (stage 1) or the factored block (stage 2) and z for one individual."""
        self._settle()
        sid = self.split_id(train, valid)
        idx = _as_int64(indices)
        nT, nV = len(train), len(valid)
        out = np.empty((nT + nV, nT), dtype=np.float64)
        z = np.empty(nT, dtype=np.float64)
        _native.check("tblup_debug_grm", self._lib.tblup_debug_grm(
            self._ctx, sid, _ptr(idx), len(idx), float(h2), _native.BRANCH[branch], int(stage), _ptr(out), _ptr(z)))
        return out, z

    def eval_keys_async(self, keys, lengths, train, valid, h2):
        """RandomKey individuals' fitness straight from a device tensor of their keys (B x ld
        float64 on this context's device): decode (k_decode_topk) and evaluation enqueued on a
        stream of this engine without waiting.  Returns (event, pinned host fitness tensor, pinned
        status words); both are valid once the event has completed (raise_status(status) then
        raises for a failed evaluation).  Later calls on the engine wait for it."""
        import torch
        self._settle()
        B, ld = keys.shape
        lens = np.asarray(lengths, dtype=np.int64)
        offsets = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        sid = self.split_id(train, valid)
        dev = keys.device
        if self._spec_stream is None:
            self._spec_stream = torch.cuda.Stream(device=dev)
        st = self._spec_stream
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev), torch.cuda.stream(st):
            d_off = torch.from_numpy(offsets).to(dev, non_blocking=True)
            d_idx = torch.empty(int(offsets[-1]), dtype=torch.int64, device=dev)
            d_fit = torch.empty(B, dtype=torch.float64, device=dev)
            self.decode_randkey_device(keys.data_ptr(), B, ld, keys.stride(0), d_off.data_ptr(), offsets,
                                       d_idx.data_ptr(), st.cuda_stream)
            self.evaluate_device(sid, d_idx.data_ptr(), d_off.data_ptr(), offsets, h2, d_fit.data_ptr(),
                                 stream_ptr=st.cuda_stream)
            host = torch.empty(B, dtype=torch.float64, pin_memory=True)
            host.copy_(d_fit, non_blocking=True)
            status = torch.zeros(2, dtype=torch.int32, pin_memory=True)
            self.status_async(status, st.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(st)
        self._pending = (ev, (keys, d_off, d_idx, d_fit, offsets))
        return ev, host, status

    # --------------------------------------------------------------- profiling
    def set_profiling(self, enable=True):
        _native.check("tblup_set_profiling", self._lib.tblup_set_profiling(self._ctx, 1 if enable else 0))

    def reset_profile(self):
        _native.check("tblup_reset_profile", self._lib.tblup_reset_profile(self._ctx))

    def profile(self):
        n = _native.N_KCLASS
        ms = np.zeros(n)
        la = np.zeros(n, dtype=np.int64)
        fl = np.zeros(n)
        by = np.zeros(n)
        _native.check("tblup_get_profile", self._lib.tblup_get_profile(
            self._ctx, _ptr(ms), _ptr(la), _ptr(fl), _ptr(by)))
        return {name: {"ms": float(ms[i]), "launches": int(la[i]), "flops": float(fl[i]), "bytes": float(by[i])}
                for i, name in enumerate(_native.KCLASS_NAMES)}

    def wg_trace(self, raw=False):
        """Per-workgroup records of the last evaluation's Cholesky launches and chained solve
        (TBLUP_WG_TRACE=1): structured array (start, end [s], kind, J, I, b, wait [s]); raw=True: the (n, 4) uint64 records
        (including each diagonal launch's phase-stamp block, kind 0)."""
        n = ctypes.c_int64(0)
        _native.check("tblup_get_wg_trace", self._lib.tblup_get_wg_trace(self._ctx, None, 0, ctypes.byref(n)))
        raw_out = raw
        raw = np.zeros((n.value, 4), dtype=np.uint64)
        if n.value:
            _native.check("tblup_get_wg_trace", self._lib.tblup_get_wg_trace(
                self._ctx, _ptr(raw), n.value, ctypes.byref(n)))
        if raw_out:
            return raw
        out = np.zeros(len(raw), dtype=[("start", "f8"), ("end", "f8"), ("kind", "i4"), ("J", "i4"), ("I", "i4"),
                                        ("b", "i8"), ("wait", "f8")])
        out["start"] = raw[:, 0] / 1e8
        out["end"] = raw[:, 1] / 1e8
        out["kind"] = (raw[:, 2] >> np.uint64(56)).astype(np.int32)
        out["I"] = ((raw[:, 2] >> np.uint64(40)) & np.uint64(0xFFFF)).astype(np.int32)
        out["b"] = (raw[:, 2] & np.uint64((1 << 40) - 1)).astype(np.int64)
        out["J"] = (raw[:, 3] & np.uint64(0xFFFF)).astype(np.int32)
        out["wait"] = (raw[:, 3] >> np.uint64(16)) / 1e8      # chained-solve units: first wait done - start
        return out[out["kind"] != 0]

    def mem_in_use(self):
        v = ctypes.c_int64(0)
        _native.check("tblup_mem_info", self._lib.tblup_mem_info(self._ctx, ctypes.byref(v)))
        return v.value

    # ----------------------------------------------------------------- cleanup
    def close(self):
        if getattr(self, "_pending", None) is not None:
            self._settle()
        if getattr(self, "_ctx", None):
            self._lib.tblup_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
