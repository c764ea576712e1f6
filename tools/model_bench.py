"""Timings of the model export (tblup_fit_batch / tblup_predict_batch); no thresholds, the
numbers go to PERFLOG.md.  One JSON line per part:

  fit      config 2 (2000 x 50k, k = 1000, 256 individuals, n_T 1280, n_V 320): fit against evaluate
           in one process, alternated, each call timed as the synchronous entry it is (wall clock
           around a call that ends in the stream's synchronisation; medians over --reps)
  predict  the 256 fitted models for all 2000 animals: time, and bytes/s over the bytes k_predict
           must read (batch x k x n genotype bytes) against the 8 TB/s HBM figure
  dual     a config-4-shaped small stand-in in the kernel form (1200 x 20k, k = 1500 > n: gblup,
           n_T 768, 32 individuals): fit against evaluate, predict for all animals
  reliability  config 2 again: reliabilities of all 2000 animals under the 256 models
           (tblup_reliability_batch) against fit and evaluate from the same process, alternated; the
           derived fp64 MFMA floor of k_reliab (batch x n_pred x ns^2 flop over the measured 72.7 TF/s
           peak); and one kernel-form shape (the `dual` stand-in, all 1200 animals)
  loglik   config 2 again: tblup_loglik_batch at 1 and at 8 grid points (per grid point: the 8-point call
           over 8) beside tblup_eval_batch from the same process, alternated; one estimate_h2 with the
           defaults (25 + 3 x 9 passes); k_loglik per launch comes from a --stats run of this part
  score    config 2 again: snp_scores() of (i) 2,000 listed SNPs under the 256 models and (ii) all 50k SNPs
           under one model, beside reliability() of 2,000 animals under the 256 models (the same number of
           right-hand sides through the same substitution) and evaluate(), alternated in one process; the
           derived fp64 MFMA floor (batch x n_cand x ns^2 flop over the measured 72.7 TF/s peak); k_snpscore
           and k_reliab per launch come from a --stats run of this part
  covar    config 2 again: fit(covariates=Q) with 16 covariates (tblup_fit_cov_batch) beside fit() (tblup_fit_batch)
           and snp_scores() of 16 listed SNPs -- the same substitution, one slab per model -- alternated in one
           process; k_covar beside k_snpscore, the second k_solve and k_cov_fitness per launch come from a
           --stats run of this part
  group    config 2 again: fit(groups=) with 64 levels, fit(covariates=Q, groups=) with 112 levels + 16 covariates
           (tblup_fit_group_batch: 63 and 127 columns under snp), fit(covariates=Q) with 16 covariates and fit(),
           alternated in one process; k_fixed_subst, k_fixed_gls and k_fixed_fitness per launch beside k_covar and
           k_snpscore come from a --stats run of this part (run it with `--only group,covar`)
  score_cov   config 2 again: snp_scores(covariates=Q) with 16 covariates (tblup_snp_score_cov_batch) beside
           snp_scores() on the same 2,000-SNP list as `score`, alternated in one process: the ratio is the cost of
           the covariate adjustment (k_covar in keep mode once per chunk, then S^T s_j, the SNP form's Q~^T x_j
           chains and the 16-step solve per slab)
  loglik_cov  config 2 again: tblup_loglik_cov_batch beside tblup_loglik_batch at the same 8 grid points,
           alternated (per grid point: one k_covar launch more per pass)
  reliab_cov  config 2 again: reliability_cov(covariates=Q) with 16 covariates (tblup_reliability_cov_batch) beside
           reliability() for all 2,000 animals under the 256 models, alternated in one process: the ratio is the cost
           of the covariate adjustment (k_covar in keep mode once per chunk, then S^T s_a and the two 16-step solves
           per slab); k_reliab's adjusted and plain launches and the k_covar keep launch come from a --stats run of
           this part (the --stats reader lists them apart)
  score_group  config 2 again: snp_scores_group() at 64 levels (63 columns under snp) and at 112 levels + 16 covariates
           (127 columns) (tblup_snp_score_group_batch) beside snp_scores() and snp_scores(covariates=16 columns) on the
           same 2,000-SNP list, alternated in one process; beside each ratio the derived flop share of the
           adjustment over the plain substitution, 2 C_m / ns + C_m^2 / ns^2; k_snpscore's plain, 16-column and
           wide launches, k_fixed_subst and k_fixed_gls (keep mode) come from a --stats run of this part
  loglik_group  config 2 again: tblup_loglik_group_batch at 64 levels and at 112 levels + 16 covariates beside
           tblup_loglik_cov_batch (16 covariates) at the same 8 grid points and fit(groups=) at both designs, alternated;
           one estimate_h2_group with the defaults (25 + 3 x 9 passes) at 64 levels
  reliab_group  config 2 again: reliability_group() at 64 levels (63 columns under snp) and at 112 levels + 16 covariates
           (127 columns) (tblup_reliability_group_batch) beside reliability(), reliability_cov(16 covariates) and
           fit(groups=) at both designs for all 2,000 animals under the 256 models, alternated in one process; beside
           each ratio the derived flop share of the adjustment over the plain substitution, 2 C_m / ns + 2 C_m^2 / ns^2
           (the cross product and the two solves); k_reliab's plain, 16-column and wide launches and k_fixed_cov come
           from a --stats run of this part
  loo      config 2 again: loo() of the 256 models (1,280 training animals each) beside reliability() of the same
           1,280 animals -- as many right-hand sides through the same substitution -- evaluate() and the 5-fold
           IntraGCV entry (evaluate_folds on a partition of the train set), alternated in one process; and the
           kernel-form stand-in of `dual` (768 training animals, unit-column right-hand sides); k_loo, k_loo_fitness
           and k_reliab per launch come from a --stats run of this part
  --stats CSV   the k_effects / k_predict / k_reliab / k_snpscore / k_loglik share of a `rocprofv3 --kernel-trace --stats` run of
           `model_bench.py --only fit,predict` (a run of its own): reads its kernel_stats CSV

    python tools/model_bench.py [--only fit,predict,dual,reliability,loglik,score,covar,group,score_cov,loglik_cov,reliab_cov,score_group,loglik_group,reliab_group,loo] [--reps 7]
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python tools/model_bench.py --only fit,predict --reps 3
    python tools/model_bench.py --stats DIR/.../trace_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0   # the microarchitecture guide's HBM figure (bench.py PEAKS)


def workload(n, P, k, pop, nT, nV, seed=1234):
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, size=P)
    geno = rng.binomial(2, maf, size=(n, P)).astype(np.int8)
    pheno = rng.standard_normal(n)
    perm = rng.permutation(n)
    if k <= P:
        genomes = [rng.choice(P, k, replace=False) for _ in range(pop)]
    else:
        genomes = [rng.integers(0, P, k) for _ in range(pop)]
    return geno, pheno, perm[:nT], perm[nT:nT + nV], genomes


def med_ms(ts):
    return round(float(np.median(ts)) * 1e3, 4)


def fit_vs_eval(eng, genomes, T, V, reps):
    """Alternated evaluate / fit calls on one engine; returns (models, stats)."""
    te, tf = [], []
    models = None
    for r in range(reps + 2):
        t0 = time.perf_counter()
        fit = eng.evaluate(genomes, T, V, 0.4)
        t1 = time.perf_counter()
        models = eng.fit(genomes, T, V, 0.4)
        t2 = time.perf_counter()
        if r >= 2:
            te.append(t1 - t0)
            tf.append(t2 - t1)
    assert np.array_equal(fit, [m.fitness for m in models], equal_nan=True)
    return models, {"evaluate_ms": med_ms(te), "fit_ms": med_ms(tf), "extra_ms": round(med_ms(tf) - med_ms(te), 4),
                    "evaluate_ms_all": [round(x * 1e3, 3) for x in te], "fit_ms_all": [round(x * 1e3, 3) for x in tf],
                    "note": "fit includes building the PanelModel objects and the D2H copy of the effects"}


def fit_raw(eng, genomes, T, V, reps):
    """The C entries alone (no PanelModel objects): tblup_eval_batch against tblup_fit_batch."""
    from tblup_amd.engine import concat_genomes
    from tblup_amd import _native
    _ptr = _native.ptr
    sid = eng.split_id(T, V)
    idx, off = concat_genomes(genomes)
    B, total = len(genomes), int(off[-1])
    fit = np.empty(B)
    icp, cen, eff = np.empty((B, eng.n_traits)), np.empty(total), np.empty((eng.n_traits, total))
    te, tf = [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        _native.check("tblup_eval_batch", eng._lib.tblup_eval_batch(eng._ctx, sid, _ptr(idx), _ptr(off), B, 0.4, 0,
                                                                    _ptr(fit), None))
        t1 = time.perf_counter()
        _native.check("tblup_fit_batch", eng._lib.tblup_fit_batch(eng._ctx, sid, _ptr(idx), _ptr(off), B, 0.4, 0,
                                                                  _ptr(fit), _ptr(icp), _ptr(cen), _ptr(eff)))
        t2 = time.perf_counter()
        if r >= 2:
            te.append(t1 - t0)
            tf.append(t2 - t1)
    return {"eval_batch_ms": med_ms(te), "fit_batch_ms": med_ms(tf), "extra_ms": round(med_ms(tf) - med_ms(te), 4),
            "eval_batch_ms_all": [round(x * 1e3, 3) for x in te], "fit_batch_ms_all": [round(x * 1e3, 3) for x in tf]}


def predict_all(eng, models, n, reps):
    an = np.arange(n)
    ts = []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        out = eng.predict(models, an)
        t1 = time.perf_counter()
        if r >= 2:
            ts.append(t1 - t0)
    k = sum(len(m.indices) for m in models)
    must = float(k) * n                      # genotype bytes the kernel must read
    s = float(np.median(ts))
    return out, {"predict_ms": med_ms(ts), "predict_ms_all": [round(x * 1e3, 3) for x in ts],
                 "bytes_must_read": must, "gbs_call": round(must / s / 1e9, 1),
                 "frac_hbm_call": round(must / s / 1e9 / HBM_GBS, 4),
                 "note": "the call includes the H2D copy of the models and the D2H copy of the EBVs; "
                         "the kernel alone: --stats"}


F64_MFMA_TFS = 72.7   # measured fp64 MFMA peak (README, profiles/r02f_mfma_peak.json)


def reliability_all(eng, genomes, T, V, n, ns, reps):
    """reliability() for the whole herd against fit() and evaluate(), alternated on one engine."""
    an = np.arange(n)
    te, tf, tr = [], [], []
    rel = None
    for r in range(reps + 2):
        t0 = time.perf_counter()
        eng.evaluate(genomes, T, V, 0.4)
        t1 = time.perf_counter()
        eng.fit(genomes, T, V, 0.4)
        t2 = time.perf_counter()
        rel = eng.reliability(genomes, T, V, 0.4, an)
        t3 = time.perf_counter()
        if r >= 2:
            te.append(t1 - t0)
            tf.append(t2 - t1)
            tr.append(t3 - t2)
    flop = float(len(genomes)) * n * ns * ns
    return {"evaluate_ms": med_ms(te), "fit_ms": med_ms(tf), "reliability_ms": med_ms(tr),
            "extra_ms_over_evaluate": round(med_ms(tr) - med_ms(te), 4),
            "reliability_ms_all": [round(x * 1e3, 3) for x in tr], "k_reliab_flop": flop,
            "k_reliab_floor_ms": round(flop / (F64_MFMA_TFS * 1e12) * 1e3, 3),
            "rel_min": float(np.nanmin(rel)), "rel_max": float(np.nanmax(rel)), "finite": bool(np.all(np.isfinite(rel))),
            "note": "the call is the whole evaluation plus k_reliab and the D2H copy of the reliabilities; "
                    "the kernel alone: --stats; the floor is derived (flop / measured fp64 MFMA peak)"}


def score_vs_reliability(eng, genomes, T, V, n, P, ns, reps, n_cand=2000):
    """snp_scores() of n_cand SNPs under every model and of all P SNPs under one model, against
    reliability() of n_cand animals (as many right-hand sides) and evaluate(), alternated on one engine."""
    rng = np.random.default_rng(99)
    cand = rng.choice(P, n_cand, replace=False)
    an = rng.choice(n, n_cand, replace=n_cand > n)
    te, tr, ts, t1 = [], [], [], []
    for r in range(reps + 2):
        t = [time.perf_counter()]
        eng.evaluate(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        eng.reliability(genomes, T, V, 0.4, an)
        t.append(time.perf_counter())
        sc = eng.snp_scores(genomes, T, V, 0.4, cand)
        t.append(time.perf_counter())
        one = eng.snp_scores(genomes[:1], T, V, 0.4)
        t.append(time.perf_counter())
        if r >= 2:
            for lst, i in ((te, 0), (tr, 1), (ts, 2), (t1, 3)):
                lst.append(t[i + 1] - t[i])
    B = len(genomes)
    flop, flop1 = float(B) * n_cand * ns * ns, float(P) * ns * ns
    floor = lambda f: round(f / (F64_MFMA_TFS * 1e12) * 1e3, 3)
    return {"evaluate_ms": med_ms(te), "reliability_ms": med_ms(tr), "score_ms": med_ms(ts),
            "score_extra_ms_over_evaluate": round(med_ms(ts) - med_ms(te), 4),
            "reliability_extra_ms_over_evaluate": round(med_ms(tr) - med_ms(te), 4),
            "score_over_reliability_extra": round((med_ms(ts) - med_ms(te)) / (med_ms(tr) - med_ms(te)), 4),
            "score_floor_ms": floor(flop), "n_cand": n_cand,
            "score_1xP_ms": med_ms(t1), "score_1xP_floor_ms": floor(flop1),
            "score_ms_all": [round(x * 1e3, 3) for x in ts], "reliability_ms_all": [round(x * 1e3, 3) for x in tr],
            "score_1xP_ms_all": [round(x * 1e3, 3) for x in t1],
            "finite": bool(np.all(np.isfinite(sc.score)) and np.all(np.isfinite(one.score))),
            "max_chi2_1xP": float(np.nanmax(one.chi2())),
            "note": "each call is the whole evaluation plus the kernel and the D2H copy of its outputs; the "
                    "kernels alone: --stats; the floors are derived (flop / measured fp64 MFMA peak)"}


def covar_vs_fit(eng, genomes, T, V, n, P, reps, n_cov=16):
    """fit(covariates=) with n_cov covariates against fit() and snp_scores() of n_cov listed SNPs (one slab per
    model through the same substitution), alternated on one engine."""
    rng = np.random.default_rng(77)
    q = rng.standard_normal((n, n_cov))
    q[:, 0] = rng.random(n) < 0.5
    cand = rng.choice(P, n_cov, replace=False)
    tf, tc, ts = [], [], []
    for r in range(reps + 2):
        t = [time.perf_counter()]
        plain = eng.fit(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        models = eng.fit(genomes, T, V, 0.4, covariates=q)
        t.append(time.perf_counter())
        eng.snp_scores(genomes, T, V, 0.4, cand)
        t.append(time.perf_counter())
        if r >= 2:
            for lst, i in ((tf, 0), (tc, 1), (ts, 2)):
                lst.append(t[i + 1] - t[i])
    return {"fit_ms": med_ms(tf), "fit_cov_ms": med_ms(tc), "score_16_ms": med_ms(ts), "n_cov": n_cov,
            "extra_ms_over_fit": round(med_ms(tc) - med_ms(tf), 4),
            "fit_ms_all": [round(x * 1e3, 3) for x in tf], "fit_cov_ms_all": [round(x * 1e3, 3) for x in tc],
            "score_16_ms_all": [round(x * 1e3, 3) for x in ts],
            "finite": bool(all(np.all(np.isfinite(m.cov_effects)) for m in models)),
            "fitness_plain_median": float(np.median([m.fitness for m in plain])),
            "fitness_cov_median": float(np.median([m.fitness for m in models])),
            "note": "each call is the whole evaluation plus its kernels, the D2H copies and the PanelModel objects; "
                    "the covariate call runs the one-workgroup k_solve twice (no chained solve); the kernels alone: "
                    "--stats"}


def group_vs_fit(eng, genomes, T, V, n, reps):
    """fit(groups=) at 64 levels and at 112 levels + 16 covariates against fit(covariates=16 columns) and fit(),
    alternated on one engine.  Labels uniform over the levels, every level on a train animal."""
    q = bench_cov(n)
    g64, g112 = bench_groups(n, T)
    ts = {"fit_ms": [], "fit_cov16_ms": [], "fit_group64_ms": [], "fit_group112_cov16_ms": []}
    for r in range(reps + 2):
        t = [time.perf_counter()]
        eng.fit(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        eng.fit(genomes, T, V, 0.4, covariates=q)
        t.append(time.perf_counter())
        m64 = eng.fit(genomes, T, V, 0.4, groups=g64)
        t.append(time.perf_counter())
        m128 = eng.fit(genomes, T, V, 0.4, covariates=q, groups=g112)
        t.append(time.perf_counter())
        if r >= 2:
            for i, key in enumerate(ts):
                ts[key].append(t[i + 1] - t[i])
    out = {k: med_ms(v) for k, v in ts.items()}
    out.update({k + "_all": [round(x * 1e3, 3) for x in v] for k, v in ts.items()})
    out["columns"] = {"group64": 63, "group112_cov16": 127}
    out["finite"] = bool(all(np.all(np.isfinite(m.group_effects)) for m in m64 + m128))
    out["note"] = ("each call is the whole evaluation plus its kernels, the D2H copies and the PanelModel objects; the "
                   "covariate and group calls run the one-workgroup k_solve twice; the kernels alone: --stats")
    return out


def bench_groups(n, T):
    """group_vs_fit's labels: 64 and 112 levels, uniform, every level on a train animal."""
    rng = np.random.default_rng(78)
    g64, g112 = rng.integers(0, 64, n), rng.integers(0, 112, n)
    g64[T[:64]], g112[T[:112]] = np.arange(64), np.arange(112)
    return g64, g112


def score_group_vs_score(eng, genomes, T, V, n, P, ns, reps, n_cand=2000):
    """snp_scores_group() at 64 levels and at 112 levels + 16 covariates against snp_scores() and
    snp_scores(covariates=16 columns) on score_vs_reliability's list, and evaluate(), alternated."""
    cand = np.random.default_rng(99).choice(P, n_cand, replace=False)
    q = bench_cov(n)
    g64, g112 = bench_groups(n, T)
    ts = {"evaluate_ms": [], "score_ms": [], "score_cov16_ms": [], "score_group64_ms": [], "score_group112_cov16_ms": []}
    for r in range(reps + 2):
        t = [time.perf_counter()]
        eng.evaluate(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        plain = eng.snp_scores(genomes, T, V, 0.4, cand)
        t.append(time.perf_counter())
        eng.snp_scores(genomes, T, V, 0.4, cand, covariates=q)
        t.append(time.perf_counter())
        s64 = eng.snp_scores_group(genomes, T, V, 0.4, g64, cand)
        t.append(time.perf_counter())
        s128 = eng.snp_scores_group(genomes, T, V, 0.4, g112, cand, covariates=q)
        t.append(time.perf_counter())
        if r >= 2:
            for i, key in enumerate(ts):
                ts[key].append(t[i + 1] - t[i])
    out = {k: med_ms(v) for k, v in ts.items()}
    out.update({k + "_all": [round(x * 1e3, 3) for x in v] for k, v in ts.items() if k != "evaluate_ms"})
    share = lambda c: round(2.0 * c / ns + float(c) * c / (ns * ns), 4)
    out.update({"n_cand": n_cand, "columns": {"cov16": 16, "group64": 63, "group112_cov16": 127},
                "over_score": {k: round(out[k + "_ms"] / out["score_ms"], 4)
                               for k in ("score_cov16", "score_group64", "score_group112_cov16")},
                "derived_flop_share": {"cov16": share(16), "group64": share(63), "group112_cov16": share(127)},
                "slab_launch_workgroups": len(genomes) * ((n_cand + 15) // 16),
                "finite": bool(all(np.all(np.isfinite(s.score)) and np.all(np.isfinite(s.info)) for s in (s64, s128))),
                "median_info_ratio": {"group64": float(np.median(s64.info / plain.info)),
                                      "group112_cov16": float(np.median(s128.info / plain.info))},
                "note": "each call is the whole evaluation plus its kernels and the D2H copy of its outputs; a group "
                        "call adds one k_fixed_subst and one k_fixed_gls (keep mode) launch per chunk; the kernels "
                        "alone: --stats"})
    return out


def loglik_group_vs_cov(eng, genomes, T, V, n, reps, grid_n=8):
    """tblup_loglik_group_batch at 64 levels and at 112 levels + 16 covariates against tblup_loglik_cov_batch at
    grid_n grid points (the C entries) and fit(groups=) at both designs, alternated; one estimate_h2_group."""
    from tblup_amd.engine import concat_genomes
    from tblup_amd import _native
    _ptr = _native.ptr
    sid = eng.split_id(T, V)
    idx, off = concat_genomes(genomes)
    B, nt = len(genomes), eng.n_traits
    q = np.ascontiguousarray(bench_cov(n))
    g64, g112 = (np.ascontiguousarray(g, dtype=np.int64) for g in bench_groups(n, T))
    hg = np.ascontiguousarray(np.repeat(np.linspace(0.1, 0.8, grid_n)[:, None], B, axis=1))
    ll = {k: np.empty((grid_n, B, nt)) for k in ("cov", "g64", "g128")}
    s2 = np.empty((grid_n, B, nt))

    def group(codes, L, cov, nc, out):
        _native.check("tblup_loglik_group_batch", eng._lib.tblup_loglik_group_batch(
            eng._ctx, sid, _ptr(cov) if nc else None, nc, _ptr(codes), L, _ptr(idx), _ptr(off), B, _ptr(hg), grid_n, 0,
            None, _ptr(out), _ptr(s2), None, None))

    ts = {"loglik_cov16": [], "loglik_group64": [], "loglik_group112_cov16": [], "fit_group64": [],
          "fit_group112_cov16": []}
    for r in range(reps + 2):
        t = [time.perf_counter()]
        _native.check("tblup_loglik_cov_batch", eng._lib.tblup_loglik_cov_batch(
            eng._ctx, sid, _ptr(q), 16, _ptr(idx), _ptr(off), B, _ptr(hg), grid_n, 0, None, _ptr(ll["cov"]), _ptr(s2),
            None))
        t.append(time.perf_counter())
        group(g64, 64, None, 0, ll["g64"])
        t.append(time.perf_counter())
        group(g112, 112, q, 16, ll["g128"])
        t.append(time.perf_counter())
        eng.fit(genomes, T, V, 0.4, groups=g64)
        t.append(time.perf_counter())
        eng.fit(genomes, T, V, 0.4, covariates=q, groups=g112)
        t.append(time.perf_counter())
        if r >= 2:
            for i, key in enumerate(ts):
                ts[key].append(t[i + 1] - t[i])
    t0 = time.perf_counter()
    est = eng.estimate_h2_group(genomes, T, V, g64)
    t_est = time.perf_counter() - t0
    out = {}
    for k, v in ts.items():
        if k.startswith("loglik"):
            out[k + "_%d_ms" % grid_n] = med_ms(v)
            out[k + "_per_grid_point_ms"] = round(med_ms(v) / grid_n, 4)
        else:
            out[k + "_ms"] = med_ms(v)
        out[k + "_ms_all"] = [round(x * 1e3, 3) for x in v]
    out.update({"finite": bool(all(np.all(np.isfinite(a)) for a in ll.values())),
                "estimate_h2_group_ms": round(t_est * 1e3, 2), "estimate_h2_passes": 25 + 3 * 9,
                "estimate_h2_group_ms_per_pass": round(t_est * 1e3 / (25 + 3 * 9), 3),
                "h2_median": float(np.nanmedian(est["h2"])), "at_bound": int(np.sum(est["at_bound"])),
                "note": "every call ends in the stream's synchronisation; a group pass adds one k_fixed_subst and one "
                        "k_fixed_gls (keep mode, no z*) launch; fit(groups=) is one pass with the second solve and the "
                        "PanelModel objects; the kernels alone: --stats"})
    return out


def bench_cov(n, n_cov=16):
    """The covariates of the score_cov / loglik_cov parts (covar_vs_fit's draw)."""
    rng = np.random.default_rng(77)
    q = rng.standard_normal((n, n_cov))
    q[:, 0] = rng.random(n) < 0.5
    return q


def score_cov_vs_score(eng, genomes, T, V, n, P, ns, reps, n_cand=2000, n_cov=16):
    """snp_scores(covariates=Q) against snp_scores() on score_vs_reliability's list, and evaluate(), alternated."""
    cand = np.random.default_rng(99).choice(P, n_cand, replace=False)
    q = bench_cov(n, n_cov)
    te, ts, tc = [], [], []
    for r in range(reps + 2):
        t = [time.perf_counter()]
        eng.evaluate(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        plain = eng.snp_scores(genomes, T, V, 0.4, cand)
        t.append(time.perf_counter())
        adj = eng.snp_scores(genomes, T, V, 0.4, cand, covariates=q)
        t.append(time.perf_counter())
        if r >= 2:
            for lst, i in ((te, 0), (ts, 1), (tc, 2)):
                lst.append(t[i + 1] - t[i])
    nslab = (n_cand + 15) // 16
    return {"evaluate_ms": med_ms(te), "score_ms": med_ms(ts), "score_cov_ms": med_ms(tc), "n_cand": n_cand,
            "n_cov": n_cov, "score_cov_over_score": round(med_ms(tc) / med_ms(ts), 4),
            "extra_over_evaluate_ratio": round((med_ms(tc) - med_ms(te)) / (med_ms(ts) - med_ms(te)), 4),
            "derived_flop_share": round(32.0 / ns, 4), "slab_launch_workgroups": len(genomes) * nslab,
            "score_ms_all": [round(x * 1e3, 3) for x in ts], "score_cov_ms_all": [round(x * 1e3, 3) for x in tc],
            "finite": bool(np.all(np.isfinite(adj.score)) and np.all(np.isfinite(adj.info))),
            "median_info_ratio": float(np.median(adj.info / plain.info)),
            "note": "each call is the whole evaluation plus its kernels and the D2H copy of its outputs; the adjusted "
                    "call adds one k_covar launch per chunk; the kernels alone: --stats"}


def reliab_cov_vs_reliab(eng, genomes, T, V, n, ns, reps, n_cov=16):
    """reliability_cov(covariates=Q) against reliability() for all n animals, and evaluate(), alternated."""
    herd = np.arange(n)
    q = bench_cov(n, n_cov)
    te, tr, tc = [], [], []
    for r in range(reps + 2):
        t = [time.perf_counter()]
        eng.evaluate(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        plain = eng.reliability(genomes, T, V, 0.4, herd)
        t.append(time.perf_counter())
        adj = eng.reliability_cov(genomes, T, V, 0.4, herd, covariates=q, return_pev=True, return_cov_cov=True)
        t.append(time.perf_counter())
        if r >= 2:
            for lst, i in ((te, 0), (tr, 1), (tc, 2)):
                lst.append(t[i + 1] - t[i])
    nslab = (n + 15) // 16
    return {"evaluate_ms": med_ms(te), "reliability_ms": med_ms(tr), "reliability_cov_ms": med_ms(tc), "animals": n,
            "n_cov": n_cov, "reliab_cov_over_reliab": round(med_ms(tc) / med_ms(tr), 4),
            "extra_over_evaluate_ratio": round((med_ms(tc) - med_ms(te)) / (med_ms(tr) - med_ms(te)), 4),
            "derived_flop_share": round(32.0 / ns, 4), "slab_launch_workgroups": len(genomes) * nslab,
            "reliability_ms_all": [round(x * 1e3, 3) for x in tr], "reliability_cov_ms_all": [round(x * 1e3, 3) for x in tc],
            "finite": bool(np.all(np.isfinite(adj.reliability)) and np.all(np.isfinite(adj.pev_total))
                           and np.all(np.isfinite(adj.cov_cov))),
            "never_above_plain": bool(np.all(adj.reliability <= plain + 1e-9)),
            "median_reliability_drop": float(np.median(plain - adj.reliability)),
            "note": "each call is the whole evaluation plus its kernels and the D2H copy of its outputs; the adjusted "
                    "call adds one k_covar launch (keep mode, no z*) and one k_cov_cov launch per chunk; the kernels "
                    "alone: --stats"}


def reliab_group_vs_reliab(eng, genomes, T, V, n, ns, reps):
    """reliability_group() at 64 levels and at 112 levels + 16 covariates against reliability(),
    reliability_cov(covariates=16 columns), fit(groups=) at both designs and evaluate(), for all n animals, alternated."""
    herd = np.arange(n)
    q = bench_cov(n)
    g64, g112 = bench_groups(n, T)
    want = dict(return_pev=True, return_fixed_cov=True)
    ts = {"evaluate_ms": [], "reliability_ms": [], "reliability_cov16_ms": [], "reliability_group64_ms": [],
          "reliability_group112_cov16_ms": [], "fit_group64_ms": [], "fit_group112_cov16_ms": []}
    for r in range(reps + 2):
        t = [time.perf_counter()]
        eng.evaluate(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        plain = eng.reliability(genomes, T, V, 0.4, herd)
        t.append(time.perf_counter())
        rc = eng.reliability_cov(genomes, T, V, 0.4, herd, covariates=q, return_pev=True, return_cov_cov=True)
        t.append(time.perf_counter())
        r64 = eng.reliability_group(genomes, T, V, 0.4, herd, g64, **want)
        t.append(time.perf_counter())
        r128 = eng.reliability_group(genomes, T, V, 0.4, herd, g112, covariates=q, **want)
        t.append(time.perf_counter())
        eng.fit(genomes, T, V, 0.4, groups=g64)
        t.append(time.perf_counter())
        eng.fit(genomes, T, V, 0.4, covariates=q, groups=g112)
        t.append(time.perf_counter())
        if r >= 2:
            for i, key in enumerate(ts):
                ts[key].append(t[i + 1] - t[i])
    out = {k: med_ms(v) for k, v in ts.items()}
    out.update({k + "_all": [round(x * 1e3, 3) for x in v] for k, v in ts.items() if k != "evaluate_ms"})
    share = lambda c: round(2.0 * c / ns + 2.0 * c * c / (ns * ns), 4)
    names = ("reliability_cov16", "reliability_group64", "reliability_group112_cov16")
    out.update({"animals": n, "columns": {"cov16": 16, "group64": 63, "group112_cov16": 127},
                "over_reliability": {k: round(out[k + "_ms"] / out["reliability_ms"], 4) for k in names},
                "derived_flop_share": {"cov16": share(16), "group64": share(63), "group112_cov16": share(127)},
                "slab_launch_workgroups": len(genomes) * ((n + 15) // 16),
                "finite": bool(all(np.all(np.isfinite(getattr(x, f))) for x in (r64, r128)
                                   for f in ("reliability", "pev_total", "fixed_cov"))),
                "never_above_cov": bool(np.all(r128.reliability <= rc.reliability + 1e-9)),
                "median_reliability_drop": {"cov16": float(np.median(plain - rc.reliability)),
                                            "group64": float(np.median(plain - r64.reliability)),
                                            "group112_cov16": float(np.median(plain - r128.reliability))},
                "note": "each call is the whole evaluation plus its kernels and the D2H copy of its outputs; a group "
                        "call adds one k_fixed_subst, one k_fixed_gls (keep mode, no z*) and one k_fixed_cov launch per "
                        "chunk; the kernels alone: --stats"})
    return out


def loo_vs_reliability(eng, genomes, T, V, ns, reps, folds=5):
    """loo() against reliability() of the n_T training animals (as many right-hand sides through the same
    substitution), evaluate() and the `folds`-fold IntraGCV entry (evaluate_folds on a partition of T), alternated
    on one engine."""
    T = np.asarray(T)
    parts = np.array_split(T, folds)
    splits = [(np.concatenate([p for j, p in enumerate(parts) if j != f]), parts[f]) for f in range(folds)]
    ts = {"evaluate_ms": [], "reliability_nT_ms": [], "loo_ms": [], "folds_ms": []}
    res = None
    for r in range(reps + 2):
        t = [time.perf_counter()]
        fit = eng.evaluate(genomes, T, V, 0.4)
        t.append(time.perf_counter())
        eng.reliability(genomes, T, V, 0.4, T)
        t.append(time.perf_counter())
        res = eng.loo(genomes, T, V, 0.4, return_leverage=True)
        t.append(time.perf_counter())
        cv = eng.evaluate_folds(genomes, splits, 0.4)
        t.append(time.perf_counter())
        if r >= 2:
            for i, key in enumerate(ts):
                ts[key].append(t[i + 1] - t[i])
    out = {k: med_ms(v) for k, v in ts.items()}
    out.update({k + "_all": [round(x * 1e3, 3) for x in v] for k, v in ts.items()})
    B, nT = len(genomes), len(T)
    flop = float(B) * nT * ns * ns
    out.update({"right_hand_sides": nT, "folds": folds,
                "loo_extra_ms_over_evaluate": round(out["loo_ms"] - out["evaluate_ms"], 4),
                "reliability_extra_ms_over_evaluate": round(out["reliability_nT_ms"] - out["evaluate_ms"], 4),
                "loo_over_evaluate": round(out["loo_ms"] / out["evaluate_ms"], 4),
                "folds_over_evaluate": round(out["folds_ms"] / out["evaluate_ms"], 4),
                "substitution_flop": flop, "substitution_floor_ms": round(flop / (F64_MFMA_TFS * 1e12) * 1e3, 3),
                "slab_launch_workgroups": B * ((nT + 15) // 16),
                "eval_fitness_bit_equal": bool(np.array_equal(res.eval_fitness, fit, equal_nan=True)),
                "finite": bool(np.all(np.isfinite(res.pred)) and np.all(np.isfinite(res.leverage))),
                "loo_fitness_median": float(np.nanmedian(res.fitness)),
                "folds_fitness_median": float(np.nanmedian(cv.mean(axis=0))),
                "evaluate_fitness_median": float(np.nanmedian(fit)),
                "leverage_max": float(np.nanmax(res.leverage)),
                "note": "each call is the whole evaluation plus its kernels and the D2H copy of its outputs; loo adds "
                        "k_effects (the solution alone), k_loo and k_loo_fitness; the floor is derived for the full "
                        "substitution (flop / measured fp64 MFMA peak; the kernel form's unit columns need half of it); "
                        "the kernels alone: --stats"})
    return out


def loglik_cov_vs_loglik(eng, genomes, T, V, n, reps, grid_n=8, n_cov=16):
    """tblup_loglik_cov_batch against tblup_loglik_batch at grid_n grid points (the C entries, alternated)."""
    from tblup_amd.engine import concat_genomes
    from tblup_amd import _native
    _ptr = _native.ptr
    sid = eng.split_id(T, V)
    idx, off = concat_genomes(genomes)
    B, nt = len(genomes), eng.n_traits
    q = np.ascontiguousarray(bench_cov(n, n_cov))
    hg = np.ascontiguousarray(np.repeat(np.linspace(0.1, 0.8, grid_n)[:, None], B, axis=1))
    ll, s2 = np.empty((grid_n, B, nt)), np.empty((grid_n, B, nt))
    llc, s2c = np.empty((grid_n, B, nt)), np.empty((grid_n, B, nt))
    tp, tc = [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        _native.check("tblup_loglik_batch", eng._lib.tblup_loglik_batch(
            eng._ctx, sid, _ptr(idx), _ptr(off), B, _ptr(hg), grid_n, 0, None, _ptr(ll), _ptr(s2)))
        t1 = time.perf_counter()
        _native.check("tblup_loglik_cov_batch", eng._lib.tblup_loglik_cov_batch(
            eng._ctx, sid, _ptr(q), n_cov, _ptr(idx), _ptr(off), B, _ptr(hg), grid_n, 0, None, _ptr(llc), _ptr(s2c), None))
        t2 = time.perf_counter()
        if r >= 2:
            tp.append(t1 - t0)
            tc.append(t2 - t1)
    return {"loglik_%d_ms" % grid_n: med_ms(tp), "loglik_cov_%d_ms" % grid_n: med_ms(tc), "n_cov": n_cov,
            "per_grid_point_ms": round(med_ms(tp) / grid_n, 4), "per_grid_point_cov_ms": round(med_ms(tc) / grid_n, 4),
            "extra_per_point_ms": round((med_ms(tc) - med_ms(tp)) / grid_n, 4),
            "loglik_ms_all": [round(x * 1e3, 3) for x in tp], "loglik_cov_ms_all": [round(x * 1e3, 3) for x in tc],
            "finite": bool(np.all(np.isfinite(llc)) and np.all(np.isfinite(s2c))),
            "note": "every call ends in the stream's synchronisation; the adjusted call adds one k_covar launch "
                    "(keep mode, no z*) per pass; the kernels alone: --stats"}


def loglik_vs_eval(eng, genomes, T, V, reps, grid_n=8):
    """tblup_eval_batch against tblup_loglik_batch at 1 and grid_n grid points (the C entries, alternated),
    then one estimate_h2 with the defaults."""
    from tblup_amd.engine import concat_genomes
    from tblup_amd import _native
    _ptr = _native.ptr
    sid = eng.split_id(T, V)
    idx, off = concat_genomes(genomes)
    B, nt = len(genomes), eng.n_traits
    fit = np.empty(B)
    h1 = np.full((1, B), 0.4)
    hg = np.ascontiguousarray(np.repeat(np.linspace(0.1, 0.8, grid_n)[:, None], B, axis=1))
    fl, ll, s2 = np.empty((grid_n, B)), np.empty((grid_n, B, nt)), np.empty((grid_n, B, nt))

    def loglik(h):
        _native.check("tblup_loglik_batch", eng._lib.tblup_loglik_batch(
            eng._ctx, sid, _ptr(idx), _ptr(off), B, _ptr(h), len(h), 0, _ptr(fl), _ptr(ll), _ptr(s2)))

    te, t1s, tgs = [], [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        _native.check("tblup_eval_batch", eng._lib.tblup_eval_batch(eng._ctx, sid, _ptr(idx), _ptr(off), B, 0.4, 0,
                                                                    _ptr(fit), None))
        t1 = time.perf_counter()
        loglik(h1)
        t2 = time.perf_counter()
        same = bool(np.array_equal(fl[0], fit, equal_nan=True))
        t2b = time.perf_counter()
        loglik(hg)
        t3 = time.perf_counter()
        if r >= 2:
            te.append(t1 - t0)
            t1s.append(t2 - t1)
            tgs.append(t3 - t2b)
    t0 = time.perf_counter()
    est = eng.estimate_h2(genomes, T, V)
    t_est = time.perf_counter() - t0
    return {"eval_batch_ms": med_ms(te), "loglik_1_ms": med_ms(t1s), "loglik_%d_ms" % grid_n: med_ms(tgs),
            "per_grid_point_ms": round(med_ms(tgs) / grid_n, 4),
            "extra_per_point_ms": round(med_ms(tgs) / grid_n - med_ms(te), 4),
            "extra_single_ms": round(med_ms(t1s) - med_ms(te), 4),
            "eval_batch_ms_all": [round(x * 1e3, 3) for x in te], "loglik_1_ms_all": [round(x * 1e3, 3) for x in t1s],
            "loglik_%d_ms_all" % grid_n: [round(x * 1e3, 3) for x in tgs], "fitness_bit_equal": same,
            "finite": bool(np.all(np.isfinite(ll))),
            "estimate_h2_ms": round(t_est * 1e3, 2), "estimate_h2_passes": 25 + 3 * 9,
            "estimate_h2_ms_per_pass": round(t_est * 1e3 / (25 + 3 * 9), 3),
            "h2_median": float(np.nanmedian(est["h2"])), "at_bound": int(np.sum(est["at_bound"])),
            "note": "every call ends in the stream's synchronisation; the grid call uploads the index lists once "
                    "and copies the results out after the last pass; k_loglik alone: --stats"}


def stats_share(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"part": "rocprof", "total_kernel_ms": round(tot / 1e6, 3), "kernels": {}}
    for r in rows:
        name = r["Name"]
        # the covariate-adjusted k_reliab instances and k_covar's keep mode (third template argument) apart
        # ... k_fixed_gls's keep mode (second) and k_snpscore's 16-column and wide instances (third: 1, 2) too
        # (k_reliab's third argument: true in traces from before its wide instances, then 1 and 2 as k_snpscore's)
        for key, alias, last in (("k_reliab", "k_reliab_cov", "true"), ("k_reliab", "k_reliab_cov", "1"),
                                 ("k_reliab", "k_reliab_fix", "2"), ("k_covar", "k_covar_keep", "true"),
                                 ("k_fixed_gls", "k_fixed_gls_keep", "true"), ("k_snpscore", "k_snpscore_cov", "1"),
                                 ("k_snpscore", "k_snpscore_fix", "2")):
            if key + "<" in name and name.split(key + "<")[1].split(">")[0].replace(" ", "").endswith("," + last):
                name = name.replace(key + "<", alias + "<")
        for key in ("k_loo_fitness", "k_loo", "k_reliab_cov", "k_reliab_fix", "k_fixed_cov", "k_covar_keep", "k_cov_cov", "k_fixed_gls_keep", "k_snpscore_cov", "k_snpscore_fix", "k_fixed_subst", "k_fixed_gls", "k_fixed_fitness", "k_effects", "k_predict", "k_reliab", "k_snpscore", "k_loglik", "k_covar", "k_cov_fitness", "k_solve", "k_chol_offdiag", "k_chol_diag"):
            if key + "<" in name or key + "(" in name:
                e = out["kernels"].setdefault(key, {"calls": 0, "total_ms": 0.0})
                e["calls"] += int(r["Calls"])
                e["total_ms"] = round(e["total_ms"] + float(r["TotalDurationNs"]) / 1e6, 4)
    for e in out["kernels"].values():
        e["avg_us"] = round(e["total_ms"] * 1e3 / max(e["calls"], 1), 2)
        e["share"] = round(e["total_ms"] * 1e6 / tot, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="fit,predict,dual")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stats", default=None, help="kernel_stats CSV of a rocprofv3 --kernel-trace --stats run")
    args = ap.parse_args()
    if args.stats:
        print(json.dumps(stats_share(args.stats)))
        return
    parts = set(args.only.split(","))
    from tblup_amd.engine import GpuBlupEngine
    if parts & {"fit", "predict"}:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            models, st = fit_vs_eval(eng, genomes, T, V, args.reps)
            if "fit" in parts:
                print(json.dumps({"part": "fit", "config": "config2", **st, "c_abi": fit_raw(eng, genomes, T, V, args.reps)}))
            if "predict" in parts:
                out, sp = predict_all(eng, models, n, args.reps)
                host = models[0].predict(geno)
                sp["max_rel_vs_numpy_model0"] = float(np.max(np.abs(out[0] - host)) / np.max(np.abs(host)))
                print(json.dumps({"part": "predict", "config": "config2", "models": pop, "k": k, "animals": n, **sp}))
    if "reliability" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            st = reliability_all(eng, genomes, T, V, n, 1024, args.reps)
            print(json.dumps({"part": "reliability", "config": "config2", "models": pop, "k": k, "animals": n,
                              "form": "snp", "ns": 1024, **st}))
        n, P, k, pop, nT, nV = 1200, 20_000, 1500, 32, 768, 192
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            st = reliability_all(eng, genomes, T, V, n, 768, args.reps)
            print(json.dumps({"part": "reliability", "config": "config4-shaped stand-in: %d x %d, k=%d (gblup), n_T=%d"
                              % (n, P, k, nT), "models": pop, "k": k, "animals": n, "form": "kernel", "ns": 768, **st}))
    if "loglik" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            st = loglik_vs_eval(eng, genomes, T, V, args.reps)
            print(json.dumps({"part": "loglik", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **st}))
    if "score" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            st = score_vs_reliability(eng, genomes, T, V, n, P, 1024, args.reps)
            print(json.dumps({"part": "score", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **st}))
    if "covar" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            st = covar_vs_fit(eng, genomes, T, V, n, P, args.reps)
            print(json.dumps({"part": "covar", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **st}))
    if "group" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            print(json.dumps({"part": "group", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **group_vs_fit(eng, genomes, T, V, n, args.reps)}))
    if parts & {"score_cov", "loglik_cov"}:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            head = {"config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024}
            if "score_cov" in parts:
                print(json.dumps({"part": "score_cov", **head,
                                  **score_cov_vs_score(eng, genomes, T, V, n, P, 1024, args.reps)}))
            if "loglik_cov" in parts:
                print(json.dumps({"part": "loglik_cov", **head, **loglik_cov_vs_loglik(eng, genomes, T, V, n, args.reps)}))
    if parts & {"score_group", "loglik_group"}:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            head = {"config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024}
            if "score_group" in parts:
                print(json.dumps({"part": "score_group", **head,
                                  **score_group_vs_score(eng, genomes, T, V, n, P, 1024, args.reps)}), flush=True)
            if "loglik_group" in parts:
                print(json.dumps({"part": "loglik_group", **head,
                                  **loglik_group_vs_cov(eng, genomes, T, V, n, args.reps)}), flush=True)
    if "reliab_cov" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            print(json.dumps({"part": "reliab_cov", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **reliab_cov_vs_reliab(eng, genomes, T, V, n, 1024, args.reps)}))
    if "reliab_group" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            print(json.dumps({"part": "reliab_group", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **reliab_group_vs_reliab(eng, genomes, T, V, n, 1024, args.reps)}), flush=True)
    if "loo" in parts:
        n, P, k, pop, nT, nV = 2000, 50_000, 1000, 256, 1280, 320
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            print(json.dumps({"part": "loo", "config": "config2", "models": pop, "k": k, "form": "snp", "ns": 1024,
                              **loo_vs_reliability(eng, genomes, T, V, 1024, args.reps)}), flush=True)
        n, P, k, pop, nT, nV = 1200, 20_000, 1500, 32, 768, 192
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            print(json.dumps({"part": "loo", "config": "config4-shaped stand-in: %d x %d, k=%d (gblup), n_T=%d"
                              % (n, P, k, nT), "models": pop, "k": k, "form": "kernel", "ns": 768,
                              **loo_vs_reliability(eng, genomes, T, V, 768, args.reps)}), flush=True)
    if "dual" in parts:
        n, P, k, pop, nT, nV = 1200, 20_000, 1500, 32, 768, 192
        geno, pheno, T, V, genomes = workload(n, P, k, pop, nT, nV)
        with GpuBlupEngine(geno, pheno) as eng:
            models, st = fit_vs_eval(eng, genomes, T, V, args.reps)
            _, sp = predict_all(eng, models, n, args.reps)
            print(json.dumps({"part": "dual", "config": "config4-shaped stand-in: %d x %d, k=%d (gblup), n_T=%d, pop %d"
                              % (n, P, k, nT, pop), **st, "c_abi": fit_raw(eng, genomes, T, V, args.reps), "predict": sp}))


if __name__ == "__main__":
    main()
