"""Generate tests/golden/model.npz from the upstream reference (ianwhale/tblup): the model the
reference fits inside blup() and never returns.

Run ONLY in the build container, where the read-only reference is mounted at /root/reference:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_model_golden.py

  snp    `BlupParallelEvaluator.snp_blup` is called as it stands, with a recorder around
         `Ridge.fit` that copies the fitted `coef_` and `intercept_` (evaluator.py:311-312).
  gblup  the all-animal `prediction` of evaluator.py:284 (which the reference indexes by the
         validation rows and drops), from the reference's own `make_grm` (utils.py:7-18).

Data only (inputs and recorded outputs), a few KB; no reference source.
"""
import os
import sys

import numpy as np

REF = os.environ.get("TBLUP_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

if not hasattr(np, "asscalar"):   # numpy >= 1.23 removed it; the reference's monitor calls it
    np.asscalar = lambda a: a.item()

import tblup.evaluator as ref_ev  # noqa: E402  (reference package)
from tblup.utils import make_grm  # noqa: E402


class RidgeRecorder:
    """Records (coef_, intercept_) of every Ridge the reference fits while it is active."""

    def __init__(self):
        self.fits = []

    def __enter__(self):
        self.orig = ref_ev.Ridge.fit
        rec = self

        def fit(est, X, y, *args, **kw):
            out = rec.orig(est, X, y, *args, **kw)
            rec.fits.append((np.array(est.coef_, dtype=np.float64), float(est.intercept_)))
            return out

        ref_ev.Ridge.fit = fit
        return self

    def __exit__(self, *exc):
        ref_ev.Ridge.fit = self.orig


def main():
    rng = np.random.default_rng(20261019)
    n, P, h2 = 48, 90, 0.4
    maf = rng.uniform(0.05, 0.5, size=P)
    geno = rng.binomial(2, maf, size=(n, P)).astype(np.int8)
    pheno = rng.standard_normal(n)
    perm = rng.permutation(n)
    T, V = perm[:30], perm[30:41]
    data = geno.astype(np.float64)
    out = {"geno": geno, "pheno": pheno, "T": T, "V": V, "h2": np.float64(h2)}
    # snp: k <= n_T (Ridge's primal solve), n_T < k <= n (its kernel solve), duplicates
    snp = {"snp_k1": rng.choice(P, 1), "snp_k12": rng.choice(P, 12, replace=False),
           "snp_k30": rng.choice(P, 30, replace=False), "snp_k44": rng.choice(P, 44, replace=False),
           "snp_dup": np.concatenate([rng.choice(P, 9, replace=False)] * 2)}
    for name, idx in snp.items():
        with RidgeRecorder() as rec:
            fit = ref_ev.BlupParallelEvaluator.snp_blup(idx, T, V, data.copy(), pheno, h2)
        (coef, intercept), = rec.fits
        out[name + "_idx"], out[name + "_coef"] = idx, coef
        out[name + "_intercept"], out[name + "_fit"] = np.float64(intercept), np.float64(fit)
    # gblup: k > n (the reference's own dispatch) and k <= n
    gb = {"gblup_k70": rng.choice(P, 70, replace=False), "gblup_k20": rng.choice(P, 20, replace=False),
          "gblup_k200": rng.integers(0, P, 200)}
    r = (1 - h2) / h2
    for name, idx in gb.items():
        G = make_grm(data[:, idx])
        G_inv = G[T, :][:, T]
        G_inv.flat[:: G_inv.shape[0] + 1] += r
        G_inv = np.linalg.inv(G_inv)
        out[name + "_idx"] = idx
        out[name + "_pred"] = np.matmul(np.matmul(G[:, T], G_inv), pheno[T])
        out[name + "_fit"] = np.float64(ref_ev.BlupParallelEvaluator.gblup(idx, T, V, data.copy(), pheno, h2))
    path = os.path.join(HERE, "model.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
