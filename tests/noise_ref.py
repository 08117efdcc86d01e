"""The noise estimate's formulas (include/rt2.h "Noise estimate", raytrace2_amd/csrc/noise.h) in numpy
float64, shared by the host test and the GPU tests. numpy rounds every operation on its own (no fused
multiply-add) and its float64 sqrt is correctly rounded, so the product must match bit for bit."""
import numpy as np


def noise_ref(a, q, n):
    """a, q: float32 (..., 3) sums of the samples and of their squares over n >= 2 frames.
    Returns (sem float32 (..., 3), err float64 (...), finite bool (...))."""
    a = np.asarray(a, np.float32)
    q = np.asarray(q, np.float32)
    finite = np.isfinite(a).all(-1) & np.isfinite(q).all(-1)
    dn = np.float64(n)
    denom = dn * np.float64(n - 1)
    with np.errstate(all="ignore"):
        a64, q64 = a.astype(np.float64), q.astype(np.float64)
        mean = a64 / dn
        ss = q64 - a64 * mean
        ss = np.where(ss > 0, ss, 0.0)
        sem = np.sqrt(ss / denom).astype(np.float32)
        s = sem.astype(np.float64)
        v = (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1] + s[..., 2] * s[..., 2]) / 3.0
        m = (mean[..., 0] + mean[..., 1] + mean[..., 2]) / 3.0
        err = np.sqrt(v) / np.where(m > 1.0, m, 1.0)
    sem = np.where(finite[..., None], sem, np.float32(np.inf)).astype(np.float32)
    err = np.where(finite, err, np.inf)
    return sem, err, finite


def ss_unclamped(a, q, n):
    """ss_c before the clamp (float64), to find the channels rounding pushed below zero."""
    a64, q64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(q, np.float32).astype(np.float64)
    return q64 - a64 * (a64 / np.float64(n))


def scalars_ref(err, finite, threshold):
    """The image's noise scalars from the per-pixel err (float64) in numpy's own summation order."""
    e = err[finite]
    n_fin = int(e.size)
    sum_sq = float(np.sum(e * e, dtype=np.float64))
    return {"pixels": int(err.size), "below": int((e <= np.float64(np.float32(threshold))).sum()),
            "nonfinite": int(err.size - n_fin), "sum_sq": sum_sq,
            "max_err": float(np.float32(e.max())) if n_fin else 0.0,
            "rms": float(np.float32(np.sqrt(np.float64(sum_sq) / np.float64(n_fin)))) if n_fin else 0.0}
