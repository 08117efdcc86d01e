"""Adaptive sampling's semantics (include/rt2.h "Adaptive sampling", raytrace2_amd/csrc/adaptive.h) in numpy,
on noise_ref: a simulator over per-frame samples, shared by the host test and the GPU tests. A pixel that
stops after n frames holds the frame-order float32 sums of its first n samples, so the whole adaptive
result (which pixel stopped when, every bit of its sums) follows from the per-frame samples."""
import numpy as np

from noise_ref import noise_ref

WINDOW_MAX = 64


def pixel_noise(a, q, n):
    """noise_ref with a sample count per pixel: a, q float32 (..., 3), n integer (...).
    Returns (sem float32 (..., 3), err float64 (...), finite bool (...))."""
    a, q, n = np.asarray(a, np.float32), np.asarray(q, np.float32), np.asarray(n)
    sem = np.zeros(a.shape, np.float32)
    err = np.zeros(n.shape, np.float64)
    finite = np.zeros(n.shape, bool)
    for v in np.unique(n):
        m = n == v
        sem[m], err[m], finite[m] = noise_ref(a[m], q[m], int(v))
    return sem, err, finite


def over_flags(a, q, n, threshold):
    """over = !(finite && err <= (double)threshold) per pixel, and finite."""
    _, err, finite = pixel_noise(a, q, n)
    with np.errstate(invalid="ignore"):
        below = err <= np.float64(np.float32(threshold))
    return ~(finite & below), finite


def window_or(over, window):
    """Per pixel: is some pixel of the same row in the columns [x - window, x + window] within the row over?
    over: bool (rows, width)."""
    assert 0 <= window <= WINDOW_MAX
    out = over.copy()
    for d in range(1, min(window, over.shape[1] - 1) + 1):
        out[:, d:] |= over[:, :-d]
        out[:, :-d] |= over[:, d:]
    return out


class AdaptiveSim:
    """The tracer's adaptive state over samples (frames, rows, width, 3) float32, frame f = samples[f]."""

    def __init__(self, samples):
        self.s = samples
        self.reset()

    def reset(self):
        shape = self.s.shape[1:3]
        self.a = np.zeros(shape + (3,), np.float32)
        self.q = np.zeros(shape + (3,), np.float32)
        self.n = np.zeros(shape, np.uint32)
        self.active = np.ones(shape, bool)
        self.frame = 0
        self.history = []  # one dict per check

    def render(self, n_frames):
        assert self.frame + n_frames <= len(self.s)
        m = self.active
        for f in range(self.frame, self.frame + n_frames):
            s = self.s[f]
            self.a[m] = self.a[m] + s[m]
            self.q[m] = self.q[m] + s[m] * s[m]
        self.n[m] += np.uint32(n_frames)
        self.frame += n_frames

    def check(self, threshold, window):
        assert self.frame >= 2
        over, finite = over_flags(self.a, self.q, self.n, threshold)
        stays = self.active & window_or(over, window)
        out = {"frames": self.frame, "pixels": int(self.n.size), "active": int(stays.sum()),
               "retired": int((self.active & ~stays).sum()), "samples": int(self.n.astype(np.uint64).sum()),
               "nonfinite": int((~finite).sum())}
        self.history.append({**out, "active_before": int(self.active.sum()),
                             "margin": margin(self.a, self.q, self.n, threshold)})
        self.active = stays
        return out

    def render_adaptive(self, threshold, max_frames, window=1, min_frames=0, check_every=16):
        """rt2_tracer_render_adaptive with check_every > 0 (0 is one stratum sweep: pass sqrt_spp^2)."""
        out = {k: 0 for k in ("frames", "pixels", "active", "retired", "samples", "nonfinite")}
        while self.frame < max_frames:
            self.render(min(check_every, max_frames - self.frame))
            if self.frame < max(min_frames, 2):
                continue
            out = self.check(threshold, window)
            if out["active"] == 0:
                break
        return out


def margin(a, q, n, threshold):
    """The smallest |err / threshold - 1| over the pixels with err > 0: how far the nearest pixel is from
    changing sides by a last-bit difference."""
    _, err, finite = pixel_noise(a, q, n)
    with np.errstate(invalid="ignore"):
        e = err[finite & (err > 0)]
    if not e.size or not np.float32(threshold) > 0:
        return np.inf
    return float(np.abs(e / np.float64(np.float32(threshold)) - 1.0).min())
