"""The feature buffers' rays and the variance-guided a-trous filter (include/rt2.h "Feature buffers and
denoiser", raytrace2_amd/csrc/denoise.h) in numpy float32, shared by the host test and the GPU tests. numpy
rounds every float32 operation on its own (no fused multiply-add) and its float32 division and sqrt are
correctly rounded, so the product must match bit for bit. Every array below is float32; no Python float
takes part in an operation."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(iterations=5, normal_power_log2=7, sigma_l=1.0, sigma_p=0.01, sigma_a=0.1, eps_l=1e-3)
K1 = (F32(0.375), F32(0.25), F32(0.0625))
FEATURE_FLOATS = 16


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def feature_rays(cp, w, h, rows=None):
    """Origin (3,) and directions (len(rows), w, 3) of the rays through the pixel centres: cp = the 21 words
    of camera_params; pc = (pixel00 + x * du) + y * dv, d = (pc - center) * (1 / sqrt(dot)) (glm::normalize)."""
    cp = np.asarray(cp, F32)
    p00, du, dv, c = cp[0:3], cp[3:6], cp[6:9], cp[9:12]
    ys = np.arange(h) if rows is None else np.asarray(rows)
    x = np.arange(w).astype(F32)[None, :, None]
    y = ys.astype(F32)[:, None, None]
    pc = (p00 + x * du) + y * dv
    v = pc - c
    d = v * (F32(1) / np.sqrt(_dot(v, v)))[..., None]
    return c.copy(), d.astype(F32)


def features_ref(oracle_scene, cp, w, h, seed, rows=None):
    """The 16-float records from oracle.hit on the rays above. Albedo: the material table's for metal and
    lambertian, (1, 1, 1) for a dielectric; the materials that read a texture (texture, diffuse_light,
    isotropic) take a solid texture's colour from the texture table, and where the texture is a checker or
    noise the albedo slots are NaN and the pixel is flagged: the caller checks those its own way.
    Returns (records, flagged mask)."""
    o, d = feature_rays(cp, w, h, rows)
    n = d.shape[0]
    out = np.zeros((n, w, FEATURE_FLOATS), F32)
    textured = np.zeros((n, w), bool)
    materials, textures = oracle_scene.materials(), oracle_scene.textures()
    bg = np.array(list(oracle_scene.info().background), F32)
    for r in range(n):
        for x in range(w):
            rec = oracle_scene.hit(o, d[r, x], seed=seed)
            if rec[0] == 0:
                out[r, x, 10:13] = bg
                continue
            out[r, x, 0:10] = rec
            m = materials[int(rec[9])]
            if int(m[0]) == 2:
                out[r, x, 10:13] = 1
            elif int(m[0]) in (3, 4, 5):
                t = textures[int(m[6])]
                if int(t[0]) == 0:
                    out[r, x, 10:13] = t[1:4]
                else:
                    out[r, x, 10:13] = np.nan
                    textured[r, x] = True
            else:
                out[r, x, 10:13] = m[1:4]
            dp = out[r, x, 2:5] - o
            out[r, x, 13] = np.sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2])
    return out, textured


def variance_of_sem(sem):
    """v = ((sem_r^2 + sem_g^2) + sem_b^2) / 3 in float32 (the tracer path's variance of the mean)."""
    s = np.asarray(sem, F32)
    with np.errstate(all="ignore"):
        return (((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2]) / F32(3)).astype(F32)


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that is inside, else fill; and the inside mask."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def _lum(c):
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / F32(3)


def denoise_ref(color, variance, features, **kw):
    """color (h, w, 3), variance (h, w), features (h, w, 16) float32 -> (color', variance')."""
    k = params(**kw)
    sl, sp, sa, el = F32(k["sigma_l"]), F32(k["sigma_p"]), F32(k["sigma_a"]), F32(k["eps_l"])
    c = np.array(color, F32)
    v = np.array(variance, F32)
    f = np.asarray(features, F32)
    hit, P, N, A, dist = f[..., 0], f[..., 2:5], f[..., 5:8], f[..., 10:13], f[..., 13]
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        for it in range(int(k["iterations"])):
            s = 1 << it
            fin = np.isfinite(c).all(-1) & np.isfinite(v)
            sv, sw = np.zeros_like(v), np.zeros_like(v)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    vq, inside = _shift(v, dx, dy)
                    fq, _ = _shift(fin, dx, dy, False)
                    hq, _ = _shift(hit, dx, dy)
                    ok = inside & fq & (hq == hit)
                    w = F32((0.25, 0.125, 0.0625)[(dx != 0) + (dy != 0)])
                    sv = np.where(ok, sv + w * vq, sv)
                    sw = np.where(ok, sw + w, sw)
            vbar = sv / sw
            lp = _lum(c)
            den_l = sl * np.sqrt(np.where(vbar > 0, vbar, zero)) + el
            den_p = sp * dist
            sc, tv, tw = np.zeros_like(c), np.zeros_like(v), np.zeros_like(v)
            anyw = np.zeros(v.shape, bool)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    h = K1[abs(dx)] * K1[abs(dy)]
                    if dx == 0 and dy == 0:
                        wgt = np.full_like(v, h)
                        ok = np.ones(v.shape, bool)
                        cq, vq = c, v
                    else:
                        cq, inside = _shift(c, s * dx, s * dy)
                        vq, _ = _shift(v, s * dx, s * dy)
                        fq, _ = _shift(fin, s * dx, s * dy, False)
                        hq, _ = _shift(hit, s * dx, s * dy)
                        Pq, _ = _shift(P, s * dx, s * dy)
                        Nq, _ = _shift(N, s * dx, s * dy)
                        Aq, _ = _shift(A, s * dx, s * dy)
                        ok = inside & fq & (hq == hit)
                        dl = lp - _lum(cq)
                        xl = np.abs(dl) / den_l
                        wl = one / (one + xl * xl)
                        wl = np.where(dl == dl, wl, zero)
                        wgt = h * wl
                        wn = _dot(N, Nq)
                        wn = np.where(wn > 0, wn, zero)
                        for _ in range(int(k["normal_power_log2"])):
                            wn = wn * wn
                        pd = _dot(N, Pq - P)
                        xp = np.abs(pd) / den_p
                        wp = np.where(den_p > 0, one / (one + xp * xp), one)
                        dA = Aq - A
                        wa = one / (one + _dot(dA, dA) / (sa * sa))
                        wgt = np.where(hit != 0, ((wgt * wn) * wp) * wa, wgt)
                        anyw |= ok & (wgt > 0)
                    tw = np.where(ok, tw + wgt, tw)
                    sc = np.where(ok[..., None], sc + wgt[..., None] * cq, sc)
                    tv = np.where(ok, tv + (wgt * wgt) * vq, tv)
            nc = sc / tw[..., None]
            nv = tv / (tw * tw)
            keep = ~fin | ~anyw
            c = np.where(keep[..., None], c, nc).astype(F32)
            v = np.where(keep, v, nv).astype(F32)
    return c, v


def synthetic_case(w, h, seed=11):
    """A (color, variance, features) case with what the filter's branches need: a hit / miss boundary (the
    left columns miss), a normal discontinuity and smoothly turning normals, two albedos, a zero-variance
    flat region next to a bright noisy one, one NaN colour, one +inf variance, one negative variance, and a
    hit with dist == 0. Positions are taken modulo the image, so every size gets what fits."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, FEATURE_FLOATS), F32)
    hit = x >= (2 * w) // 5 if w > 1 else np.ones((h, w), bool)
    f[..., 0] = hit
    f[..., 1] = 5 + 0.25 * x
    f[..., 2], f[..., 3], f[..., 4] = 0.1 * x - 2, 0.1 * y - 1, 5 + 0.01 * x + 0.02 * y
    right = x >= (3 * w) // 4
    n = np.stack([np.where(right, 1.0, 0.1 * np.sin(0.3 * x)), np.full((h, w), 0.05), np.where(right, 0.0, 1.0)], -1)
    f[..., 5:8] = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(F32)
    f[..., 8] = 1
    f[..., 9] = np.where(y >= h // 2, 1, 2)
    f[..., 10:13] = np.where((y >= h // 2)[..., None], F32([0.73, 0.73, 0.73]), F32([0.65, 0.05, 0.05]))
    p = f[..., 2:5]
    f[..., 13] = np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
    f[(h // 3) % h, (w - 2) % w, 13] = 0  # a hit at the camera's centre
    f[~hit] = 0
    f[~hit, 10:13] = F32([0.5, 0.7, 1.0])  # the background
    c = (rng.random((h, w, 3), F32) * F32(0.5) + F32(0.25)).astype(F32)
    v = (rng.random((h, w), F32) * F32(0.01)).astype(F32)
    bright = (x >= w // 2) & (y < h // 2)
    c[bright] = (c[bright] * F32(20)).astype(F32)
    v[bright] = F32(1.5)
    flat = (x >= w // 2) & (y >= h // 2) & (x < w // 2 + max(3, w // 5))
    c[flat] = F32([0.3, 0.3, 0.3])
    v[flat] = 0
    c[(h // 2) % h, (w // 2 + 1) % w, 1] = np.nan
    v[(h - 1) % h, (w - 1) % w] = np.inf
    v[0, (w // 2) % w] = F32(-0.25)
    return c, v, f
