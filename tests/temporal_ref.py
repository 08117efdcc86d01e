"""Temporal reuse (include/rt2.h "Temporal reuse", raytrace2_amd/csrc/temporal.h) in numpy float32, shared by
the host test and the GPU tests. numpy rounds every float32 operation on its own (no fused multiply-add) and
its float32 division is correctly rounded, so the product must match the header bit for bit. Every array
below is float32; no Python float takes part in an operation."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(max_history=1024.0, max_history_specular=0.0, min_normal_dot=0.9, sigma_p=0.01, sigma_a=0.1)
FEATURE_FLOATS = 16


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]).astype(F32)


def _finite(x):
    return (x - x) == 0


def project(P, cam, w, h):
    """(ok, fx, fy): the history-image position of the points P (h, w, 3) under the 21 camera words."""
    cam = np.asarray(cam, F32)
    p00, du, dv, ctr = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    r = P - ctr
    e = p00 - ctr
    m = _cross(du, dv)
    dr, de = _dot(r, m), _dot(e, m)
    ok = _finite(dr) & _finite(de) & (dr != 0) & (de != 0) & ((dr > 0) == (de > 0))
    s = de / dr
    q = r * s[..., None] - e
    fx = _dot(q, du) / _dot(du, du)
    fy = _dot(q, dv) / _dot(dv, dv)
    ok &= _finite(fx) & _finite(fy)
    ok &= (fx >= F32(-1)) & (fx < F32(w)) & (fy >= F32(-1)) & (fy < F32(h))
    return ok, fx, fy


def specular_mask(mat, materials):
    """Where the material index (float image) names a metal (type 0) or a dielectric (type 2) of the table."""
    if materials is None or len(materials) == 0:
        return np.zeros(mat.shape, bool)
    t = np.asarray(materials, F32).reshape(-1, 8)
    inside = (mat >= 0) & (mat < F32(len(t)))
    idx = np.where(inside, mat, 0).astype(np.int64)
    whole = idx.astype(F32) == mat
    ty = t[idx, 0]
    return inside & whole & ((ty == 0) | (ty == 2))


def temporal_ref(color, variance, length, features, hist_color, hist_variance, hist_length, hist_features, hist_camera,
                 materials=None, trace=None, **kw):
    """The statement of temporal.h over whole images: color (h, w, 3), variance (h, w), length (h, w), features
    (h, w, 16) of the current image and of the history, the history's 21 camera words, the material table (n, 8)
    or None -> (color', variance', length'). trace: a dict that receives the per-pixel branch masks."""
    k = params(**kw)
    mh, ms = F32(k["max_history"]), F32(k["max_history_specular"])
    mnd, sp, sa = F32(k["min_normal_dot"]), F32(k["sigma_p"]), F32(k["sigma_a"])
    c, v, n = np.asarray(color, F32), np.asarray(variance, F32), np.asarray(length, F32)
    f = np.asarray(features, F32)
    hc, hv, hn = np.asarray(hist_color, F32), np.asarray(hist_variance, F32), np.asarray(hist_length, F32)
    hf = np.asarray(hist_features, F32)
    h, w = v.shape
    hit, P, N, mat, A, dist = f[..., 0], f[..., 2:5], f[..., 5:8], f[..., 9], f[..., 10:13], f[..., 13]
    one, zero = F32(1), F32(0)
    tr = trace if trace is not None else {}
    with np.errstate(all="ignore"):
        fin = _finite(c).all(-1) & _finite(v)
        proj, fx, fy = project(P, hist_camera, w, h)
        cand = fin & (hit != 0) & proj
        fx0, fy0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - fx0, fy - fy0
        x0 = np.where(cand, fx0, zero).astype(np.int64)
        y0 = np.where(cand, fy0, zero).astype(np.int64)
        hfin = _finite(hc).all(-1) & _finite(hv)
        sw, sv, sn = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
        sc = np.zeros_like(c)
        tol_p, tol_a = sp * dist, sa * sa
        for key in ("outside_l", "outside_r", "outside_b", "outside_t", "b_zero", "len_zero", "hist_nonfinite", "old_miss",
                    "mat", "normal", "plane", "albedo", "accepted"):
            tr[key] = np.zeros((h, w), bool)
        for j in (0, 1):
            for i in (0, 1):
                x, y = x0 + i, y0 + j
                inside = cand & (x >= 0) & (x < w) & (y >= 0) & (y < h)
                tr["outside_l"] |= cand & (x < 0)
                tr["outside_r"] |= cand & (x >= w)
                tr["outside_b"] |= cand & (y < 0)
                tr["outside_t"] |= cand & (y >= h)
                xs, ys = np.where(inside, x, 0), np.where(inside, y, 0)
                b = (tx if i else one - tx) * (ty if j else one - ty)
                ok = inside & (b > 0)
                tr["b_zero"] |= inside & ~(b > 0)
                qn, qf = hn[ys, xs], hf[ys, xs]
                t_len = qn > 0
                t_fin = hfin[ys, xs]
                t_hit = qf[..., 0] != 0
                t_mat = qf[..., 9] == mat
                t_nrm = _dot(N, qf[..., 5:8]) >= mnd
                t_pln = np.abs(_dot(N, qf[..., 2:5] - P)) <= tol_p
                dA = qf[..., 10:13] - A
                t_alb = _dot(dA, dA) <= tol_a
                for key, t in (("len_zero", t_len), ("hist_nonfinite", t_fin), ("old_miss", t_hit), ("mat", t_mat),
                               ("normal", t_nrm), ("plane", t_pln), ("albedo", t_alb)):
                    tr[key] |= ok & ~t
                    ok = ok & t
                tr["accepted"] |= ok
                sw = np.where(ok, sw + b, sw)
                sc = np.where(ok[..., None], sc + b[..., None] * hc[ys, xs], sc)
                sv = np.where(ok, sv + b * hv[ys, xs], sv)
                sn = np.where(ok, sn + b * qn, sn)
        spec = specular_mask(mat, materials)
        cap = np.where(spec, ms, mh)
        mean_n = sn / sw
        Nn = np.where(mean_n < cap, mean_n, cap)
        has = cand & (sw > 0) & (Nn > 0)
        a = n / (Nn + n)
        mc = sc / sw[..., None]
        mv = sv / sw
        bc = mc + a[..., None] * (c - mc)
        ia = one - a
        bv = (ia * ia) * mv + (a * a) * v
        oc = np.where(has[..., None], bc, c).astype(F32)
        ov = np.where(has, bv, v).astype(F32)
        on = np.where(has, Nn + n, np.where(fin, n, zero)).astype(F32)
    tr.update(finite=fin, hit=hit != 0, projected=proj, candidate=cand, specular=spec, has=has,
              capped=has & ~(mean_n < cap), uncapped=has & (mean_n < cap), tx_zero=cand & (tx == 0),
              cap_zero=cand & (sw > 0) & (cap == 0))
    return oc, ov, on


def synthetic_case(w, h, seed=11):
    """A dict with the current image (color, variance, length, features), the history (hist_*), the history camera
    and a material table, built so that every branch of the statement is reached at 70 x 37 (and whatever fits at
    smaller sizes): the current image is a plane z = 4 seen from a camera A, the history the same plane seen from
    a camera B shifted sideways by a whole number of pixels plus a fraction, so that the taps run off the left and
    the bottom edge; single pixels are then edited for the other branches. Positions are taken modulo the image."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((5, 8), F32)
    mats[:, 0] = [1, 0, 2, 4, 1]  # lambertian, metal, dielectric, diffuse_light, lambertian
    mats[:, 1:4] = [[0.73, 0.73, 0.73], [0.8, 0.6, 0.2], [1, 1, 1], [0, 0, 0], [0.65, 0.05, 0.05]]
    mats[2, 5] = 1.5
    plane_z = 4.0
    # the history camera B: every word a short binary fraction, so the projection of the plane's points is exact
    # and the fractions chosen below (and tx == 0) arrive as they are
    camB = np.zeros(21, F32)
    ctr = np.array([0.25, 0.25, 0.0])
    du, dv = np.array([1 / 32, 0, 0]), np.array([0, 1 / 32, 0])
    p00 = ctr + np.array([-(w // 2) / 32, -(h // 2) / 32, 1.0])
    camB[0:3], camB[3:6], camB[6:9], camB[9:12], camB[19], camB[20] = p00, du, dv, ctr, 1, 1

    def plane_points(ox, oy):
        """The plane points under history-pixel coordinates (x + ox, y + oy)."""
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        d = p00 + (x + ox)[..., None] * du + (y + oy)[..., None] * dv - ctr
        return ctr + d * plane_z

    def record(P, mat_idx):
        f = np.zeros((h, w, FEATURE_FLOATS), F32)
        f[..., 0] = 1
        f[..., 2:5] = P
        f[..., 5:8] = [0, 0, -1]
        f[..., 8] = 1
        f[..., 9] = mat_idx
        f[..., 10:13] = mats[mat_idx, 1:4]
        f[..., 13] = np.sqrt((P * P).sum(-1))
        f[..., 1] = f[..., 13]
        return f

    yy, xx = np.mgrid[0:h, 0:w]
    mat_idx = np.where(xx >= (2 * w) // 3, 4, 0)
    hf = record(plane_points(0.0, 0.0), mat_idx)
    # the current pixels look at the plane points 2.375 history pixels to the left and 1.5 below their own
    f = record(plane_points(-2.375, -1.5), np.where(xx - 2 >= (2 * w) // 3, 4, 0))
    # the right columns reproject past the right edge, the top rows past the top edge
    f[:, (w - 1) % w, 2:5] = plane_points(0.5, 0.25)[:, (w - 1) % w]
    f[(h - 1) % h, :, 2:5] = plane_points(0.25, 0.5)[(h - 1) % h]
    c = (rng.random((h, w, 3), F32) * F32(0.5) + F32(0.25)).astype(F32)
    v = (rng.random((h, w), F32) * F32(0.01) + F32(0.001)).astype(F32)
    n = np.full((h, w), 4, F32)
    hc = (rng.random((h, w, 3), F32) * F32(0.5) + F32(0.25)).astype(F32)
    hv = (rng.random((h, w), F32) * F32(0.001) + F32(0.0001)).astype(F32)
    hn = np.full((h, w), 64, F32)
    hn[:, (w // 2) % w:] = 2000  # past the default cap

    def at(yf, xf):
        return int(yf * h) % h, int(xf * w) % w

    def old_of(p):
        """A history pixel that the current pixel p taps with positive weight (clamped into the image)."""
        return min(max(p[0] - 1, 0), h - 1), min(max(p[1] - 2, 0), w - 1)

    # current-pixel edits
    p = at(0.3, 0.3)
    f[p] = 0
    f[p][10:13] = [0.5, 0.7, 1.0]  # a miss
    c[at(0.3, 0.4)][1] = np.nan  # not finite
    v[at(0.3, 0.45)] = np.inf
    p = at(0.4, 0.3)
    f[p][4] = -3.0  # behind the old camera
    p = at(0.4, 0.4)
    f[p][4] = 0.0  # dr == 0: in the old camera's plane
    p = at(0.4, 0.5)
    f[p][2:5] = plane_points(-3.0, -1.5)[p]  # tx == 0
    p = at(0.5, 0.3)
    f[p][13] = 0  # dist == 0
    for q, (m_i, yf, xf) in enumerate([(1, 0.6, 0.3), (2, 0.6, 0.45), (1, 0.6, 0.8), (2, 0.6, 0.9)]):
        p = at(yf, xf)  # metal and dielectric current hits whose history agrees
        o = old_of(p)
        for rec in (f, hf):
            for yy_, xx_ in ((p,) if rec is f else ((o[0] + a, o[1] + b) for a in (0, 1, 2) for b in (0, 1, 2))):
                if 0 <= yy_ < h and 0 <= xx_ < w:
                    rec[yy_, xx_, 9] = m_i
                    rec[yy_, xx_, 10:13] = mats[m_i, 1:4]
    # history edits, each under a current pixel that would otherwise accept it
    def olds(yf, xf):
        o = old_of(at(yf, xf))
        return [(min(o[0] + a, h - 1), min(o[1] + b, w - 1)) for a in (0, 1) for b in (0, 1)]

    for o in olds(0.7, 0.2):
        hn[o] = 0  # no history
    for o in olds(0.7, 0.3):
        hc[o][2] = np.inf
    for o in olds(0.7, 0.35):
        hv[o] = np.nan
    for o in olds(0.7, 0.45):
        hf[o] = 0  # an old miss
    for o in olds(0.7, 0.55):
        hf[o][9] = 3  # another material
    for o in olds(0.8, 0.2):
        hf[o][5:8] = [0.6, 0, -0.8]  # normal
    for o in olds(0.8, 0.3):
        hf[o][4] = plane_z + 1.0  # off the plane
    for o in olds(0.8, 0.45):
        hf[o][10:13] = [0.2, 0.9, 0.2]  # albedo
    return dict(color=c, variance=v, length=n, features=f, hist_color=hc, hist_variance=hv, hist_length=hn,
                hist_features=hf, hist_camera=camB, materials=mats)


def case_args(case):
    """The positional arguments of temporal_ref / temporal_buffers from a synthetic_case dict (without materials)."""
    return [case[k] for k in ("color", "variance", "length", "features", "hist_color", "hist_variance", "hist_length",
                              "hist_features", "hist_camera")]
