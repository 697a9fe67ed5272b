"""Emitter sampling in float64 numpy, written from the specification and not from either implementation: what
pgo_emitter_probe (oracle) and pg_emitter_probe (device) are held to.  Bands take the form of tests/surface_model.py:
C (2^-24 ops |q| + sum_j |dq/dx_j| ulp(x_j)), plus the terms named below.

Specification (scene.sample_emitter_direction without its visibility test, and si.spawn_ray_to)
  choice        the emitter list is the flagged quads, then the flagged spheres, then the directional lights; a lane takes
                entry idx = min(floor(e1 count), count - 1) and goes on with the reused sample e1' = e1 count - idx.
  quad          light point L = origin + e1' E1 + e2 E2; ds_d the unit vector from p to L; density |L - p|^2 / (|cos| A) / count
                with cos = ds_d . normal, and no sample (density 0) unless cos < 0; em_weight = radiance count / density.
  sphere        no sample for |c - p|^2 <= (r (1 - kSphereEps))^2.  Else a direction uniform in the cone of half-angle
                alpha_max = asin(r / |c - p|) about the axis (c - p) / |c - p|: 1 - cos theta = (1 - cos alpha_max) e1', azimuth
                2 pi e2 in Duff's frame of -axis; L the near point of the sphere on that direction; density
                1 / (2 pi (1 - cos alpha_max)) / count.
  directional   (level 3) ds_d = -direction, ds_delta, density 1 / count, em_weight = irradiance count, L = p - direction
                2 max(R, |p - centre|) for the scene's bounding sphere (centre, R).
  shadow ray    sh_o = p +- n (1 + max |p_i|) kRayEps with the sign of n . (L - p); sh_d the unit vector from sh_o to L;
                sh_tmax = |L - sh_o| (1 - kShadowEps); need_shadow exactly where the density is > 0, and always for a
                directional light.  A lane without a sample holds zeros and sh_d = (0, 0, 1).

The light point is recovered from a lane's outputs as L_rec = sh_o + sh_d sh_tmax / (1 - kShadowEps).  For a quad and a
directional light it is compared with the model's L.  For a sphere it is NOT (float32 loses half the mantissa of
sin_alpha = sqrt(1 - cos_alpha^2) near the cap's centre, and 1 - cos_max cancels far away: the two points differ by up to
5e-4 r and 9e-3 r); the lane is judged by properties instead -- L_rec on the sphere, on its near side, ds_d the direction to it
and inside the cone, the density, em_weight ds_pdf = radiance, 1 - cos theta against (1 - cos alpha_max) e1' on the branch
sin^2 alpha_max > 0.00068523, and the azimuth of (L_rec - c) against 2 pi e2.

ops, the float32 roundings on a quantity's own path:
  light (quad)      4   two products, two sums; |q| := |origin| + |e1' E1| + |e2 E2|; e1' carries the rounding of e1 count
                        (one ulp of e1 count, not of e1'): an input step of its own
  light (dir.)     12   p - centre (1), its square (5), root, max, 2 ., product, difference
  recover           3   what rounding sh_d (quotient), sh_tmax (product) leave in L_rec, in units of 2^-24 sh_tmax
  ds_d, sh_d       10   difference, square (5), root, quotient; |q| := 1
  sh_o              5   max, 1 + ., . kRayEps, product, sum; |q| := |p| + the offset
  side              7   difference (1), dot (5), and 1 for ds_d's own rounding (directional); |q| := sum |n_k (L - p)_k|
  sh_tmax           9   difference, square (5), root, product
  pdf (quad)       17   as surface_model's
  pdf (cone)       20   as surface_model's, with its two cancellation terms (surface_model.cone_density)
  weight            4   radiance / pdf, . count, pdf / count, and the product the test forms
  radius           14   as surface_model's p (sphere), plus `recover`
  map              12   1 + (cos_max - 1) e1' (2), its square, 1 - ., and the same again for cos_theta; |q| := 1; plus d_ca e1'
                        (surface_model's cancellation term of cos alpha_max), (1 - cos alpha_max) ulp(e1 count), and
                        sin theta times the angular error of ds_d (`angle`) and half its square
  angle             -   of a direction to L_rec from p: (the light point's own uncertainty + ulp(p) + ulp(c) + 4 2^-24 r + the
                        tangential term) / |L - p| + 10 2^-24 (ds_d's roundings).  The tangential term: sin_alpha =
                        sqrt(1 - cos_alpha^2) carries 2 2^-24 / sin_alpha, at most sqrt(4 2^-24) = 4.9e-4 at the cap's centre: the
                        light point sits that far, times r, along the surface from where float64 puts it
  azimuth          12   2 pi e2 (1), sincos (2), the frame (6), to_world (3) in units of 2^-24 / sin(polar angle of L_rec - c); plus
                        (ulp(c) + ulp(L_rec) + `recover`) / (r sin) and 2^-24 2 pi e2 for the argument's own rounding

Decisions within float32's own reach are AMBIGUOUS; the lane must then equal the model under one assignment of them:
  choice        e1 count within one ulp of an integer k                     -> entry k - 1 with e1' = e1 count - (k - 1), or k with 0
  facing        cos at the light within its band of 0 (quad); for a sphere the cosine at the sampled point,
                cos^2 = 2 cos_max (1 - cos_max) (1 - e1') / sin_max^2 within the band of 0 (the tangent ring, e1' -> 1)
                                                                             -> no sample, or the facing one (a grazing quad:
                                                                                any density from the band's edge up)
  side          n . (L - p) within its band of 0                             -> either offset
  inside        |c - p| within its band of r (1 - kSphereEps)                -> no sample, or the cone's
  switch        sin^2 alpha_max within its band of 0.00068523                -> `map` is not judged
C per quantity (BAND_C) is four times the worst ratio measured on the CPU oracle over the suite's own input sets
(profiles/emitter/band.txt, written by tools/emitter_mutants.py --band)."""
import functools

import numpy as np

import surface_model as SM
from surface_model import AMBIGUOUS_CAP, EPS, _dot, _unit, ulp  # noqa: F401 (the cap: defined once, read as EM.AMBIGUOUS_CAP)

K_RAY = float(np.float32(1e-4))
K_SHADOW = float(np.float32(1e-3))
ONE_MINUS_SHADOW = float(np.float32(1.0) - np.float32(1e-3))   # (1.0f - kShadowEps is itself rounded)
K_SPHERE = 1500 * 2.0 ** -24
SWITCH = float(np.float32(0.00068523))
# four times the worst |difference| / bracket measured on the oracle (profiles/emitter/band.txt); 64 would mean a missing term
BAND_C = {"light": 1.66, "ds_d": 0.75, "sh_o": 0.91, "sh_d": 0.78, "tmax": 0.85, "pdf": 3.00, "weight": 2.62, "radius": 1.38,
          "cone": 0.01, "map": 2.49, "azimuth": 1.16, "near": 0.21}
C_DECISION = 4.0   # a decision is doubtful within this many brackets of its threshold
OPS = {"light_quad": 4, "light_dir": 12, "recover": 3, "unit": 10, "sh_o": 5, "side": 7, "tmax": 9, "pdf_quad": 17, "weight": 4,
       "radius": 14, "map": 12, "azimuth": 12}


class Tables(SM.Tables):
    """surface_model's tables, the directional lights, the bounding sphere and the emitter list"""

    def __init__(self, sc):
        super().__init__(sc)
        self.dir = np.asarray(getattr(sc, "dir_lights", np.zeros((0, 8))), np.float32).reshape(-1, 8).astype(np.float64)
        self.bsphere = np.asarray(sc.bounding_sphere(), np.float32).astype(np.float64) if self.dir.shape[0] else np.zeros(4)
        q, s = np.nonzero(self.quads[:, 15] != 0)[0], np.nonzero(self.spheres[:, 5] != 0)[0]
        self.emitters = np.concatenate([q, self.first_sphere + s, -1 - np.arange(self.dir.shape[0])]).astype(np.int64)
        self.count = self.emitters.shape[0]


# surface_model's bracket, with a bracket that is not a number widened to inf: a band that wide judges nothing
_bracket = functools.partial(SM.bracket, nan_is_inf=True)


def _tangential(r, sin_alpha):
    """how far float32's sin_alpha = sqrt(1 - cos_alpha^2) moves a sphere's light point along the surface: cos_alpha carries
    2 2^-24, so sin_alpha 2 2^-24 / sin_alpha, and at the cap's centre, where that has no end, sqrt(4 2^-24) = 4.9e-4"""
    return r * np.minimum(np.sqrt(4 * EPS), 2 * EPS / np.maximum(sin_alpha, 1e-300))


def choice(T, e1):
    """-> (idx, e1', step of e1', alternative idx, alternative e1', doubtful) of the uniform choice among T.count emitters"""
    x = np.asarray(e1, np.float32).astype(np.float64) * T.count
    idx = np.minimum(np.floor(x), T.count - 1).astype(np.int64)
    k = np.rint(x)
    doubt = (np.abs(x - k) <= ulp(x)) & (k >= 1) & (k <= T.count - 1) & (x != k)
    below = idx == k - 1
    alt = np.where(doubt, np.where(below, k, k - 1), idx).astype(np.int64)
    return idx, x - idx, ulp(x), alt, np.where(doubt, np.where(below, 0.0, x - (k - 1)), x - idx), doubt


class Verdict:
    pass


@np.errstate(invalid="ignore", over="ignore", divide="ignore")
def _assignment(T, p, n, e2, idx, e1r, e1h, out, C):
    """the lanes judged with emitter T.emitters[idx] and reused sample e1r (uncertain by e1h) -> Verdict: checks (name -> (n,) ok),
    ratios (band -> (n,)), amb (n,), and what consistency() needs"""
    N = p.shape[0]
    g = {k: np.asarray(out[k], np.float32).astype(np.float64) for k in ("ds_d", "ds_pdf", "em_weight", "sh_o", "sh_d", "sh_tmax")}
    sampled = np.asarray(out["need_shadow"]) != 0
    delta = np.asarray(out["ds_delta"]) != 0
    prim = T.emitters[idx]
    kq, ks, kd = (prim >= 0) & (prim < T.first_sphere), prim >= T.first_sphere, prim < 0
    v = Verdict()
    v.ok, v.ratio, v.amb, v.why = {}, {}, np.zeros(N, bool), {}
    v.prim, v.kind = prim, np.where(kd, 2, np.where(ks, 1, 0))
    inv = 1.0 / T.count
    one = np.ones(N)

    def banded(name, band, got, q, b, sel):
        ok = SM._within(got, q, b, C[band])
        v.ok[name] = ok | ~sel
        v.ratio[band] = np.maximum(v.ratio.get(band, 0.0), np.where(sel, SM._ratio(got, q, b), 0.0))

    # ---- the light point: the model's (quad, directional) or the lane's own (sphere) ----
    tmax = g["sh_tmax"]
    L_rec = g["sh_o"] + g["sh_d"] * (tmax / ONE_MINUS_SHADOW)[:, None]
    b_rec = (EPS * OPS["recover"] * tmax)[:, None] * np.ones(3)
    L, uL = L_rec.copy(), b_rec.copy()
    nl, area, rad = np.zeros((N, 3)), one.copy(), np.zeros((N, 3))
    if kq.any():
        Q = T.quads[np.where(kq, prim, 0)]
        lf = lambda o_, a_, b_, u_, w_: o_ + u_[:, None] * a_ + w_[:, None] * b_
        size = np.abs(Q[:, 0:3]) + np.abs(e1r[:, None] * Q[:, 3:6]) + np.abs(e2[:, None] * Q[:, 6:9])
        lq, lb = _bracket(lf, [Q[:, 0:3], Q[:, 3:6], Q[:, 6:9], e1r, e2], OPS["light_quad"], size, [None, None, None, e1h, None])
        L[kq], uL[kq], nl[kq], area[kq], rad[kq] = lq[kq], lb[kq], Q[kq, 9:12], Q[kq, 14], Q[kq, 19:22]
    if kd.any():
        D = T.dir[np.where(kd, -1 - prim, 0)]
        bs = np.tile(T.bsphere, (N, 1))
        lf = lambda p_, d_, s_: p_ - d_ * (2 * np.maximum(s_[:, 3], np.sqrt(_dot(p_ - s_[:, 0:3], p_ - s_[:, 0:3]))))[:, None]
        size = np.abs(p) + np.abs(lf(p, D[:, 0:3], bs) - p)
        lq, lb = _bracket(lf, [p, D[:, 0:3], bs], OPS["light_dir"], size)
        L[kd], uL[kd], rad[kd] = lq[kd], lb[kd], D[kd, 3:6]
        v.dir_d = D[:, 0:3]
    centre, radius = np.zeros((N, 3)), one.copy()
    if ks.any():
        S = T.spheres[np.where(ks, prim - T.first_sphere, 0)]
        centre[ks], radius[ks], rad[ks] = S[ks, 0:3], S[ks, 3], S[ks, 6:9]
    v.L, v.centre, v.radius, v.nl = L, centre, radius, nl
    dist = np.sqrt(_dot(L - p, L - p))

    # ---- is there a sample? ----
    expect = np.ones(N, bool)
    doubt = np.zeros(N, bool)
    graze = np.zeros(N, bool)
    cosf = lambda p_, l_, n_: _dot(_unit(l_ - p_), n_)
    if kq.any():
        cos, cos_b = _bracket(cosf, [p, L, nl], 13, one, [None, uL, None])
        expect[kq] = (cos < 0)[kq]
        graze = kq & (np.abs(cos) <= C_DECISION * cos_b) & (dist > 0)
        doubt |= graze
        v.why["graze"] = graze
    inside = np.zeros(N, bool)
    if ks.any():
        D_, D_b = _bracket(lambda p_, c_: np.sqrt(_dot(c_ - p_, c_ - p_)), [p, centre], 8)
        adj = radius * (1 - K_SPHERE)
        inside = ks & (D_ <= adj)
        cut = ks & (np.abs(D_ - adj) <= C_DECISION * (D_b + 3 * EPS * radius))
        sin, sin_b, cone_q, cone_b, cm, d_ca = SM.cone_density(p, centre, radius, inv)
        sin = np.minimum(sin, 1.0)
        # the cosine at the sampled point, squared; its noise: the roundings of 1 - tt^2 (absolute, of the size of 1) and cos_max's own
        one_m = sin ** 2 / (1 + cm)                                       # 1 - cos alpha_max without the cancellation
        cos2 = 2 * cm * one_m * np.maximum(1 - e1r, 0.0) / sin ** 2
        # ... and the angular error of the direction to a light point t away, which p's and c's last places leave
        cos_t = 1 - one_m * e1r
        t_near = D_ * cos_t - np.sqrt(np.maximum(radius ** 2 - D_ ** 2 * (1 - cos_t ** 2), 0.0))
        sin_a = np.maximum(t_near, 0.0) * np.sqrt(np.maximum(1 - cos_t ** 2, 0.0)) / radius      # (law of sines in p, c, L)
        turn = (ulp(p).max(axis=1) + ulp(centre).max(axis=1) + 4 * EPS * radius + _tangential(radius, sin_a)) / np.maximum(t_near, 1e-300) + 8 * EPS
        # (below the switch sin^2 theta = sin_max^2 e1' has relative roundings only: cos^2 = 1 - e1' to 4 2^-24 and e1''s own step)
        taylor = sin ** 2 <= SWITCH
        cos2 = np.where(taylor, np.maximum(1 - e1r, 0.0), cos2)
        noise2 = np.where(taylor, 4 * EPS + e1h, (4 * EPS + 2 * cm * d_ca + 2 * one_m * e1h) / sin ** 2)
        ring = ks & ~inside & ((cos2 <= C_DECISION * noise2) | (np.sqrt(cos2) <= C_DECISION * turn))
        v.why.update({"ring": ring, "cut": cut})
        expect[ks] = ~inside[ks]
        doubt |= cut | ring
        v.sin, v.sin_b, v.cm, v.d_ca, v.one_m, v.inside, v.cut = sin, sin_b, cm, d_ca, one_m, inside, cut
    if T.count == 0:
        expect[:] = False
    v.amb |= doubt
    v.ok["sampled"] = doubt | (sampled == expect)
    no = ~sampled
    zero3 = lambda a: (a == 0).all(axis=1)
    v.ok["no sample: zeros"] = ~no | ((g["ds_pdf"] == 0) & zero3(g["em_weight"]) & zero3(g["sh_o"]) & (tmax == 0) & ~delta &
                                      (g["sh_d"] == np.array([0.0, 0.0, 1.0])).all(axis=1))
    v.ok["need_shadow is ds_pdf > 0"] = sampled == (g["ds_pdf"] > 0)
    v.ok["delta"] = no | (delta == kd)
    # a light that faces away still has its direction (NaN where p is the light point itself); inside a sphere there is none
    dq, db = _bracket(lambda l_, p_: _unit(l_ - p_), [L, p], OPS["unit"], 1.0, [uL, None])
    away = no & kq
    v.ok["ds_d (no sample)"] = ~no | np.where(away, SM._within(g["ds_d"], dq, db, C["ds_d"]) | np.isnan(g["ds_d"]).any(axis=1) | (dist == 0),
                                             zero3(g["ds_d"]) | (ks & ~inside & doubt))
    v.sampled = sampled

    # ---- the sample ----
    y = sampled
    banded("light point", "light", L_rec, L, uL + b_rec, y & ~ks)
    banded("ds_d", "ds_d", g["ds_d"], dq, db, y)
    if kd.any():
        banded("ds_d is -direction", "ds_d", g["ds_d"], -v.dir_d, np.zeros((N, 3)), y & kd)
    # the offset's side
    sidef = lambda n_, l_, p_: _dot(n_, l_ - p_)
    sd, sd_b = _bracket(sidef, [n, L, p], OPS["side"], np.abs(n * (L - p)).sum(axis=1), [None, uL, None])
    if kd.any():   # (a directional light's side is decided by n . ds_d itself)
        sd2, sd2_b = _bracket(lambda n_, d_: -_dot(n_, d_), [n, v.dir_d], OPS["side"], np.abs(n * v.dir_d).sum(axis=1))
        sd, sd_b = np.where(kd, sd2, sd), np.where(kd, sd2_b, sd_b)
    side_doubt = y & (np.abs(sd) <= C_DECISION * sd_b)
    v.amb |= side_doubt
    v.why["side"] = side_doubt
    sof = lambda p_, n_, s_: p_ + n_ * (s_ * (1 + np.abs(p_).max(axis=1)) * K_RAY)[:, None]
    sgn = np.where(sd < 0, -1.0, 1.0)
    so_ok = np.zeros(N, bool)
    for flip in (1.0, -1.0):
        mag = np.abs(n) * ((1 + np.abs(p).max(axis=1)) * K_RAY)[:, None]
        oq, ob = _bracket(lambda p_, n_: sof(p_, n_, sgn * flip), [p, n], OPS["sh_o"], np.abs(p) + mag)
        ok = SM._within(g["sh_o"], oq, ob, C["sh_o"])
        so_ok |= ok & ((flip > 0) | side_doubt)
        if flip > 0:
            v.ratio["sh_o"] = np.where(y & ~side_doubt, SM._ratio(g["sh_o"], oq, ob), 0.0)
    v.ok["sh_o"] = ~y | so_ok
    so = g["sh_o"]
    hq, hb = _bracket(lambda l_, o_: _unit(l_ - o_), [L, so], OPS["unit"], 1.0, [uL, None])
    banded("sh_d", "sh_d", g["sh_d"], hq, hb, y)
    tq, tb = _bracket(lambda l_, o_: np.sqrt(_dot(l_ - o_, l_ - o_)) * ONE_MINUS_SHADOW, [L, so], OPS["tmax"], None, [uL, None])
    banded("sh_tmax", "tmax", tmax, tq, tb, y)
    # the density
    pq, pb = np.full(N, inv), np.full(N, EPS * inv)
    if kq.any():
        form = lambda p_, l_, n_, a_: _dot(l_ - p_, l_ - p_) / np.abs(cosf(p_, l_, n_)) / a_ * inv
        fq, fb = _bracket(form, [p, L, nl, area], OPS["pdf_quad"], None, [None, uL, None, None])
        pq, pb = np.where(kq, fq, pq), np.where(kq, fb, pb)
        edge = dist ** 2 / (np.abs(cos) + C_DECISION * cos_b) / area * inv * (1 - C["pdf"] * OPS["pdf_quad"] * EPS)
    if ks.any():
        pq, pb = np.where(ks, cone_q, pq), np.where(ks, cone_b, pb)
    got = g["ds_pdf"]
    ok = SM._within(got, pq, pb, C["pdf"])
    if kq.any():
        ok |= graze & (got >= edge)
    v.ok["ds_pdf"] = ~y | ok
    v.ratio["pdf"] = np.where(y & ~graze, SM._ratio(got, pq, pb), 0.0)
    v.pdf_q, v.pdf_b, v.graze = pq, pb, graze
    # the weight: em_weight ds_pdf = radiance (area lights); irradiance count (directional)
    area_light = y & ~kd
    banded("em_weight ds_pdf = radiance", "weight", g["em_weight"] * got[:, None], rad, EPS * OPS["weight"] * rad, area_light)
    banded("em_weight (directional)", "weight", g["em_weight"], rad * T.count, EPS * OPS["weight"] * rad * T.count, y & kd)

    # ---- a sphere's sample, by its properties ----
    z = y & ks
    if z.any():
        x = L_rec - centre
        rr = np.sqrt(_dot(x, x))
        rb = EPS * OPS["radius"] * radius + 1.75 * ulp(L_rec).max(axis=1) + ulp(centre).max(axis=1) + ulp(radius) + b_rec[:, 0]
        v.ok["on the sphere"] = ~z | (np.abs(rr - radius) <= C["radius"] * rb)
        v.ratio["radius"] = np.where(z, np.abs(rr - radius) / rb, 0.0)
        dcp = np.sqrt(_dot(centre - p, centre - p))
        axis = (centre - p) / dcp[:, None]
        to_l = _unit(L_rec - p)
        sin_p = np.sqrt(np.maximum(1 - _dot(x / rr[:, None], -axis) ** 2, 0.0))
        angle = (b_rec[:, 0] + ulp(p).max(axis=1) + ulp(centre).max(axis=1) + 4 * EPS * radius + _tangential(radius, sin_p)) / dist + EPS * OPS["unit"]
        # the near side: the normal at L_rec faces p
        facing = _dot(to_l, x / radius[:, None])
        nb = angle * dcp / radius + EPS * 8
        v.ok["near side"] = ~z | (facing <= C["near"] * nb)
        v.ratio["near"] = np.where(z, np.maximum(facing, 0.0) / nb, 0.0)
        # inside the cone
        d = g["ds_d"]
        sin_t = np.sqrt(_dot(np.cross(d, axis), np.cross(d, axis)))
        cone_band = sin_b + angle
        v.ok["inside the cone"] = ~z | (sin_t <= v.sin + C["cone"] * cone_band) & (_dot(d, axis) > 0)
        v.ratio["cone"] = np.where(z, np.maximum(sin_t - v.sin, 0.0) / cone_band, 0.0)
        # 1 - cos theta = (1 - cos alpha_max) e1' on the branch above the switch
        s2, s2_b = v.sin ** 2, 2 * v.sin * v.sin_b + EPS * v.sin ** 2
        sw = z & (np.abs(s2 - SWITCH) <= C_DECISION * s2_b)
        v.amb |= sw
        v.why["switch"] = sw
        above = z & (s2 > SWITCH) & ~sw
        got_m = 0.5 * _dot(d - axis, d - axis)           # (1 - cos theta of two unit vectors, without cancellation)
        want_m = v.one_m * e1r
        mb = EPS * OPS["map"] + v.d_ca * e1r + v.one_m * e1h + np.minimum(sin_t, 1.0) * angle + 0.5 * np.minimum(angle, 2.0) ** 2 + EPS * 2 * got_m
        v.ok["1 - cos theta"] = ~above | (np.abs(got_m - want_m) <= C["map"] * mb)
        v.ratio["map"] = np.where(above, np.abs(got_m - want_m) / mb, 0.0)
        # the azimuth of the light point about -axis, in Duff's frame of the float32 normal the lane made
        nf = -axis
        sign = np.where(np.signbit(nf[:, 2].astype(np.float32)), -1.0, 1.0)
        dl = x / rr[:, None]
        ab = (EPS * OPS["azimuth"] + (ulp(centre).max(axis=1) + ulp(L_rec).max(axis=1) + b_rec[:, 0]) / radius) / sin_p + EPS * 2 * np.pi * e2 + EPS * 4
        want_a = 2 * np.pi * e2
        best = np.full(N, np.inf)
        flips = z & (np.abs(nf[:, 2]) <= 8 * EPS)          # (the frame's sign hangs on the sign of a component at 0)
        for sg in (1.0, -1.0):
            fs, ft = SM.duff(nf, sign * sg)
            a = np.arctan2(_dot(dl, ft), _dot(dl, fs))
            diff = np.abs((a - want_a + np.pi) % (2 * np.pi) - np.pi)
            best = np.where((sg > 0) | flips, np.minimum(best, diff), best)
        judged = z & (C["azimuth"] * ab < 0.5)
        v.ok["azimuth"] = ~judged | (best <= C["azimuth"] * ab)
        v.ratio["azimuth"] = np.where(judged & ~flips, best / ab, 0.0)
        v.azimuth_judged = judged
    return v


def judge(T, p, n, e, out, C=None):
    """out: the probe's columns (oracle.pg_oracle.EMITTER_FIELDS / EMITTER_FLAGS) for the lanes (p, n, e).
    -> (failures: name -> lanes, ratios: band -> (n,), ambiguous: (n,) bool, the Verdict of the assignment each lane passed)"""
    C = C or BAND_C
    p, n, e = (np.asarray(a, np.float32).astype(np.float64) for a in (p, n, e))
    N = p.shape[0]
    if T.count == 0:
        z3 = lambda k: (np.asarray(out[k]) == 0).all(axis=1)
        ok = z3("ds_d") & z3("em_weight") & z3("sh_o") & (out["ds_pdf"] == 0) & (out["sh_tmax"] == 0) & (out["ds_delta"] == 0) & \
            (out["need_shadow"] == 0) & (np.asarray(out["sh_d"]) == np.array([0, 0, 1], np.float32)).all(axis=1)
        bad = np.nonzero(~ok)[0]
        return ({"no emitters: zeros": bad} if bad.size else {}), {}, np.zeros(N, bool), None
    idx, e1r, e1h, alt, alt_r, doubt = choice(T, e[:, 0])
    a = _assignment(T, p, n, e[:, 1], idx, e1r, e1h, out, C)
    passed = np.ones(N, bool)
    for ok in a.ok.values():
        passed &= ok
    bad = {k: np.nonzero(~ok)[0] for k, ok in a.ok.items()}
    if doubt.any():
        b = _assignment(T, p, n, e[:, 1], alt, alt_r, e1h, out, C)
        other = np.ones(N, bool)
        for ok in b.ok.values():
            other &= ok
        rescued = doubt & ~passed & other
        bad = {k: np.setdiff1d(lanes, np.nonzero(rescued)[0]) for k, lanes in bad.items()}
    amb = a.amb | doubt
    ratio = {k: np.where(doubt, 0.0, r) for k, r in a.ratio.items()}   # (but for a doubtful choice, every lane a check applies to)
    return {k: lanes for k, lanes in bad.items() if lanes.size}, ratio, amb, a


@np.errstate(invalid="ignore", over="ignore", divide="ignore")
def consistency(T, p, e, out, hit=None, C=None):
    """MIS: at the sampled light point, ds_pdf against emitter_hit_pdf for ref = p, the hit at the light point and the light's
    normal there.  hit None: the hit pdf is surface_model.emitter_pdf's (the model's); else the columns of a surface probe fed
    with the ray p -> light point (p, n, emitter_pdf), whose density is then compared within the sum of the two brackets.
    -> (lanes that fail, lanes judged, lanes between the sampler's inside cut and the hit pdf's cap limit -- where the
        reference formulas themselves disagree, cone against area form, and nothing is asserted)"""
    C = C or BAND_C
    p, e = (np.asarray(a, np.float32).astype(np.float64) for a in (p, e))
    N = p.shape[0]
    idx, e1r, e1h, alt, alt_r, doubt = choice(T, e[:, 0])
    fails, judged, between = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    first = True
    for ix, er in ((idx, e1r), (alt, alt_r)):
        v = _assignment(T, p, np.zeros((N, 3)), e[:, 1], ix, er, e1h, out, C)
        area = v.sampled & (v.kind != 2)
        m = SM.Model()
        m.is_em, m.kind, m.prim, m.radius, m.centre = np.ones(N, np.int32), v.kind, np.maximum(v.prim, 0), v.radius, v.centre
        tmax = np.asarray(out["sh_tmax"], np.float64)
        L = np.asarray(out["sh_o"], np.float64) + np.asarray(out["sh_d"], np.float64) * (tmax / ONE_MINUS_SHADOW)[:, None]
        nrm = np.where((v.kind == 1)[:, None], _unit(L - v.centre), v.nl)
        at_p, at_n = (L, nrm) if hit is None else (hit["p"], hit["n"])
        h = SM.emitter_pdf(T, m, p, at_p, at_n)
        got = np.asarray(out["ds_pdf"], np.float64)
        ref_q = h.q if hit is None else np.asarray(hit["emitter_pdf"], np.float64)
        band = C["pdf"] * v.pdf_b + SM.BAND_C["pdf"] * h.b
        ok = (np.abs(got - ref_q) <= band) | (h.amb & (np.abs(got - h.alt) <= C["pdf"] * v.pdf_b + SM.BAND_C["pdf"] * h.alt_b))
        ok |= (h.graze & ((got >= h.at_least) | (got == 0) | (hit is not None))) | v.graze   # (grazing: no upper end)
        gap = area & (v.kind == 1) & (getattr(v, "sin", np.zeros(N)) + C_DECISION * getattr(v, "sin_b", np.zeros(N)) >= SM.CAP_LIMIT)
        ok |= gap | ~area
        if first:
            fails, judged, between = ~ok, area & ~gap, gap
        else:
            fails &= ~(doubt & ok)
        first = False
    return np.nonzero(fails)[0], judged, between
