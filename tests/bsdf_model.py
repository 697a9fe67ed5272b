"""A plain float64 model of the renderer's BSDF layer, written from the published formulas -- not from the device's
csrc/pg_render_dev.hpp nor from the oracle's restatement of it, whose bit parity cannot show an error both share.

What is modelled (local frame, z the normal; `value` includes cos(theta_o), as Mitsuba's eval does):

  diffuse            value = refl / pi * cos(theta_o), pdf = cos(theta_o) / pi, both directions above the surface
  conductor Fresnel  complex arithmetic: n = eta + i k, sin(theta_t) = sin(theta_i) / n, r_s and r_p from the Fresnel equations,
                     F = (|r_s|^2 + |r_p|^2) / 2; the smooth conductor is a delta lobe of weight F * specular reflectance
  dielectric Fresnel Snell's law, r_s and r_p, total internal reflection where sin(theta_t) >= 1; the smooth dielectric is a
                     delta reflection (probability F) or refraction (1 - F, weight 1 / eta^2: radiance transport)
  microfacets        D: Beckmann exp(-tan^2 / a^2) / (pi a^2 cos^4), GGX a^2 / (pi cos^4 (a^2 + tan^2)^2);
                     G1: GGX exact, 2 / (1 + sqrt(1 + a^2 tan^2)); Beckmann by Mitsuba's rational fit in 1 / (a tan) below 1.6
                     -- the fit is the specification; the exact erf form is g1_beckmann_exact and tests bound the fit by it
  rough conductor    Walter et al. 2007, eq. 20: F D G / (4 |cos_i|) (times cos_o / cos_o), G = G1(wi) G1(wo); the pdf of
                     sampling VISIBLE normals (Heitz & d'Eon 2014): D G1(wi) |wi.m| / |cos_i| times the Jacobian 1 / (4 |wo.m|)
  rough dielectric   eq. 21 with the generalised half vector m = +-normalize(wi + eta wo) of either side, the Jacobian
                     eta^2 |wo.m| / (wi.m + eta wo.m)^2 (eq. 17), the radiance scale 1 / eta^2, the lobe probabilities F, 1 - F
                     (an index ratio of exactly 1 -- no interface, a delta the lobes cannot express -- gives zeros)
  wrapping           a two-sided row mirrors wi and wo when wi is below; a one-sided row hit from behind gives zeros;
                     feature levels as include/pgsd.h states them for pg_bsdf_probe

The float32 inputs are taken as given (nothing is renormalised; the kernels do not either).  There is NO sampler here: a
sampled direction is judged by the model's pdf and value AT that direction (judge_sample) and by the density test of
tests/test_bsdf_model.py, which keeps the model independent of how an implementation inverts the distribution.

Conditioning.  Beside every quantity q the model returns band(q) = C * (2^-24 * ops * |q| + sum_j |dq_j|): dq_j is the change
of q (float64 differences, both signs, the larger) when float32 input j moves by one unit in its last place -- q's sensitivity
to that input, 2^-24 * |q| times its relative sensitivity -- and `ops` counts the float32 roundings on q's
path (OPS below).  The sensitivities stand for the roundings of intermediate results: a rounded half vector is the half vector
of a slightly different wo.  C is measured (profiles/bsdf/band.txt) and fixed in BAND_C.

Branches.  The implementation decides by float32 comparisons; where the float64 value b of the compared quantity is within
its own reach (the same expression for b, with C = 64, far beyond any band's) either decision is legitimate and the
case is AMBIGUOUS: `candidates` then returns the model's answer under every combination of the doubtful decisions and an
output must lie in the band of one of them -- nothing else is accepted.  Decisions:
  side_i, side_o   sign of wi.m, wo.m against the side wi, wo are on (G1's visibility test, the pdf's side test)
  a16_i, a16_o     the Beckmann fit's switch at 1 / (a tan) >= 1.6
  dcut             D * cos(theta_m) > 1e-20 (microfacet.h's cut)
  front            the sign of wi.m where Fresnel's side (eta or 1 / eta) is taken from it
  mflip            which of +-m points up (m.z of the generalised half vector)
  tir              total internal reflection (cos^2(theta_t) <= 0)
  reflect          cos_i * cos_o > 0: reflection or transmission (inputs as given: doubtful only where the product underflows)
  lobe             u1 <= F (sampling only)
and, for reporting only (it changes which direction is sampled, never the density), sincos_phi's switch (phi_switch)."""
import itertools

import numpy as np

U = 2.0 ** -24
DIFFUSE, ROUGH_CONDUCTOR, CONDUCTOR, DIELECTRIC, ROUGH_DIELECTRIC = range(5)
STRIDE = 16
# columns of the input matrix X (float64 copies of the float32 inputs): what the sensitivities move
WI, WO, ALPHA, ETA, K, REFL, U1 = slice(0, 3), slice(3, 6), 6, slice(7, 10), slice(10, 13), slice(13, 16), 16
NX = 17

# float32 roundings on the path of a quantity, by the kind of row (counted on the formulas above as the kernels must
# evaluate them; transcendental error is not itemised, BAND_C covers it):
#   half vector: 3 adds (+3 products with eta), 3 squares, 2 adds, sqrt, 3 divisions                      12 (15)
#   D: 2 divisions by a, 3 squares, 2 adds, a division, exp, 4 products below                             13
#   G1: 2 products, 2 squares, add, square, division, sqrt, reciprocal; fit 9 / GGX 4; dot 5               18
#   conductor Fresnel: 24 per channel; dielectric Fresnel: 22; dot products wi.m, wo.m: 5 each
OPS = {
    "diffuse": 3,                              # refl / pi * cos: two products (the pdf: one)
    "rc_value": 12 + 13 + 2 * 18 + 5 + 24 + 6,  # ... and (D (G G)) / (4 cos), F * (refl * res)
    "rc_pdf": 12 + 13 + 18 + 4,
    "rd_value": 15 + 13 + 2 * 18 + 10 + 22 + 14,
    "rd_pdf": 15 + 13 + 18 + 10 + 22 + 14,
    "fresnel_c": 24 + 1,
    "fresnel_d": 22,
    "refract": 22 + 4,
}
BRANCH_OPS = 16   # roundings behind a compared quantity (a dot product of a normalised half vector, the fit's argument ...)
BRANCH_C = 64.0   # the reach of a decision: the C at which a band's bracket is taken to be missing a term (no BAND_C comes near)
# measured on the oracle (profiles/bsdf/band.txt: worst ratio of |difference| to the bracket, times four)
# value 1.249, pdf 1.252; a sampled direction's pdf 1.088 and weight * pdf 0.527; a delta lobe's pdf 1.426, direction 0.393
BAND_C = {"value": 5.0, "pdf": 5.1, "sample": 4.4, "delta": 5.8}
TINY = 1e-37      # float32 has no normal numbers below 1.2e-38: differences down there are the format's
AMBIGUOUS_CAP = 0.02


def _dot(a, b):
    return (a * b).sum(-1)


def _absdot(a, b):
    return (np.abs(a) * np.abs(b)).sum(-1)


class _Dec:
    """the decisions of one evaluation: forced where `forced` has them, natural otherwise; remembers b and its scale"""

    def __init__(self, forced):
        self.forced = forced or {}
        self.b, self.scale, self.taken = {}, {}, {}

    def __call__(self, name, b, scale, natural=None):
        natural = (b > 0.0) if natural is None else natural
        d = self.forced.get(name)
        d = natural if d is None else d
        # (a decision made twice -- Fresnel's on both lobes -- keeps the first record)
        if name not in self.b:
            self.b[name], self.scale[name], self.taken[name] = b, scale, d
        return d


# ---- the formulas -----------------------------------------------------------------------------------------------------------
def fresnel_conductor(cos_i, eta, k):
    """unpolarised reflectance of a conductor of index eta + i k (relative to the outside), complex arithmetic"""
    c = np.abs(cos_i).astype(np.complex128)
    n = eta + 1j * k
    sin2_i = 1.0 - c * c
    cos_t = np.sqrt(1.0 - sin2_i / (n * n))
    r_s = (c - n * cos_t) / (c + n * cos_t)
    r_p = (n * c - cos_t) / (n * c + cos_t)
    return 0.5 * (np.abs(r_s) ** 2 + np.abs(r_p) ** 2)


def fresnel_dielectric(cos_i, eta, dec=None, outside=None):
    """-> F, signed cos(theta_t) (opposite side), eta_it (index ratio along the ray: eta entering from outside, 1 / eta from
    inside).  Snell's law: sin_t = sin_i / eta_it."""
    dec = dec or _Dec(None)
    outside = (cos_i >= 0.0) if outside is None else outside   # (given where the caller has decided the side already)
    eta_it = np.where(outside, eta, 1.0 / eta)
    ci = np.abs(cos_i)
    cos2_t = 1.0 - (1.0 - ci * ci) / (eta_it * eta_it)
    transmits = dec("tir", cos2_t, 1.0 + (1.0 - ci * ci) / (eta_it * eta_it))
    ct = np.sqrt(np.abs(cos2_t))
    r_s = (ci - eta_it * ct) / (ci + eta_it * ct)
    r_p = (eta_it * ci - ct) / (eta_it * ci + ct)
    F = 0.5 * (r_s * r_s + r_p * r_p)
    F = np.where(transmits, F, 1.0)
    ct = np.where(transmits, ct, 0.0)
    F = np.where(ci == 0.0, 1.0, F)
    F = np.where(eta == 1.0, 0.0, F)
    return F, np.where(outside, -ct, ct), eta_it


def microfacet_D(m, alpha, dec):
    """alpha > 0: Beckmann, < 0: GGX of roughness -alpha (the row's convention); m need not be normalised exactly"""
    a = np.abs(alpha)
    c2 = m[..., 2] ** 2
    tan2 = (m[..., 0] ** 2 + m[..., 1] ** 2) / c2
    beck = np.exp(-tan2 / (a * a)) / (np.pi * a * a * c2 * c2)
    ggx = a * a / (np.pi * c2 * c2 * (a * a + tan2) ** 2)
    D = np.where(alpha < 0.0, ggx, beck)
    D = np.where(np.isfinite(D), D, 0.0)
    keep = dec("dcut", D * m[..., 2] - 1e-20, D * np.abs(m[..., 2]))
    return np.where(keep, D, 0.0)


def g1_beckmann_fit(a):
    """Mitsuba's rational approximation of the Beckmann G1 in a = 1 / (alpha tan(theta)), below a = 1.6"""
    return (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a)


def g1_beckmann_exact(a):
    from math import erf
    a = np.asarray(a, np.float64)
    e = np.vectorize(erf)(a)
    return 2.0 / (1.0 + e + np.exp(-a * a) / (a * np.sqrt(np.pi)))


def smith_G1(v, alpha, visible, dec, which):
    """G1 of direction v: 0 where the microfacet's front is not seen from v's side (`visible`)"""
    a_ = np.abs(alpha)
    tan2 = (v[..., 0] ** 2 + v[..., 1] ** 2) / v[..., 2] ** 2
    perpendicular = (v[..., 0] == 0.0) & (v[..., 1] == 0.0)
    with np.errstate(all="ignore"):
        a = 1.0 / (a_ * np.sqrt(tan2))
        beckmann = (alpha > 0.0) & ~perpendicular & np.isfinite(a)
        large = dec("a16_" + which, np.where(beckmann, a - 1.6, 1.0), np.where(beckmann, a, 1.0), np.where(beckmann, a >= 1.6, True))
        g_b = np.where(large, 1.0, g1_beckmann_fit(a))
        g_g = 2.0 / (1.0 + np.sqrt(1.0 + a_ * a_ * tan2))
    g = np.where(alpha < 0.0, g_g, g_b)
    g = np.where(perpendicular, 1.0, g)
    return np.where(visible, g, 0.0)


def _rough(X, kind, dec):
    """rough conductor (kind 1) and rough dielectric (kind 4), wi on either side: value (n,3), pdf"""
    wi, wo, alpha = X[:, WI], X[:, WO], X[:, ALPHA]
    ci, co = wi[:, 2], wo[:, 2]
    reflect = dec("reflect", ci * co, 0.0)    # (no rounding to speak of: doubtful only where the product underflows)
    eta_m = X[:, 7]
    eta = np.where(kind == ROUGH_DIELECTRIC, np.where(ci > 0.0, eta_m, 1.0 / eta_m), 1.0)
    scale_o = np.where(reflect, 1.0, eta)
    h = wi + wo * scale_o[:, None]
    norm = np.sqrt(_dot(h, h))
    m = h / norm[:, None]
    up = dec("mflip", m[:, 2], (np.abs(ci) + scale_o * np.abs(co)) / norm)
    m = np.where(up[:, None], m, -m)
    wim, wom = _dot(wi, m), _dot(wo, m)
    side_i = dec("side_i", wim * np.sign(ci), _absdot(wi, m))
    # (wo exactly on the horizon is on neither side, whatever wo.m is: an exact comparison)
    side_o = dec("side_o", np.where(co == 0.0, -np.inf, wom * np.sign(co)), _absdot(wo, m))
    D = microfacet_D(m, alpha, dec)
    g_i = smith_G1(wi, alpha, side_i, dec, "i")
    g_o = smith_G1(wo, alpha, side_o, dec, "o")
    # (from which medium the microfacet is met follows the sign of wi.m as computed: a decision of its own where that is doubtful)
    front = dec("front", wim, _absdot(wi, m), side_i == (ci > 0.0))
    F_d, _, _ = fresnel_dielectric(wim, eta_m, dec, front)
    F_c = np.stack([fresnel_conductor(wim, X[:, 7 + c], X[:, 10 + c]) for c in range(3)], -1)
    d_vis = D * g_i * np.abs(wim) / np.abs(ci)          # density of the visible normals
    refl_value = D * g_i * g_o / (4.0 * np.abs(ci))
    refl_pdf = d_vis / (4.0 * np.abs(wom))
    denom = wim + eta * wom
    trans_value = np.abs(wim * wom) * (1.0 - F_d) * g_i * g_o * D * eta * eta / (np.abs(ci) * denom * denom) / (eta * eta)
    trans_pdf = d_vis * (1.0 - F_d) * eta * eta * np.abs(wom) / (denom * denom)
    is_rd = kind == ROUGH_DIELECTRIC
    v_rd = np.where(reflect, F_d * refl_value, trans_value)
    p_rd = np.where(reflect, F_d * refl_pdf, trans_pdf)
    value = np.where(is_rd[:, None], v_rd[:, None] * np.ones(3), F_c * X[:, REFL] * refl_value[:, None])
    pdf = np.where(is_rd, p_rd, refl_pdf)
    # a conductor reflects only, and only above (the wrapper has mirrored a two-sided row)
    # ... and an index ratio of exactly 1 is no interface: light goes straight on, a delta the lobes cannot express -- zeros
    dead = (ci == 0.0) | (~is_rd & ~((ci > 0.0) & (co > 0.0))) | (is_rd & (eta_m == 1.0))
    # the density a sampler gives the direction before anybody asks on which side of the microfacet it left (what a sample
    # of weight 0 still reports), and the pdf proper
    lobe = np.where(side_i & ~dead & np.isfinite(pdf), pdf, 0.0)
    pdf = np.where(side_i & side_o, pdf, 0.0)
    value = np.where(dead[:, None] | ~np.isfinite(value), 0.0, value)
    pdf = np.where(dead | ~np.isfinite(pdf), 0.0, pdf)
    return value, pdf, lobe


def effective_rows(rows, idx, level):
    """(type, one_sided) of every lane as a kernel of feature level `level` reads its row"""
    kind = rows[idx, 0].astype(np.int64)
    one_sided = rows[idx, 11] != 0.0
    if level < 3:
        one_sided = np.zeros_like(one_sided)
        kind = np.where(kind >= CONDUCTOR, DIFFUSE, kind)
    if level < 1:
        kind = np.zeros_like(kind)
    return kind, one_sided


def pack(rows, idx, wi, wo, u1=None):
    """the input matrix: float64 copies of the float32 numbers an implementation is given"""
    n = idx.shape[0]
    X = np.zeros((n, NX))
    X[:, WI], X[:, WO] = np.asarray(wi, np.float32), np.asarray(wo, np.float32)
    r = np.asarray(rows, np.float32)[idx]
    X[:, ALPHA], X[:, ETA], X[:, K], X[:, REFL] = r[:, 4], r[:, 5:8], r[:, 8:11], r[:, 1:4]
    if u1 is not None:
        X[:, U1] = np.asarray(u1, np.float32)
    return X


def eval_core(X, kind, one_sided, forced=None):
    """-> {"value": (n,3), "pdf": (n,), "pdf_lobe": (n,)}, the decisions' record"""
    dec = _Dec(forced)
    X = X.copy()
    with np.errstate(all="ignore"):
        below = X[:, 2] < 0.0
        mirror = below & ~one_sided & (kind != ROUGH_DIELECTRIC)
        X[mirror, 2] *= -1.0
        X[mirror, 5] *= -1.0
        wi, wo = X[:, WI], X[:, WO]
        v_r, p_r, l_r = _rough(X, kind, dec)
        above = (wi[:, 2] > 0.0) & (wo[:, 2] > 0.0)
        p_d = np.where(above, wo[:, 2] / np.pi, 0.0)
        v_d = X[:, REFL] * p_d[:, None]
        rough = (kind == ROUGH_CONDUCTOR) | (kind == ROUGH_DIELECTRIC)
        delta = (kind == CONDUCTOR) | (kind == DIELECTRIC)
        value = np.where(rough[:, None], v_r, v_d)
        pdf = np.where(rough, p_r, p_d)
        value = np.where(delta[:, None], 0.0, value)
        pdf = np.where(delta, 0.0, pdf)
        lobe = np.where(rough, l_r, pdf)
    # decisions that cannot matter are never doubtful: no microfacets, a conductor with a direction below, Snell on a conductor
    idle = ~rough | (wi[:, 2] == 0.0) | ((kind == ROUGH_CONDUCTOR) & ~above) | ((kind == ROUGH_DIELECTRIC) & (X[:, 7] == 1.0))
    for name in dec.b:
        dec.b[name] = np.where(idle | ((name == "tir") & (kind != ROUGH_DIELECTRIC)), np.inf, dec.b[name])
    return {"value": value, "pdf": pdf, "pdf_lobe": lobe}, dec


def delta_core(X, kind, one_sided, forced=None):
    """what sampling a smooth conductor or a smooth dielectric returns: wo, pdf, weight, eta; zeros for any other row"""
    dec = _Dec(forced)
    n = X.shape[0]
    with np.errstate(all="ignore"):
        wi = X[:, WI]
        ci = wi[:, 2]
        F, cos_t, eta_it = fresnel_dielectric(ci, X[:, 7], dec)
        # (F is exact where it is a constant: total internal reflection, the horizon, no interface at all)
        exact = (F == 1.0) | (F == 0.0)
        reflect = dec("lobe", np.where(exact, np.inf, F - X[:, U1]), np.maximum(F, X[:, U1]), X[:, U1] <= F)
        mirror = np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], -1)
        refr = np.stack([-wi[:, 0] / eta_it, -wi[:, 1] / eta_it, cos_t], -1)
        is_d = kind == DIELECTRIC
        wo_d = np.where(reflect[:, None], mirror, refr)
        pdf_d = np.where(reflect, F, 1.0 - F)
        w_d = np.where(reflect, 1.0, 1.0 / (eta_it * eta_it))[:, None] * np.ones(3)
        eta_d = np.where(reflect, 1.0, eta_it)
        ok_c = (kind == CONDUCTOR) & ((ci > 0.0) | ((ci < 0.0) & ~one_sided))
        F_c = np.stack([fresnel_conductor(ci, X[:, 7 + c], X[:, 10 + c]) for c in range(3)], -1) * X[:, REFL]
        z3 = np.zeros((n, 3))
        out = {
            "wo": np.where(is_d[:, None], wo_d, np.where(ok_c[:, None], mirror, z3)),
            "pdf": np.where(is_d, pdf_d, np.where(ok_c, 1.0, 0.0)),
            "weight": np.where(is_d[:, None], w_d, np.where(ok_c[:, None], F_c, z3)),
            "eta": np.where(is_d, eta_d, np.where(ok_c, 1.0, 0.0)),
            "delta": np.where(is_d | ok_c, 1.0, 0.0),
        }
    for name in dec.b:
        dec.b[name] = np.where(is_d, dec.b[name], np.inf)
    return out, dec


# ---- conditioning -----------------------------------------------------------------------------------------------------------
def _ulp(X):
    """one unit in the last place of every float32 input (0 for an input that is exactly 0: its products are exact)"""
    x32 = X.astype(np.float32)
    h = np.spacing(np.abs(x32)).astype(np.float64)
    return np.where(x32 == 0.0, 0.0, h)


class Answer:
    """q[name], the sensitivities dq[name] = sum_j |dq_j| and the decisions' margins of one evaluation"""

    def __init__(self, q, dq, doubtful, taken):
        self.q, self.dq, self.doubtful, self.taken = q, dq, doubtful, taken

    def band(self, name, ops, C):
        q = self.q[name]
        o = ops if np.ndim(ops) == 0 or np.ndim(q) == 1 else np.asarray(ops)[:, None]
        return C * (U * o * np.abs(q) + self.dq[name]) + TINY


def conditioned(core, X, kind, one_sided, forced=None):
    """core's answer with every decision held at what it is at X (or at `forced`), its sensitivities, and which decisions
    are within their reach of going the other way"""
    q0, d0 = core(X, kind, one_sided, forced)
    held = dict(d0.taken)
    h = _ulp(X)
    dq = {k: np.zeros_like(v) for k, v in q0.items()}
    db = {k: np.zeros_like(v, dtype=np.float64) for k, v in d0.b.items()}
    for j in range(NX):
        if not h[:, j].any():
            continue
        best = {k: np.zeros_like(v) for k, v in q0.items()}
        bestb = {k: np.zeros_like(v) for k, v in db.items()}
        for s in (1.0, -1.0):
            Xp = X.copy()
            Xp[:, j] += s * h[:, j]
            q, d = core(Xp, kind, one_sided, held)
            with np.errstate(all="ignore"):
                for k in q0:
                    diff = np.abs(q[k] - q0[k])
                    best[k] = np.maximum(best[k], np.where(np.isfinite(diff), diff, np.inf))
                for k in db:
                    diff = np.abs(d.b[k] - d0.b[k])
                    bestb[k] = np.maximum(bestb[k], np.where(np.isfinite(diff), diff, 0.0))
        for k in q0:
            dq[k] += best[k]
        for k in db:
            db[k] += bestb[k]
    doubtful = {}
    with np.errstate(all="ignore"):
        for k in d0.b:
            # (... and below float32's normal numbers a product may have vanished; an exact 0 is a 0 in float32 too)
            reach = BRANCH_C * (U * BRANCH_OPS * np.abs(d0.scale[k]) + db[k]) + np.where(d0.b[k] == 0.0, 0.0, TINY)
            doubtful[k] = np.isfinite(d0.b[k]) & (np.abs(d0.b[k]) <= reach) & (reach > 0.0)
    return Answer(q0, dq, doubtful, held)


def candidates(core, X, kind, one_sided, most=5, base=None):
    """-> (natural Answer, ambiguous (n,) bool, [(lanes, Answer)]): the answers of the lanes that have doubtful decisions
    under every assignment of those decisions (one decision can change what another compares -- which of +-m points up
    decides the sides -- so the doubtful ones are SET, both ways, and all others follow naturally).  A lane with more than
    `most` doubtful decisions gets the assignments of its first `most`."""
    base = base or {}   # decisions the caller knows (which lobe a sample says it took): held in every answer, never doubtful
    nat = conditioned(core, X, kind, one_sided, base)
    names = [k for k in nat.doubtful if nat.doubtful[k].any() and k not in base]
    out = []
    if not names:
        return nat, np.zeros(X.shape[0], bool), out
    flags = np.stack([nat.doubtful[k] for k in names], -1)
    amb = flags.any(-1)
    for pattern in np.unique(flags[amb], axis=0):
        lanes = np.nonzero((flags == pattern).all(-1))[0]
        which = [k for k, f in zip(names, pattern) if f][:most]
        for values in itertools.product((False, True), repeat=len(which)):
            forced = {k: np.full(lanes.size, v) for k, v in zip(which, values)}
            forced.update({k: v[lanes] for k, v in base.items()})
            out.append((lanes, conditioned(core, X[lanes], kind[lanes], one_sided[lanes], forced)))
    return nat, amb, out


def phi_switch(rows, idx, wi):
    """sincos_phi's switch in sampling the visible normals (sin^2 of the stretched wi against 4 * 2^-24): True where it is
    within reach of going either way.  For reporting: it changes which direction a u gives, not the density."""
    a = np.abs(np.asarray(rows, np.float64)[idx, 4])
    w = np.asarray(wi, np.float64) * np.stack([a, a, np.ones_like(a)], -1)
    with np.errstate(all="ignore"):
        s2 = (w[:, 0] ** 2 + w[:, 1] ** 2) / _dot(w, w)
    return np.abs(s2 - 4.0 * 2.0 ** -24) <= BRANCH_C * U * BRANCH_OPS * s2


# ---- judging outputs --------------------------------------------------------------------------------------------------------
def _ops(kind, what):
    table = {DIFFUSE: OPS["diffuse"], ROUGH_CONDUCTOR: OPS["rc_" + what], CONDUCTOR: 1, DIELECTRIC: 1, ROUGH_DIELECTRIC: OPS["rd_" + what]}
    return np.array([table[t] for t in range(5)], np.float64)[kind]


def _within(got, ans, name, ops, C):
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        ok = np.abs(got - ans.q[name]) <= ans.band(name, ops, C)
    return ok.all(-1) if ok.ndim == 2 else ok


def _ratio(got, ans, name, ops):
    """|difference| over the band's bracket (the band with C = 1): what BAND_C is measured from"""
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(got - ans.q[name]) / ans.band(name, ops, 1.0)
    r = np.where(np.isfinite(r), r, np.where(np.abs(got - ans.q[name]) == 0, 0.0, np.inf))
    return r.max(-1) if r.ndim == 2 else r


class Verdict:
    """ok (n,) bool: the output is in the band of the natural answer or, on an ambiguous lane, of a candidate's;
    ambiguous (n,) bool; ratio (n,): the natural answer's ratio on unambiguous lanes (0 elsewhere), per quantity"""

    def __init__(self, ok, ambiguous, ratio, why=None):
        self.ok, self.ambiguous, self.ratio, self.why = ok, ambiguous, ratio, why or {}

    def failures(self):
        return np.nonzero(~self.ok)[0]


def judge_eval(rows, idx, wi, wo, value, pdf, level=3, C=None):
    """an implementation's eval outputs against the model"""
    C = C or BAND_C
    kind, one_sided = effective_rows(np.asarray(rows), idx, level)
    X = pack(rows, idx, wi, wo)
    nat, amb, cands = candidates(eval_core, X, kind, one_sided)
    return _judge(nat, amb, cands, {"value": (value, _ops(kind, "value"), C["value"]), "pdf": (pdf, _ops(kind, "pdf"), C["pdf"])})


def _judge(nat, amb, cands, outputs):
    """outputs: {quantity: (what the implementation returned, ops, C)}.  A lane whose doubtful decisions all lead to the
    natural answer (within its band) is not ambiguous: there is one answer."""
    n = amb.shape[0]
    ok = np.ones(n, bool)
    for name, (got, ops, C) in outputs.items():
        ok &= _within(got, nat, name, ops, C)
    differs = np.zeros(n, bool)
    ok_natural = ok.copy()
    for lanes, ans in cands:
        good = np.ones(lanes.size, bool)
        same = np.ones(lanes.size, bool)
        for name, (got, ops, C) in outputs.items():
            o = ops[lanes] if np.ndim(ops) else ops
            good &= _within(np.asarray(got)[lanes], ans, name, o, C)
            with np.errstate(all="ignore"):
                near = np.abs(ans.q[name] - nat.q[name][lanes]) <= nat.band(name, ops, C)[lanes]
            same &= near.all(-1) if near.ndim == 2 else near
        ok[lanes] |= good
        differs[lanes] |= ~same | (good & ~ok_natural[lanes])   # (... or has the same answer with another band, and needs it)
    amb = amb & differs
    ratio = {name: np.where(amb, 0.0, _ratio(got, nat, name, ops)) for name, (got, ops, C) in outputs.items()}
    why = {k: int((d & amb).sum()) for k, d in nat.doubtful.items() if (d & amb).any()}
    return Verdict(ok, amb, ratio, why)


def judge_sample(rows, idx, wi, u, swo, spdf, weight, eta, delta, level=3, C=None):
    """an implementation's sample outputs against the model.  Non-delta rows: at the direction returned, the returned pdf is
    the model's pdf and weight * pdf the model's value (a failed sample -- pdf 0 -- is left to the density test, which
    compares the valid fraction with the pdf's mass); eta is 1 for a reflection and the index ratio along wi for a
    transmission, delta 0.  Delta rows: direction, pdf, weight, eta and the flag are the model's mirror or refracted direction."""
    C = C or BAND_C
    rows = np.asarray(rows)
    kind, one_sided = effective_rows(rows, idx, level)
    swo = np.asarray(swo, np.float32)
    spdf64, w64 = np.asarray(spdf, np.float64), np.asarray(weight, np.float64)
    is_delta = (kind == CONDUCTOR) | (kind == DIELECTRIC)
    failed = ~is_delta & (spdf64 == 0.0)
    ok = ~failed | ((swo == 0).all(-1) & (w64 == 0).all(-1))
    # A direction of weight 0 -- a reflection that ends below the macro-surface, its microfacet's back -- carries nothing and
    # the density test counts it with the failed ones; its pdf is still the density of the lobe it says it took (eta 1: the
    # reflection), at the direction it returned, and is held to that below.
    weightless = ~failed & ~is_delta & (w64 == 0).all(-1)
    failed |= weightless
    live = ~is_delta & ~failed
    ok &= is_delta | (np.asarray(delta) == 0)
    wi32 = np.asarray(wi, np.float32)
    eta_m = rows[idx, 5].astype(np.float32)
    with np.errstate(all="ignore"):
        crossed = (swo[:, 2] * wi32[:, 2] < 0) & (kind == ROUGH_DIELECTRIC)
        want_eta = np.where(crossed, np.where(wi32[:, 2] > 0, eta_m, np.float32(1.0) / eta_m), np.float32(1.0))
    ok &= ~live | (np.asarray(eta, np.float32) == want_eta)
    # -- non-delta rows at the returned direction: pdf, and weight * pdf as the value
    k_eval = np.where(is_delta, DIFFUSE, kind)
    nat, amb, cands = candidates(eval_core, pack(rows, idx, wi, swo), k_eval, one_sided)
    ops_v, ops_p = _ops(k_eval, "value"), _ops(k_eval, "pdf")
    with np.errstate(all="ignore"):
        wp = w64 * spdf64[:, None]
    # (the product's band: the value's, and the pdf's carried by the weight)
    for a in [nat] + [c for _, c in cands]:
        a.q["wp"] = a.q["value"]
    nat.dq["wp"] = nat.dq["value"] + np.abs(w64) * (U * ops_p * np.abs(nat.q["pdf"]) + nat.dq["pdf"])[:, None]
    for lanes, c in cands:
        c.dq["wp"] = c.dq["value"] + np.abs(w64[lanes]) * (U * ops_p[lanes] * np.abs(c.q["pdf"]) + c.dq["pdf"])[:, None]
    v = _judge(nat, amb & live, cands, {"pdf": (spdf64, ops_p, C["sample"]), "wp": (wp, ops_v, C["sample"])})
    ok &= ~live | v.ok
    ratio = {"sample_pdf": np.where(live, v.ratio["pdf"], 0.0), "sample_value": np.where(live, v.ratio["wp"], 0.0)}
    # -- weightless directions: the lobe's density
    if weightless.any():
        z = np.nonzero(weightless)[0]
        took_reflection = np.where((kind[z] == ROUGH_DIELECTRIC), np.asarray(eta, np.float32)[z] == 1.0, True)
        nz, az, cz = candidates(eval_core, pack(rows, idx[z], np.asarray(wi)[z], swo[z]), k_eval[z], one_sided[z], base={"reflect": took_reflection})
        vz = _judge(nz, az, cz, {"pdf_lobe": (spdf64[z], ops_p[z], C["sample"])})
        ok[z] &= vz.ok   # (in the band or a branch answer, like every lane; but a direction that carries nothing is not
        # counted into the ambiguous share, which speaks of the lanes that have an answer somebody uses)
        ratio["weightless_pdf"] = np.zeros(idx.shape[0])
        ratio["weightless_pdf"][z] = vz.ratio["pdf_lobe"]
    # -- delta rows
    natd, ambd, candsd = candidates(delta_core, pack(rows, idx, wi, swo, u[:, 0]), kind, one_sided)
    outs = {"wo": (swo, OPS["refract"], C["delta"]), "pdf": (spdf64, OPS["fresnel_d"], C["delta"]),
            "weight": (w64, OPS["fresnel_c"], C["delta"]), "eta": (np.asarray(eta, np.float64), 1, C["delta"]),
            "delta": (np.asarray(delta, np.float64), 0, 1.0)}
    vd = _judge(natd, ambd & is_delta, candsd, outs)
    ok &= ~is_delta | vd.ok
    for k, r in vd.ratio.items():
        ratio["delta_" + k] = np.where(is_delta, r, 0.0)
    return Verdict(ok, (v.ambiguous & live) | (vd.ambiguous & is_delta), ratio, {**v.why, **vd.why})
