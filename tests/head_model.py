"""The head of one path vertex in float64 numpy, written from the reference's lines (path_guiding_integrator.py:16-24, 185-220,
272-297) and not from either implementation: what pgo_head_probe (oracle) and pg_head_probe (device) are held to.  The
committed models of the stages are composed, not restated: surface_model (the surface at the hit, the hit density of emitter
sampling), emitter_model (the emitter sample and its shadow ray), bsdf_model (the BSDF towards the emitter sample and at the
sampled direction) and vertex_model's PCG32 and its widening of a BSDF band under a frame's roundings.

A lane is judged stage by stage, and every stage takes the probe's OWN float32 outputs of the stage before it as exact inputs,
so that the committed bands apply unchanged:
  surface       surface_model at (prim, ray, t, uv): p, n, refl in their bands (a doubtful decision: either assignment), ng and
                the material row exact.  A miss: p = 0, n = ng = (0, 0, 1), refl = 0, row 0, no flag but what follows.
  wi            to_local(frame(n_out), -ray_d), the frame Duff et al.'s.
  emission      radiance only on an emitter with wi_out.z > 0; emitter_pdf = surface_model.emitter_pdf(prev_p, p_out, n_out), 0
                where prev_delta or no emitter was hit; mis = a^2 / (a^2 + b^2) of (prev_bsdf_pdf, emitter_pdf) in float32's
                range (a square that overflows is inf, and inf / inf a NaN), 0 for a <= 0 or NaN; Le = thr mis radiance.
                HAS_LE exactly where Le_out has a non-zero bit.
  active_next   depth + 1 < max_depth (uint32) and VALID.  active_em = active_next and Smooth: every row is smooth below
                level 3 (bsdf_model.effective_rows), conductor and dielectric rows are not at level 3.
  draws         e1, e2 unmasked; then, where active_next only, s1, s2x, s2y and the pick u (PCG32, vertex_model's): 2 or 6
                draws, the state afterwards bit for bit.
  emitter       where active_em: emitter_model.judge at p = p_out, n = ng_out, e = (e1, e2), its need_shadow the emitter's own
                (density > 0, or a delta light).  Elsewhere the no-sample values bit for bit.  ACTIVE_EM = active_em and
                ds_pdf_out != 0.
  bv_em, bp_em  where ACTIVE_EM: bsdf_model at (wi_out, to_local(frame(n_out), ds_d_out)), its committed band widened by the
                frame's roundings of the local direction (vertex_model.tree_bsdf); else zero.
  NEE_LIVE      ACTIVE_EM and not (bv_em_out exactly zero and em_w_out finite); NEED_SHADOW = NEE_LIVE and the emitter's own.
  BSDF sample   where active_next: at to_local(frame(n_out), wo_out) the returned pdf is the model's pdf and weight pdf the
                model's value (same widened band); eta 1 unless a rough dielectric was crossed; on a diffuse row the direction
                itself is Mitsuba's square_to_cosine_hemisphere(s2x, s2y), mirrored with wi below a two-sided surface; a delta
                row returns bsdf_model.delta_core's mirror or refracted direction, pdf, weight, eta at u1 = s1; wo_out a unit
                vector.  Elsewhere the failed sample's zeros.
  classes       DELTA as sampled; DO_MIS = active_next, not DELTA, guided; SMP_TREE = (u > f) and DO_MIS (two float32 numbers:
                exact); BSDF_MIS = DO_MIS and not SMP_TREE.

New brackets (surface_model.bracket's form, C (2^-24 ops |q| + sum_j |dq/dx_j| step_j)), ops the float32 roundings on the path:
  wi      11   Duff's frame of n_out (6) and a 3-term dot product (5); |q| := sum_k |d_k| (the frame's components are <= 1)
  Le       6   two squares, a sum, a quotient, two products; the hit density enters with surface_model's committed band as its step
  unit    24   |wo_out| - 1: the sampled local direction's normalisation (8) and to_world in a 16-rounding frame; |q| := 1
  dir     32   local(wo_out) - cosine_hemisphere(s2x, s2y): the warp (2 u - 1, a quotient, two products, sincos, two products,
               the root: 16) and the frame's 16 there and back; |q| := 1; z = sqrt(1 - r^2) carries 2 2^-24 / z besides (the
               four roundings of 1 - r^2 through the root's slope 1 / (2 z))
C per quantity (BAND_C) is four times the worst ratio measured on the CPU oracle over the suite's broad sets
(profiles/head/band.txt, written by tools/head_mutants.py --band).

Ambiguous, and accepted under either assignment: a doubtful decision of a composed model (surface_model's, emitter_model's
choice, facing, side, inside; bsdf_model.candidates); the model's own wi.z within its band of 0 on an emitter (Le with or
without the radiance); a^2 or a^2 + b^2 below 2^-120 or within 2^-20 of float32's largest number (a product that may have
vanished or overflowed); the local z of wo_out within the frame's roundings of 0 on a rough dielectric (eta either way).
Whether the emitter sample is live is a function of the probe's own bv_em_out and em_w_out, which are judged: no assignment is
needed.  The pick u > f compares two float32 numbers: never ambiguous."""
import numpy as np

import bsdf_model as BM
import emitter_model as EM
import surface_model as SM
import vertex_model as VM

F_VALID, F_ACTIVE_NEXT, F_ACTIVE_EM, F_NEED_SHADOW, F_DS_DELTA, F_DELTA, F_DO_MIS, F_SMP_TREE, F_BSDF_MIS, F_NEE_LIVE, F_HAS_LE = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
EPS = SM.EPS
AMBIGUOUS_CAP = SM.AMBIGUOUS_CAP
FLT_MAX = float(np.finfo(np.float32).max)
VANISHING = VM.VANISHING
FRAME_OPS = VM.FRAME_OPS
OPS = {"wi": 11, "Le": 6, "unit": 24, "dir": 32}
# four times the worst |difference| / bracket measured on the oracle (profiles/head/band.txt); 64 would mean a missing term
BAND_C = {"wi": 0.50, "Le": 0.97, "unit": 1.18, "dir": 1.57}
VECTORS = ("p", "n", "ng", "wi", "refl", "Le", "ds_d", "em_w", "bv_em", "sh_o", "sh_d", "wo", "bsdf_w")
SCALARS = ("ds_pdf", "bp_em", "sh_tmax", "bsdf_pdf", "eta")


class Params:
    def __init__(self, max_depth, frac, guided):
        self.max_depth, self.frac, self.guided = int(max_depth), float(np.float32(frac)), bool(guided)

    def args(self):
        return self.max_depth, self.frac, self.guided


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _dot(a, b):
    return (a * b).sum(-1)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    same = a.view(np.uint32) == b.view(np.uint32)
    return same.all(-1) if same.ndim == 2 else same


def _zero(a):
    z = np.asarray(a) == 0
    return z.all(-1) if z.ndim == 2 else z


def frame(n):
    """Duff's frame of the float32 normals n (the sign that of the float32 n.z itself) -> s, t"""
    return SM.duff(n, np.where(np.signbit(n[:, 2]), -1.0, 1.0))


def to_local(n, v):
    s, t = frame(n)
    return np.stack([_dot(v, s), _dot(v, t), _dot(v, n)], -1)


def rows_of(T, level):
    """the material table a kernel of this level reads (level 0 reads none: one two-sided diffuse row stands for the quads')"""
    return np.zeros((1, 16), np.float32) if T.mats is None or level == 0 else T.mats.astype(np.float32)


def draws(I, active_next):
    """the head's sampler draws -> (e (n,2), s (n,3), u (n,), the state afterwards, the number of draws)"""
    st, inc = np.asarray(I["rng_state"], np.uint64), np.asarray(I["rng_inc"], np.uint64)
    got = []
    for k in range(6):
        x, nxt = VM.pcg32_draw(st, inc)
        if k >= 2:                       # masked by active_next: the value is 0 and the state stays
            x, nxt = np.where(active_next, x, 0.0), np.where(active_next, nxt, st)
        got.append(x)
        st = nxt
    return np.stack(got[0:2], -1), np.stack(got[2:5], -1), got[5], st, np.where(active_next, 6, 2)


@np.errstate(all="ignore")
def power_f32(a, b):
    """:16-24 in float32's range: a^2 / (a^2 + b^2), 0 for a <= 0 or NaN; a square or a sum beyond float32 is inf"""
    over = lambda x: np.where(np.abs(x) > FLT_MAX, np.inf, x)
    a2 = over(a * a)
    r = np.where(a > 0.0, a2 / over(b * b + a2), 0.0)
    return np.where(np.isnan(r), 0.0, r)


@np.errstate(all="ignore")
def cosine_hemisphere(u, v):
    """Mitsuba's warp::square_to_cosine_hemisphere (the concentric disk, z = safe_sqrt(1 - r^2))"""
    x, y = 2.0 * u - 1.0, 2.0 * v - 1.0
    q13 = np.abs(x) < np.abs(y)
    r, rp = np.where(q13, y, x), np.where(q13, x, y)
    phi = 0.25 * np.pi * rp / r
    phi = np.where(q13, 0.5 * np.pi - phi, phi)
    phi = np.where((x == 0.0) & (y == 0.0), 0.0, phi)
    px, py = r * np.cos(phi), r * np.sin(phi)
    return np.stack([px, py, np.sqrt(np.maximum(1.0 - (px * px + py * py), 0.0))], -1)


def _ratio(got, q, b):
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        r = np.where((got == q) | (np.isnan(got) & np.isnan(q)), 0.0, np.abs(got - q) / (b + 4 * VM.SUBNORMAL))
    r = np.where(np.isnan(r), np.inf, r)
    return r.max(-1) if r.ndim == 2 else r


def _bsdf_at(rows, level, n, wi, refl, mat, wo, lanes):
    """bsdf_model's value and pdf at (wi, to_local(frame(n), wo)) on `lanes`, the band widened by the frame's roundings
    -> (natural vertex_model.Bsdf over all lanes, doubtful (n,), [(lanes, Bsdf)] the candidates)"""
    flags = np.where(lanes, VM.F_SMP_TREE, 0)
    return VM.tree_bsdf(rows, dict(flags=flags, n=n, wo=wo, wi=wi, mat=mat, refl=refl), level)


@np.errstate(all="ignore")
def _bsdf_ok(nat, cands, value, pdf, extra=None):
    """value (n,3) and pdf (n,) within the natural answer's band, or a candidate's -> (ok (n,), ratio to the natural band (n,))"""
    value, pdf = np.asarray(value, np.float64), np.asarray(pdf, np.float64)
    extra = np.zeros_like(value) if extra is None else extra

    def within(b, sel=slice(None)):
        dv = b.d_value + extra[sel] * b.d_pdf[:, None] if extra is not None else b.d_value
        okv = (np.abs(value[sel] - b.value) <= dv) | (value[sel] == b.value)
        okp = (np.abs(pdf[sel] - b.pdf) <= b.d_pdf) | (pdf[sel] == b.pdf)
        r = np.maximum(np.where(value[sel] == b.value, 0.0, np.abs(value[sel] - b.value) / dv).max(-1),
                       np.where(pdf[sel] == b.pdf, 0.0, np.abs(pdf[sel] - b.pdf) / b.d_pdf))
        return okv.all(-1) & okp, np.nan_to_num(r, nan=np.inf)

    ok, ratio = within(nat)
    for lanes, b in cands:
        ok[lanes] |= within(b, lanes)[0]
    return ok, ratio


@np.errstate(all="ignore")
def judge(T, level, I, P, out, C=None):
    """an implementation's outputs (the columns of pg_head_out, the sampler's new state as "rng_out") for the lanes I (the
    columns of pg_head_lanes) of the scene with tables T (emitter_model.Tables) against the model
    -> ({check: lanes that fail}, {quantity: (n,) ratio to its bracket, 0 on ambiguous lanes}, ambiguous (n,) bool)"""
    C = C or BAND_C
    prim = np.asarray(I["prim"], np.int64)
    n_l = prim.shape[0]
    o, d, thr, prev_p = (_f64(I[k]).reshape(n_l, 3) for k in ("ray_o", "ray_d", "thr", "prev_p"))
    uv = _f64(I["uv"]).reshape(n_l, 2)
    g = {k: _f64(out[k]) for k in VECTORS + SCALARS}
    flags = np.asarray(out["flags"]).astype(np.int64)
    has = lambda bit: (flags & bit) != 0
    ok, ratio = {}, {}
    amb = np.zeros(n_l, bool)
    valid = prim >= 0
    hit = np.nonzero(valid)[0]
    everywhere = lambda sub, fill=True: np.where(valid, np.put(x := np.full(n_l, fill), hit, sub) or x, fill)

    # ---- the surface ----
    m = SM.surface(T, prim[hit], o[hit], d[hit], _f64(I["t"])[hit], uv[hit, 0], uv[hit, 1])

    def banded(q, got, c):
        good = SM._within(got, q.q, q.b, c) | (q.amb & SM._within(got, q.alt, q.alt_b, c))
        return good, np.where(q.amb, 0.0, SM._ratio(got, q.q, q.b))

    good, ratio["p"] = (everywhere(x, y) for x, y in zip(banded(m.p, g["p"][hit], SM.BAND_C["p"]), (True, 0.0)))
    ok["p"] = good
    good, r = banded(m.n, g["n"][hit], SM.BAND_C["n"])
    any_unit = getattr(m.n, "any_unit", None)
    if any_unit is not None and any_unit.any():
        good |= any_unit & (np.abs(_dot(g["n"][hit], g["n"][hit]) - 1) <= SM.BAND_C["frame"] * EPS * SM.OPS["frame"])
    ok["n"], ratio["n"] = everywhere(good), everywhere(r, 0.0)
    flat = m.kind != 1
    ok["ng"] = everywhere(np.where(flat, (g["ng"][hit] == m.ng).all(-1), _bits(out["ng"][hit], out["n"][hit])))
    good, r = banded(m.refl, g["refl"][hit], SM.BAND_C["refl"])
    any_texel = m.refl.amb & np.isinf(m.refl.alt_b).any(-1) & (g["refl"][hit] >= 0).all(-1) & (g["refl"][hit] <= 1).all(-1)
    ok["refl"] = everywhere(np.where(m.textured, good | any_texel, (g["refl"][hit] == m.refl.q).all(-1)))
    ratio["refl"] = everywhere(np.where(m.textured, r, 0.0), 0.0)
    row = np.zeros(n_l, np.int64)
    row[hit] = 0 if level == 0 else m.row
    mat = np.asarray(out["mat"], np.int64)
    ok["mat"] = mat == row
    amb[hit] |= m.p.amb | m.n.amb | (m.refl.amb & m.textured)
    miss = ~valid
    unit_z = np.array([0.0, 0.0, 1.0])
    ok["miss"] = valid | (_zero(out["p"]) & (g["n"] == unit_z).all(-1) & (g["ng"] == unit_z).all(-1) & _zero(out["refl"]) & _zero(out["Le"])
                          & ((flags & ~F_VALID) == (flags & (F_VALID - 1))) & (flags == 0))
    ok["valid"] = has(F_VALID) == valid
    mat = np.where(ok["mat"], mat, 0)   # (a wrong row has failed already: the later stages must not index with it)

    # ---- wi ----
    n_out, wi = g["n"], g["wi"]
    wq, wb = SM.bracket(lambda d_, n_: -to_local(n_, d_), [d, n_out], OPS["wi"], scale=np.abs(d).sum(-1)[:, None] * np.ones(3), nan_is_inf=True)
    ok["wi"] = SM._within(wi, wq, wb, C["wi"])
    ratio["wi"] = SM._ratio(wi, wq, wb)

    # ---- emission ----
    is_em = np.zeros(n_l, bool)
    is_em[hit] = m.is_em != 0
    radiance = np.zeros((n_l, 3))
    radiance[hit] = m.radiance
    e = SM.emitter_pdf(T, m, prev_p[hit], out["p"][hit], out["n"][hit])
    counted = (is_em & (np.asarray(I["prev_delta"]) == 0))[hit]
    full = lambda x: np.put(y := np.zeros(n_l), hit, np.where(counted, x, 0.0)) or y
    b_q, b_b, b_alt, b_alt_b = full(e.q), full(SM.BAND_C["pdf"] * e.b), full(e.alt), full(SM.BAND_C["pdf"] * e.alt_b)
    b_amb, b_graze = np.zeros(n_l, bool), np.zeros(n_l, bool)
    b_amb[hit], b_graze[hit] = e.amb & counted, e.graze & counted
    b_least = np.put(y := np.full(n_l, np.inf), hit, e.at_least) or y
    a = _f64(I["prev_bsdf_pdf"])
    front = wi[:, 2] > 0.0
    le = lambda thr_, a_, b_, rad_: thr_ * power_f32(a_, b_)[:, None] * rad_

    def le_ok(rad, b, step):
        q, br = SM.bracket(le, [thr, a, b, rad], OPS["Le"], steps=[None, None, step, None], nan_is_inf=True)
        return ((np.abs(g["Le"] - q) <= C["Le"] * br + 4 * VM.SUBNORMAL) | (g["Le"] == q)).all(-1), _ratio(g["Le"], q, br)

    rad = np.where((is_em & front)[:, None], radiance, 0.0)
    good, ratio["Le"] = le_ok(rad, b_q, b_b)
    other = np.where((is_em & ~front)[:, None], radiance, 0.0)      # (... with the model's own wi.z on the other side of 0)
    doubt_wi = is_em & (np.abs(wq[:, 2]) <= C["wi"] * wb[:, 2])
    good |= doubt_wi & le_ok(other, b_q, b_b)[0]
    good |= b_amb & le_ok(rad, b_alt, b_alt_b)[0]
    top = le(thr, a, np.where(b_graze, b_least, 0.0), rad)
    good |= b_graze & ((g["Le"] >= 0.0) & (g["Le"] <= top * (1 + 64 * EPS))).all(-1)
    a2, den = a * a, a * a + b_q * b_q
    edge = lambda x: ((x > 0) & (x < VANISHING)) | (np.abs(x / FLT_MAX - 1.0) <= 2.0 ** -20)
    doubt_range = is_em & front & (edge(a2) | edge(den))
    ok["Le"] = good | doubt_range
    le_amb = doubt_wi | b_amb | b_graze | doubt_range
    amb |= le_amb
    ratio["Le"] = np.where(le_amb, 0.0, ratio["Le"])
    ok["HAS_LE"] = has(F_HAS_LE) == (np.ascontiguousarray(out["Le"], np.float32).view(np.uint32) != 0).any(-1)

    # ---- active_next, active_em, the draws ----
    depth = np.asarray(I["depth"]).astype(np.int64)
    active_next = valid & (((depth + 1) & 0xFFFFFFFF) < P.max_depth)
    ok["ACTIVE_NEXT"] = has(F_ACTIVE_NEXT) == active_next
    rows = rows_of(T, level)
    kind, one_sided = BM.effective_rows(rows, mat, level)
    kind, one_sided = np.where(valid, kind, BM.DIFFUSE), one_sided & valid
    is_delta = (kind == BM.CONDUCTOR) | (kind == BM.DIELECTRIC)
    active_em0 = active_next & ~is_delta
    e12, s, u, state, count = draws(I, active_next)
    ok["sampler"] = np.asarray(out["rng_out"], np.uint64) == state

    # ---- the emitter sample ----
    sel = np.nonzero(active_em0)[0]
    ds_delta = has(F_DS_DELTA)
    need_own = (g["ds_pdf"] > 0.0) | ds_delta       # (the emitter's own need_shadow: a density > 0, or a delta light)
    em_out = dict(ds_d=out["ds_d"][sel], ds_pdf=out["ds_pdf"][sel], em_weight=out["em_w"][sel], sh_o=out["sh_o"][sel], sh_d=out["sh_d"][sel],
                  sh_tmax=out["sh_tmax"][sel], ds_delta=ds_delta[sel].astype(np.int32), need_shadow=need_own[sel].astype(np.int32))
    ok["emitter sample"] = np.ones(n_l, bool)
    if sel.size:
        bad_e, ratio_e, amb_e, _ = EM.judge(T, out["p"][sel], out["ng"][sel], e12[sel].astype(np.float32), em_out)
        for k, lanes in bad_e.items():
            ok["emitter sample"][sel[lanes]] = False
            ok.setdefault("emitter: " + k, np.ones(n_l, bool))[sel[lanes]] = False
        amb[sel] |= amb_e
        for k, r in ratio_e.items():
            ratio["emitter " + k] = np.put(y := np.zeros(n_l), sel, r) or y
    none = ~active_em0
    ok["no emitter sample"] = ~none | (_bits(out["ds_d"], np.zeros(3)) & _bits(out["ds_pdf"], 0.0) & _bits(out["em_w"], np.zeros(3)) &
                                       _bits(out["sh_o"], np.zeros(3)) & _bits(out["sh_d"], unit_z) & _bits(out["sh_tmax"], 0.0) & ~ds_delta)
    active_em = active_em0 & (g["ds_pdf"] != 0.0)
    ok["ACTIVE_EM"] = has(F_ACTIVE_EM) == active_em

    # ---- the BSDF towards the emitter sample ----
    nat, amb_b, cands = _bsdf_at(rows, level, out["n"], out["wi"], out["refl"], mat, out["ds_d"], active_em)
    good, r = _bsdf_ok(nat, cands, g["bv_em"], g["bp_em"])
    ok["bv_em, bp_em"] = np.where(active_em, good, _bits(out["bv_em"], np.zeros(3)) & _bits(out["bp_em"], 0.0))
    ratio["bsdf_em"] = np.where(active_em & ~amb_b, r, 0.0)
    amb |= amb_b & active_em
    live = active_em & ~(_zero(out["bv_em"]) & np.isfinite(g["em_w"]).all(-1))
    ok["NEE_LIVE"] = has(F_NEE_LIVE) == live
    ok["NEED_SHADOW"] = has(F_NEED_SHADOW) == (live & need_own)

    # ---- the BSDF sample ----
    wo, w, pdf, eta = g["wo"], g["bsdf_w"], g["bsdf_pdf"], g["eta"]
    local = to_local(n_out, wo)
    off = ~active_next
    ok["no BSDF sample"] = ~off | (_zero(out["wo"]) & _zero(out["bsdf_w"]) & (pdf == 0.0) & (eta == 0.0) & ~has(F_DELTA))
    rough = active_next & ~is_delta
    failed = rough & (pdf == 0.0)
    weightless = rough & ~failed & _zero(out["bsdf_w"])
    sampled = rough & ~failed & ~weightless
    ok["failed BSDF sample"] = ~failed | _zero(out["bsdf_w"])
    nat, amb_s, cands = _bsdf_at(rows, level, out["n"], out["wi"], out["refl"], mat, out["wo"], sampled)
    good, r = _bsdf_ok(nat, cands, w * pdf[:, None], pdf, np.abs(w))
    ok["BSDF sample: pdf and weight * pdf at wo"] = ~sampled | good
    ratio["bsdf_sample"] = np.where(sampled & ~amb_s, r, 0.0)
    amb |= amb_s & sampled
    eta_row = rows[mat, 5].astype(np.float64)
    crossed = (local[:, 2] * wi[:, 2] < 0.0) & (kind == BM.ROUGH_DIELECTRIC)
    want_eta = lambda x: np.where(x, np.where(wi[:, 2] > 0.0, eta_row, _f64(np.float32(1.0) / rows[mat, 5])), 1.0)
    doubt_eta = (kind == BM.ROUGH_DIELECTRIC) & (np.abs(local[:, 2]) <= FRAME_OPS * EPS)
    ok["eta"] = ~sampled | (eta == want_eta(crossed)) | (doubt_eta & (eta == want_eta(~crossed)))
    amb |= doubt_eta & sampled
    unit_b = EPS * OPS["unit"]
    length = np.sqrt(_dot(wo, wo))
    directed = active_next & ~failed & ~(is_delta & (pdf == 0.0))
    ok["wo is a unit vector"] = ~directed | (np.abs(length - 1.0) <= C["unit"] * unit_b)
    ratio["unit"] = np.where(directed, np.abs(length - 1.0) / unit_b, 0.0)
    diffuse = active_next & (kind == BM.DIFFUSE) & ~failed
    flip = (wi[:, 2] < 0.0) & ~one_sided
    want = cosine_hemisphere(s[:, 1], s[:, 2]) * np.where(flip, -1.0, 1.0)[:, None] ** np.array([0, 0, 1])
    # (z = sqrt(1 - r^2) near the rim: the four roundings of 1 - r^2, each up to 2^-24, reach z divided by 2 z)
    dir_b = EPS * (OPS["dir"] + np.array([0.0, 0.0, 1.0]) * (2.0 / np.maximum(want[:, 2:3], 1e-300)))
    ok["the diffuse direction is the warp's"] = ~diffuse | (np.abs(local - want) <= C["dir"] * dir_b).all(-1)
    ratio["dir"] = np.where(diffuse, (np.abs(local - want) / dir_b).max(-1), 0.0)
    # the delta rows (level 3): bsdf_model.delta_core at u1 = s1, the direction through the frame
    dl = np.nonzero(active_next & is_delta)[0]
    ok["delta sample"] = np.ones(n_l, bool)
    if dl.size:
        rows_l = rows[mat[dl]].copy()
        rows_l[:, 1:4] = np.asarray(out["refl"], np.float32)[dl]
        idx = np.arange(dl.size)
        X = BM.pack(rows_l, idx, out["wi"][dl], local[dl].astype(np.float32), s[dl, 0])
        natd, ambd, candsd = BM.candidates(BM.delta_core, X, kind[dl], one_sided[dl])
        got = {"wo": local[dl], "pdf": pdf[dl], "weight": w[dl], "eta": eta[dl], "delta": has(F_DELTA)[dl].astype(np.float64)}
        ops = {"wo": BM.OPS["refract"], "pdf": BM.OPS["fresnel_d"], "weight": BM.OPS["fresnel_c"], "eta": 1, "delta": 0}

        def within(ans, lanes=slice(None)):
            good = np.ones(got["pdf"][lanes].shape[0], bool)
            for k in got:
                band = ans.band(k, ops[k], BM.BAND_C["delta"] if k != "delta" else 1.0) + (FRAME_OPS * EPS if k == "wo" else 0.0)
                near = np.abs(got[k][lanes] - ans.q[k]) <= band
                good &= near.all(-1) if near.ndim == 2 else near
            return good

        good = within(natd)
        for lanes, ans in candsd:
            good[lanes] |= within(ans, lanes)
        ok["delta sample"][dl] = good
        amb[dl] |= ambd
    delta = has(F_DELTA)
    ok["DELTA"] = delta == (active_next & is_delta & (pdf != 0.0)) if level >= 3 else ~delta

    # ---- the classes ----
    do_mis = active_next & ~delta & P.guided
    pick = u > P.frac
    ok["DO_MIS"] = has(F_DO_MIS) == do_mis
    ok["SMP_TREE"] = has(F_SMP_TREE) == (pick & do_mis)
    ok["BSDF_MIS"] = has(F_BSDF_MIS) == (do_mis & ~pick)
    ok["one class"] = ~(has(F_SMP_TREE) & has(F_BSDF_MIS)) & ((flags >> 11) == 0)
    bad = {k: np.nonzero(~v)[0] for k, v in ok.items() if not v.all()}
    return bad, {k: np.where(amb, 0.0, r) for k, r in ratio.items()}, amb


def draw_count(I, out):
    """how many PCG32 draws take rng_state to the returned state (0..8) -> (n,) int, -1 where none does"""
    st, inc = np.asarray(I["rng_state"], np.uint64), np.asarray(I["rng_inc"], np.uint64)
    got = np.full(st.shape[0], -1)
    for k in range(9):
        got = np.where((got < 0) & (st == np.asarray(out["rng_out"], np.uint64)), k, got)
        _, st = VM.pcg32_draw(st, inc)
    return got
