"""The bookkeeping of one path vertex in float64 numpy, written from the reference's lines
(path_guiding_integrator.py:16-24, 247-261, 302-311, 318-346, 352-378, 443-471) and not from either implementation: what
pgo_vertex_probe (oracle) and pg_vertex_probe (device) are held to.

Specification (f: the BSDF sampling fraction; flags as include/pgsd.h names them)
  emitter weight  em = em_w, and zero where the lane is occluded or its emitter sample is not live.
  emitter pdf     f bp_em + (1 - f) pdf_nee when guided, else bp_em; of a sample that is not live every factor is zero.
  MIS weight      mis_em = 1 for a live sample of a delta light (a directional light exists from level 3 on: below it the
                  flag is not honoured); else the power heuristic a^2 / (a^2 + b^2) of (ds_pdf, emitter pdf), 0 for a <= 0 or NaN.
  radiance        L' = L + Le + thr mis_em bv_em em   (Le where PG_VERTEX_HAS_LE, else 0).
  tree lanes      value and pdf of the BSDF are the model's (bsdf_model) at to_local(frame(n), wo), the frame Duff et al.'s.
  mixture         where DO_MIS: woPdf = f pdf + (1 - f) pdf_tree, weight = value / woPdf, and zero where woPdf is not positive
                  (the reference divides 0 / 0 there); elsewhere woPdf = bsdf_pdf and weight = bsdf_w, bit for bit.
  record          (record and VALID) weight, thr BEFORE it is multiplied (bit for bit), L' (after the add), woPdf, and
                  nee_lum = luminance(scrub(Lr_dir / thr)) where store_nee, else 0: the scrub takes NaN (0 / 0 of a dead channel)
                  to 0 and leaves an infinity; Rec.709 weights.  ray_of = the lane, or 0xffffffff where the lane is not valid;
                  nothing else is written for a lane that is not recorded.
  advance         ior' = ior eta at level 3 (no material below it has an index), thr' = thr weight, prev_pdf = woPdf (the
                  MIXTURE, :358), delta_out = the DELTA flag, ray_d = wo bit for bit.
  continuation    ACTIVE_NEXT and max(thr') != 0 and (depth < rr_depth or rr < min(max(thr') ior'^2, 0.95)), NaN -> 0.95, with
                  0.95 the float32 the reference's Float holds.  The throughput is NOT divided by the roulette's probability:
                  :376 scales the local maximum only.  A NaN in thr' leaves max() to the order of its comparisons: not judged.
  spawned ray     ray_o = p +- ng (1 + max |p_i|) kRayEps, the sign that of ng . wo, + at exactly 0.
  sampler         one draw of PCG32 (O'Neill's XSH-RR 64/32; a float as Mitsuba's next_float32: 23 bits under the exponent of 1,
                  minus 1), whatever the flags: the state afterwards is state * 6364136223846793005 + inc.

Bands.  Every quantity q carries surface_model.bracket's  2^-24 ops |q| + sum_j |dq/dx_j| ulp(x_j)  and passes within C times it
(plus a few units of the smallest subnormal: a product down there is rounded to it).  On a tree lane the BSDF's value and pdf
enter as inputs whose step is bsdf_model's own committed band, taken at the model's local direction and widened by the change
of the BSDF under 16 roundings (surface_model's count for a frame and a dot product) of each component of that direction.
ops, the float32 roundings on the quantity's own path:
  L'        14   the mixture (1 - f, two products, diffuse factor, sum: 5), the heuristic (two squares, sum, quotient: 4), three
                 products, two sums;  |q| := |L| + |Le| + |Lr_dir|
  woPdf      4   1 - f, two products, a sum
  weight     6   value = weight pdf (1), woPdf (4), the quotient
  thr'       7   ... and the product
  nee_lum   18   Lr_dir (12), the quotient, the luminance (5);  |q| := sum of the weighted channels' magnitudes
  ior'       1
  rr_prob   10   thr' (7), the square, the product (and max() is exact)
  ray_o      4   1 + max |p|, times kRayEps, times ng, the sum;  |q| := |p| + the offset
  ng . wo    5   a 3-term dot (its bracket: 2^-24 5 sum |ng_k wo_k|, the inputs being exact)

Decisions within float32's own reach are AMBIGUOUS, and the lane must equal the model under one assignment:
  rr against min(rr_prob, 0.95)   rr within the band of rr_prob where that decides (rr < 0.95 itself is a comparison of two
                                  float32 numbers, exact: so is rr_prob within its band of 0.95 unless rr is there too)
  ng . wo within its band of 0    either sign of the offset
  woPdf or max(thr') below 2^-120 a product that may have vanished: the path may end, the weight may be zero
  a doubtful decision of the BSDF model on a tree lane (bsdf_model.candidates): the vertex under every candidate
C per quantity (BAND_C) is four times the worst ratio measured on the CPU oracle over the suite's own sets
(profiles/vertex/band.txt, written by tools/vertex_mutants.py --band).
"""
import numpy as np

import bsdf_model as BM
import surface_model as SM

F_VALID, F_ACTIVE_NEXT, F_DS_DELTA, F_DELTA, F_DO_MIS, F_SMP_TREE, F_NEE_LIVE, F_HAS_LE = 1, 2, 16, 32, 64, 128, 512, 1024
INVALID_RAY = 0xFFFFFFFF
RAY_EPS = float(np.float32(1e-4))
C95 = float(np.float32(0.95))
LUMINANCE = tuple(float(np.float32(w)) for w in (0.212671, 0.715160, 0.072169))   # mi.luminance, Rec.709
EPS = SM.EPS
SUBNORMAL = 2.0 ** -149
VANISHING = 2.0 ** -120   # a product of float32 numbers below this may have lost bits to the subnormal range, or all of them
FRAME_OPS = 16
AMBIGUOUS_CAP = 0.02
OPS = {"L": 14, "wopdf": 4, "weight": 6, "thr": 7, "nee": 18, "ior": 1, "rr_prob": 10, "ray_o": 4, "side": 5}
# four times the worst |difference| / bracket measured on the oracle (profiles/vertex/band.txt); 64 would mean a missing term
BAND_C = {"L": 0.75, "wopdf": 1.36, "weight": 1.40, "thr": 1.28, "nee": 0.88, "ior": 0.56, "ray_o": 0.79}
DECISION_C = 64.0         # the reach of a decision: the C at which a bracket is taken to be missing a term


class Params:
    def __init__(self, frac, guided, record, store_nee, rr_depth):
        self.frac, self.guided, self.record, self.store_nee, self.rr_depth = float(np.float32(frac)), bool(guided), bool(record), bool(store_nee), int(rr_depth)

    def args(self):
        return self.frac, self.guided, self.record, self.store_nee, self.rr_depth


def pcg32_draw(state, inc):
    """one draw of PCG32 XSH-RR as a float in [0, 1) -> (float64 holding the float32, the state afterwards)"""
    old = np.asarray(state, np.uint64)
    with np.errstate(over="ignore"):
        new = old * np.uint64(6364136223846793005) + np.asarray(inc, np.uint64)
    xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
    rot = (old >> np.uint64(59)).astype(np.uint32)
    word = (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))
    f = ((word >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return f.astype(np.float64), new


def _dot(a, b):
    return (a * b).sum(-1)


def _power(a, b):
    with np.errstate(all="ignore"):
        r = np.where(a > 0.0, a * a / (a * a + b * b), 0.0)
    return np.where(np.isnan(r), 0.0, r)


def _f64(I, k):
    return np.asarray(I[k], np.float32).astype(np.float64)


class Bsdf:
    """value (n,3), pdf (n,) of the tree lanes' BSDF at the model's local direction and their steps (the committed band)"""

    def __init__(self, value, pdf, d_value, d_pdf):
        self.value, self.pdf, self.d_value, self.d_pdf = value, pdf, d_value, d_pdf

    def put(self, lanes, other):
        """a copy with other's answers on `lanes`"""
        r = Bsdf(self.value.copy(), self.pdf.copy(), self.d_value.copy(), self.d_pdf.copy())
        r.value[lanes], r.pdf[lanes], r.d_value[lanes], r.d_pdf[lanes] = other.value, other.pdf, other.d_value, other.d_pdf
        return r


@np.errstate(all="ignore")
def _bsdf_of(ans, X, kind, one_sided):
    """a bsdf_model Answer as a Bsdf: its committed band, widened by the frame's and the dot products' roundings of wo"""
    ops_v, ops_p = BM._ops(kind, "value"), BM._ops(kind, "pdf")
    dv = ans.band("value", ops_v, BM.BAND_C["value"])
    dp = ans.band("pdf", ops_p, BM.BAND_C["pdf"])
    h = EPS * FRAME_OPS
    for c in range(3):
        mv, mp = 0.0, 0.0
        for s in (h, -h):
            Y = X.copy()
            Y[:, 3 + c] += s
            q, _ = BM.eval_core(Y, kind, one_sided, ans.taken)
            with np.errstate(all="ignore"):
                mv = np.maximum(mv, np.nan_to_num(np.abs(q["value"] - ans.q["value"]), nan=np.inf))
                mp = np.maximum(mp, np.nan_to_num(np.abs(q["pdf"] - ans.q["pdf"]), nan=np.inf))
        dv, dp = dv + BM.BAND_C["value"] * mv, dp + BM.BAND_C["pdf"] * mp
    return Bsdf(ans.q["value"], ans.q["pdf"], dv, dp)


def tree_bsdf(rows, I, level):
    """-> (the natural Bsdf over all lanes -- zeros off the tree lanes --, doubtful (n,) bool, [(lanes, Bsdf)] the candidates)"""
    flags = np.asarray(I["flags"]).astype(np.int64)
    n = flags.shape[0]
    tree = np.nonzero(flags & F_SMP_TREE)[0]
    nat = Bsdf(np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3)), np.zeros(n))
    amb = np.zeros(n, bool)
    if not tree.size:
        return nat, amb, []
    nn = _f64(I, "n")[tree]
    s, t = SM.duff(nn)
    wo = _f64(I, "wo")[tree]
    local = np.stack([_dot(wo, s), _dot(wo, t), _dot(wo, nn)], -1)
    rows = np.asarray(rows, np.float32)
    idx = np.asarray(I["mat"], np.int64)[tree]
    kind, one_sided = BM.effective_rows(rows, idx, level)
    X = BM.pack(rows, idx, _f64(I, "wi")[tree], local.astype(np.float32))
    X[:, BM.WO] = local                      # (the model's direction, not its float32 rounding)
    X[:, BM.REFL] = _f64(I, "refl")[tree]    # the reflectance the surface left, not the row's
    a, doubtful, cands = BM.candidates(BM.eval_core, X, kind, one_sided)
    nat = nat.put(tree, _bsdf_of(a, X, kind, one_sided))
    amb[tree] = doubtful
    return nat, amb, [(tree[lanes], _bsdf_of(c, X[lanes], kind[lanes], one_sided[lanes])) for lanes, c in cands]


class Answer:
    """q[name], b[name] (the bracket, C = 1) per quantity; exact[name]: what must hold bit for bit; the decisions' doubts"""


@np.errstate(all="ignore")
def evaluate(I, P, level, bsdf, force_dead=None):
    """the model's answer on every lane.  force_dead (n,) bool: lanes whose woPdf is taken as not positive (a vanished product)"""
    flags = np.asarray(I["flags"]).astype(np.int64)
    n = flags.shape[0]
    has = lambda bit: (flags & bit) != 0
    valid, active_next, do_mis, tree, live = has(F_VALID), has(F_ACTIVE_NEXT), has(F_DO_MIS), has(F_SMP_TREE), has(F_NEE_LIVE)
    f = P.frac
    occluded = np.asarray(I["occluded"]) != 0
    delta_one = live & has(F_DS_DELTA) & (level >= 3)
    dead = np.zeros(n, bool) if force_dead is None else force_dead
    thr, L, ior, eta = _f64(I, "thr"), _f64(I, "L"), _f64(I, "ior"), _f64(I, "eta")
    Le = np.where(has(F_HAS_LE)[:, None], _f64(I, "Le"), 0.0)
    em = np.where((occluded | ~live)[:, None], 0.0, _f64(I, "em_w"))
    bv = np.where(live[:, None], _f64(I, "bv_em"), 0.0)
    bp_em, ds_pdf = np.where(live, _f64(I, "bp_em"), 0.0), np.where(live, _f64(I, "ds_pdf"), 0.0)
    pdf_nee, pdf_tree = _f64(I, "pdf_nee"), _f64(I, "pdf_tree")
    bsdf_w, bsdf_pdf = _f64(I, "bsdf_w"), _f64(I, "bsdf_pdf")
    p, ng, wo = _f64(I, "p"), _f64(I, "ng"), _f64(I, "wo")
    A = Answer()
    A.q, A.b, A.scale = {}, {}, {}

    @np.errstate(all="ignore")
    def lr(thr_, bv_, em_, ds_, bp_, nee_):
        mix = f * bp_ + (1.0 - f) * nee_ if P.guided else bp_
        mis = np.where(delta_one, 1.0, _power(ds_, mix))
        return thr_ * mis[:, None] * bv_ * em_

    @np.errstate(all="ignore")
    def new_L(L_, Le_, *rest):
        return L_ + (Le_ + lr(*rest))

    nee_in = (thr, bv, em, ds_pdf, bp_em, pdf_nee)
    with np.errstate(all="ignore"):
        scale_L = np.abs(L) + np.abs(Le) + np.abs(lr(*nee_in))
    A.q["L"], A.b["L"] = SM.bracket(new_L, (L, Le) + nee_in, OPS["L"], scale=scale_L, nan_is_inf=True)

    @np.errstate(all="ignore")
    def wopdf(w_, pdf_, tree_, tv_, tp_):
        pdf = np.where(tree, tp_, pdf_)
        return np.where(do_mis, f * pdf + (1.0 - f) * tree_, pdf_)

    @np.errstate(all="ignore")
    def weight(w_, pdf_, tree_, tv_, tp_):
        value = np.where(tree[:, None], tv_, w_ * pdf_[:, None])
        wp = wopdf(w_, pdf_, tree_, tv_, tp_)
        mixed = np.where(((wp > 0.0) & ~dead)[:, None], value / wp[:, None], 0.0)
        return np.where(do_mis[:, None], mixed, w_)

    w_in = (bsdf_w, bsdf_pdf, pdf_tree, bsdf.value, bsdf.pdf)
    w_steps = (None, None, None, bsdf.d_value, bsdf.d_pdf)
    A.q["wopdf"], A.b["wopdf"] = SM.bracket(wopdf, w_in, OPS["wopdf"], steps=w_steps, nan_is_inf=True)
    A.q["weight"], A.b["weight"] = SM.bracket(weight, w_in, OPS["weight"], steps=w_steps, nan_is_inf=True)

    @np.errstate(all="ignore")
    def new_thr(thr_, *w):
        return thr_ * weight(*w)

    A.q["thr"], A.b["thr"] = SM.bracket(new_thr, (thr,) + w_in, OPS["thr"], steps=(None,) + w_steps, nan_is_inf=True)

    @np.errstate(all="ignore")
    def channels(*a):
        rn = lr(*a) / a[0]
        return np.where(np.isnan(rn), 0.0, rn) * np.array(LUMINANCE)

    @np.errstate(all="ignore")
    def nee_lum(*a):
        return channels(*a).sum(-1) if P.store_nee else np.zeros(n)

    with np.errstate(all="ignore"):
        scale_nee = np.abs(channels(*nee_in)).sum(-1)
    A.q["nee"], A.b["nee"] = SM.bracket(nee_lum, nee_in, OPS["nee"], scale=scale_nee, nan_is_inf=True)

    @np.errstate(all="ignore")
    def new_ior(ior_, eta_):
        return ior_ * eta_ if level >= 3 else ior_

    A.q["ior"], A.b["ior"] = SM.bracket(new_ior, (ior, eta), OPS["ior"], nan_is_inf=True)

    @np.errstate(all="ignore")
    def rr_prob(ior_, eta_, *t):
        return new_thr(*t).max(-1) * new_ior(ior_, eta_) ** 2

    x, bx = SM.bracket(rr_prob, (ior, eta, thr) + w_in, OPS["rr_prob"], steps=(None, None, None) + w_steps, nan_is_inf=True)
    rr, A.rng_out = pcg32_draw(I["rng_state"], I["rng_inc"])
    with np.errstate(all="ignore"):
        tmax = A.q["thr"].max(-1)
        wins = np.where(np.isnan(x), rr < C95, (rr < x) & (rr < C95))
        rr_active = np.asarray(I["depth"]).astype(np.int64) >= P.rr_depth
        A.go = active_next & (tmax != 0.0) & (~rr_active | wins)
        A.go_undecided = np.isnan(A.q["thr"]).any(-1)
        A.doubt_rr = active_next & rr_active & (tmax != 0.0) & (rr < C95) & (np.abs(rr - x) <= DECISION_C * bx + SUBNORMAL)
        A.doubt_end = active_next & (tmax != 0.0) & (np.abs(tmax) < VANISHING)
        A.doubt_wopdf = do_mis & (A.q["wopdf"] > 0.0) & (A.q["wopdf"] < VANISHING)
        side = _dot(ng, wo)
        A.doubt_side = np.abs(side) <= DECISION_C * EPS * OPS["side"] * _dot(np.abs(ng), np.abs(wo))
        A.doubt_side &= ~((ng == 0.0) | (wo == 0.0)).all(-1)   # (an exact 0 of exact zeros is a 0 in float32 too)
        sign = np.where(side < 0.0, -1.0, 1.0)

        def origin(sgn):
            off = lambda p_, ng_: p_ + ng_ * ((1.0 + np.abs(p_).max(-1)) * RAY_EPS * sgn)[:, None]
            scale = np.abs(p) + np.abs(off(p, ng) - p)
            return SM.bracket(off, (p, ng), OPS["ray_o"], scale=scale, nan_is_inf=True)

        A.q["ray_o"], A.b["ray_o"] = origin(sign)
        A.other_side = origin(-sign)
    A.recorded = valid & P.record
    A.ray_of = np.where(valid, np.arange(n), INVALID_RAY)
    A.exact_weight, A.do_mis = ~do_mis, do_mis
    return A


def _ratio(got, q, b):
    """|difference| over the bracket (with its few subnormal units), the worst component; 0 where both hold the same
    non-number or infinity"""
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        same = (got == q) | (np.isnan(got) & np.isnan(q))
        r = np.where(same, 0.0, np.abs(got - q) / (b + 4 * SUBNORMAL))
    r = np.where(np.isnan(r), np.inf, r)
    return r.max(-1) if r.ndim == 2 else r


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return same.all(-1) if same.ndim == 2 else same


FLOATS = ("L", "wopdf", "weight", "thr", "nee", "ior", "ray_o")


def _check(A, I, P, level, out, C, fill):
    """-> ({check: (n,) bool ok}, {quantity: (n,) ratio}) of an implementation's outputs against one answer"""
    rec = A.recorded
    plane = lambda k: np.asarray(out[k]).T if np.asarray(out[k]).ndim == 2 else np.asarray(out[k])
    got = {"L": out["L"], "thr": out["thr"], "ior": out["ior"], "ray_o": out["ray_o"], "wopdf": out["prev_pdf"]}
    ratio = {k: _ratio(got[k], A.q[k], A.b[k]) for k in got}
    # the weight is seen in the record, and in thr' wherever it is not
    ratio["weight"] = np.where(rec, _ratio(plane("r_bsdf"), A.q["weight"], A.b["weight"]), 0.0)
    ratio["nee"] = np.where(rec, _ratio(plane("r_nee"), A.q["nee"], A.b["nee"]), 0.0)
    ok = {k: ratio[k] <= C[k] for k in ratio}
    ok["record L"] = ~rec | _bits(plane("r_tr"), out["L"])
    ok["record thr"] = ~rec | _bits(plane("r_tb"), I["thr"])
    ok["record woPdf"] = ~rec | _bits(plane("r_wp"), out["prev_pdf"])
    ok["ray_of"] = (np.asarray(out["ray_of"]).astype(np.int64) == A.ray_of) if P.record else (np.asarray(out["ray_of"]) == fill["ray_of"])
    for k in ("r_bsdf", "r_tb", "r_tr", "r_nee", "r_wp"):
        untouched = plane(k) == np.float32(fill[k])
        ok["unrecorded " + k] = rec | (untouched.all(-1) if untouched.ndim == 2 else untouched)
    ok["weight as given"] = ~(rec & A.exact_weight) | _bits(plane("r_bsdf"), I["bsdf_w"])
    ok["woPdf as given"] = A.do_mis | _bits(out["prev_pdf"], I["bsdf_pdf"])
    ok["ior as given"] = _bits(out["ior"], I["ior"]) if level < 3 else np.ones(rec.shape[0], bool)
    ok["ray_d"] = _bits(out["ray_d"], I["wo"])
    ok["delta"] = np.asarray(out["delta"]) == ((np.asarray(I["flags"]).astype(np.int64) & F_DELTA) != 0)
    ok["sampler"] = np.asarray(out["rng_out"], np.uint64) == A.rng_out
    ok["go"] = (np.asarray(out["go"]) == A.go) | A.go_undecided
    return ok, ratio


def judge(rows, I, P, level, out, C=None, fill=None):
    """an implementation's outputs (the columns of pg_vertex_out, the sampler's new state as "rng_out", record planes (3, n))
    against the model -> ({check: lanes that fail}, {quantity: (n,) ratio to the natural answer's bracket, 0 on ambiguous
    lanes}, ambiguous (n,) bool)"""
    C = C or BAND_C
    fill = fill or {"ray_of": 0xFFFFFFFE, "r_bsdf": -7.0, "r_tb": -7.0, "r_tr": -7.0, "r_nee": -7.0, "r_wp": -7.0}
    nat_bsdf, amb, cands = tree_bsdf(rows, I, level)
    A = evaluate(I, P, level, nat_bsdf)
    ok, ratio = _check(A, I, P, level, out, C, fill)
    n = amb.shape[0]
    amb = amb | A.doubt_rr | A.doubt_end | A.doubt_wopdf | A.doubt_side
    # the decisions that touch one output only: either outcome
    ok["go"] |= A.doubt_rr | A.doubt_end
    q, b = A.other_side
    ok["ray_o"] |= A.doubt_side & (_ratio(out["ray_o"], q, b) <= C["ray_o"])
    good = np.ones(n, bool)
    for v in ok.values():
        good &= v
    # the decisions that reach further: the whole lane under the other assignment
    alternatives = [(lanes, bs, None) for lanes, bs in cands]
    if A.doubt_wopdf.any():
        alternatives.append((np.nonzero(A.doubt_wopdf)[0], None, A.doubt_wopdf))
    for lanes, bs, dead in alternatives:
        B = evaluate(I, P, level, nat_bsdf if bs is None else nat_bsdf.put(lanes, bs), dead)
        ok_b, _ = _check(B, I, P, level, out, C, fill)
        ok_b["go"] |= B.doubt_rr | B.doubt_end | A.doubt_rr | A.doubt_end
        qb, bb = B.other_side
        ok_b["ray_o"] |= A.doubt_side & (_ratio(out["ray_o"], qb, bb) <= C["ray_o"])
        all_b = np.ones(n, bool)
        for v in ok_b.values():
            all_b &= v
        rescued = np.zeros(n, bool)
        rescued[lanes] = all_b[lanes] & ~good[lanes]
        for k in ok:
            ok[k] |= rescued
        good |= rescued
    bad = {k: np.nonzero(~v)[0] for k, v in ok.items() if not v.all()}
    return bad, {k: np.where(amb, 0.0, r) for k, r in ratio.items()}, amb
