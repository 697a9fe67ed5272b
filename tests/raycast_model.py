"""A float64 model of ray casting, written from the geometry: no BVH, every ray meets every primitive.

It reads the scene's float32 tables (the values, taken as exact reals) and knows nothing of the walk, of the
oracle (oracle/pg_oracle_render.c) or of the device code (csrc/pg_render_dev.hpp) beyond WHICH formula each
shape is tested with -- the number of float32 operations of that formula is all the band below is made of.

Two answers per ray
-------------------
exact   nearest t > 0 over all primitives in float64 with inclusive borders, its shape number (quads,
        spheres, 6 faces per box as 2 axis + (outward normal negative), triangles) and, for a triangle,
        its barycentrics.
band    t_lo <= t_hi: whatever a float32 evaluation of the same formulas may report lies in [t_lo, t_hi].
        Every (ray, primitive) pair gets a forward bound on what the float32 inside tests (u, v, 1-u-v;
        the quads' edge parameters; the boxes' slab order; the spheres' discriminant) and t can be off by.
        A pair is SURE when all its inside margins exceed their bounds and t - E_t > 0, POSSIBLE when they
        exceed minus the bounds and t + E_t > 0.  A float32 evaluation accepts every sure pair and no pair
        that is not possible, and reports min t_hat over what it accepts, so

            min over possible (t - E_t)  =  t_lo  <=  reported t  <=  t_hi  =  min over sure (t + E_t)

        (a miss is t = +inf).  t_sure / t_poss are the nearest sure / possible hits' own t; a ray is
        AMBIGUOUS when they differ by more than their two E_t together (or only one of them exists):
        then float32 may legitimately see another surface than exact geometry does.  The exact hit lies
        between the two, so on a ray that is not ambiguous the reported t equals the exact one within the
        band.  `n_close` counts the possible pairs that reach into the band: above 1, WHICH primitive is
        reported is not determined (the runner-up is within the bound), only t is.

The bounds
----------
Standard forward rounding analysis (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3): every
float32 operation returns its exact result times (1 + delta), |delta| <= u = 2^-24; a value that went
through k of them carries a factor within 1 +- g(k), g(k) = k u / (1 - k u); a sum of such terms is off by
at most g(k) times the sum of the terms' ABSOLUTE values, which are computed here in float64.  (Underflow
is not modelled: scene-scale data keeps every product far above 2^-126 or makes it exactly 0.)  The
constants are operation counts of the longest path to the quantity; divisions are correctly rounded
(-fhip-fp32-correctly-rounded-divide-sqrt; IEEE on the CPU).

Triangles (Moeller-Trumbore; p = d x e2, det = e1.p, s = o - v0, q = s x e1, u = s.p / det, v = d.q / det,
t = e2.q / det, with x / det done as x * (1 / det)):
  p_i    2 products, 1 difference: both terms went through 2 ops          -> g(2) * (|a b| + |c d|)
  det    3-term dot of (exact e1, p): product + 2 sums on top of p's 2    -> K_DET = 5
  s_i    1 difference                                                     -> 1
  s.p    s (1) + p (2) + dot (3)                                          -> K_SP  = 6
  q_i    s (1) + product, difference (2)                                  -> 3
  d.q    q (3) + dot (3)                                                  -> K_DQ  = 6   (e2.q the same)
  x/det  reciprocal + product                                             -> K_DIV = 2
  so  E_det = g(5) sum|e1_i| P_i,  E_u = (g(6) sum|s_i| P_i + |u| E_det) / (|det| - E_det) + g(2) (|u| + that),
  likewise E_v, E_t with Q_i in place of P_i; u + v is one more operation: E_w = (E_u + E_v)(1 + u) + u (|u| + |v|).
  |det| <= E_det: nothing is known of that pair (every bound infinite) -- unless |s.p| - E or |d.q| - E exceeds |det| + E_det:
  then |u_hat| or |v_hat| > 1 and the pair is refused.  det and all its terms exactly 0: refused by everyone.
Quads (t = n.(q0 - o) / n.d, w = (o + d t) - q0, a = (w.e1) inv1, b = (w.e2) inv2):
  n.d    product + 2 sums                                                 -> K_ND = 3
  n.(q0 - o)   difference + product + 2 sums                              -> K_NQ = 4
  t      one division                                                     -> + u |t|
  w_i    product, sum, difference on top of t's error: |d_i| E_t + g(3) (|d_i t| + |o_i| + |q0_i|)
  a      3-term dot (3) + the product with inv1 (1) on top of w           -> K_WE = 4
Spheres (the quadratic in float64, the root rounded to float32 once): the float64 operations carry
  u64 = 2^-53 in place of u: E_disc = g64(8) (B^2 + |4 A C|), a root is off by the square root's share
  min(E_disc / sqrt(disc), sqrt(E_disc)) / A plus g64(8) of its terms, and by u |t| for the rounding to
  float32.  The two roots are two candidates (the near one, else the far one, whichever is > 0).
Boxes (ol = R (o - c), dl = R d, slab planes at -1 and 1, t = (+-1 - ol_k) (1 / dl_k)):
  ol_k   difference + 3-term dot                                          -> K_OL = 4
  dl_k   3-term dot                                                       -> K_DL = 3
  t      difference, reciprocal, product                                  -> K_SLAB = 3
  The entry is the greatest near plane, the exit the least far plane; max and min move by no more than
  their arguments do, so E_in / E_out are the greatest bound among the three.  Entry and exit are two
  candidates, both tied to exit - entry exceeding (sure) or not undershooting (possible) E_in + E_out.
  A direction whose local component is not exactly 0 but within its bound of 0: nothing is known.
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def g(k, u=U32):
    return k * u / (1.0 - k * u)


K_DET, K_SP, K_DQ, K_DIV = 5, 6, 6, 2
K_ND, K_NQ, K_WE = 3, 4, 4
K_OL, K_DL, K_SLAB = 4, 3, 3
K_SPHERE = 8
INF = np.inf


class Tables:
    """The float32 tables of a scene object as float64 arrays, and the shape numbering."""

    def __init__(self, scene):
        f = lambda a, w: np.asarray(a, np.float32).reshape(-1, w).astype(np.float64)
        self.quads = f(scene.quads, 24)
        self.spheres = f(getattr(scene, "spheres", np.zeros((0, 12))), 12)
        self.boxes = f(getattr(scene, "boxes", np.zeros((0, 32))), 32)
        self.tris = f(getattr(scene, "tris", np.zeros((0, 16))), 16)
        self.bvh = np.asarray(getattr(scene, "bvh", np.zeros((0, 32))), np.uint32).reshape(-1, 32)
        self.first_sphere = self.quads.shape[0]
        self.first_box = self.first_sphere + self.spheres.shape[0]
        self.first_tri = self.first_box + 6 * self.boxes.shape[0]
        self.bbox = (np.asarray(scene.bbox_min, np.float64), np.asarray(scene.bbox_max, np.float64))


def _dot_abs(a, b):
    return np.abs(a[..., 0] * b[..., 0]) + np.abs(a[..., 1] * b[..., 1]) + np.abs(a[..., 2] * b[..., 2])


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _cross_abs(a, b):
    return np.stack([np.abs(a[..., 1] * b[..., 2]) + np.abs(a[..., 2] * b[..., 1]), np.abs(a[..., 2] * b[..., 0]) + np.abs(a[..., 0] * b[..., 2]),
                     np.abs(a[..., 0] * b[..., 1]) + np.abs(a[..., 1] * b[..., 0])], -1)


def _quot_err(num, e_num, den, e_den, k_after):
    """bound on |fl(num_hat / den_hat) - num / den| given the bounds of numerator and denominator and k_after more ops"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = np.abs(num / den)
        room = np.abs(den) - e_den
        e = (e_num + x * e_den) / room
        e = e + g(k_after) * (x + e)
        return np.where(room > 0.0, e, INF)


def _tri_block(T, o, d):
    v0, e1, e2 = T.tris[None, :, 0:3], T.tris[None, :, 3:6], T.tris[None, :, 6:9]
    o, d = o[:, None, :], d[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p, P = _cross(d, e2), _cross_abs(d, e2)
        det, e_det = _dot(e1, p), g(K_DET) * _dot_abs(e1, P)
        s = o - v0
        q, Q = _cross(s, e1), _cross_abs(s, e1)
        nu, nv, nt = _dot(s, p), _dot(d, q), _dot(e2, q)
        u, v, t = nu / det, nv / det, nt / det
        e_nu, e_nv = g(K_SP) * _dot_abs(s, P), g(K_DQ) * _dot_abs(d, Q)
        e_u = _quot_err(nu, e_nu, det, e_det, K_DIV)
        e_v = _quot_err(nv, e_nv, det, e_det, K_DIV)
        e_t = _quot_err(nt, g(K_DQ) * _dot_abs(e2, Q), det, e_det, K_DIV)
        e_w = (e_u + e_v) * (1.0 + U32) + U32 * (np.abs(u) + np.abs(v))
        w = u + v
        known = np.isfinite(e_u) & np.isfinite(e_v) & np.isfinite(e_t) & (det != 0.0)
        sure = np.minimum.reduce([u - e_u, (1.0 - u) - e_u, v - e_v, (1.0 - w) - e_w, t - e_t])
        poss = np.minimum.reduce([u + e_u, (1.0 - u) + e_u, v + e_v, (1.0 - w) + e_w, t + e_t])
        exact = (det != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (w <= 1.0) & (t > 0.0)
        zero = (det == 0.0) & (e_det == 0.0)  # every term is exactly 0 in float32 too: skipped by both
        sure = np.where(known, sure, -INF)
        # |det| within its bound of 0: the quotients' bounds are infinite, but |u_hat| >= (|s.p| - E) / (|det| + E_det) still
        # holds, and a u_hat or v_hat beyond 1 in magnitude is refused whatever its sign (v > 1 with u >= 0 fails u + v <= 1)
        ceil_ = (np.abs(det) + e_det) * (1.0 + g(K_DIV + 1))
        refused = ((np.abs(nu) - e_nu) > ceil_) | ((np.abs(nv) - e_nv) > ceil_)
        poss = np.where(known, poss, np.where(zero | refused, -INF, INF))  # nothing known: anything is possible ...
        t_p = np.where(known, t, 0.0)                            # ... at any distance
        e_tp = np.where(known, e_t, 0.0)
        return dict(t=np.where(det != 0.0, t, INF), exact=exact, sure=sure > 0.0, poss=poss >= 0.0, t_lo=t_p - e_tp, t_hi=t + e_t,
                    e_t=e_tp, u=u, v=v, e_u=e_u, e_v=e_v)


def _quad_block(T, o, d):
    Q = T.quads[None]
    q0, e1, e2, n, inv1, inv2 = Q[..., 0:3], Q[..., 3:6], Q[..., 6:9], Q[..., 9:12], Q[..., 12], Q[..., 13]
    o, d = o[:, None, :], d[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den, e_den = _dot(n, d), g(K_ND) * _dot_abs(n, d)
        num, e_num = _dot(n, q0 - o), g(K_NQ) * _dot_abs(n, q0 - o)
        t = num / den
        e_t = _quot_err(num, e_num, den, e_den, 1)
        w = (o + d * t[..., None]) - q0
        e_wi = np.abs(d) * e_t[..., None] + g(3) * (np.abs(d * t[..., None]) + np.abs(o) + np.abs(q0))
        a, b = _dot(w, e1) * inv1, _dot(w, e2) * inv2
        e_a = inv1 * (g(K_WE) * _dot_abs(w, e1) + (1.0 + g(K_WE)) * _dot_abs(e_wi, e1))
        e_b = inv2 * (g(K_WE) * _dot_abs(w, e2) + (1.0 + g(K_WE)) * _dot_abs(e_wi, e2))
        known = np.isfinite(e_t) & (den != 0.0)
        sure = np.minimum.reduce([a - e_a, (1.0 - a) - e_a, b - e_b, (1.0 - b) - e_b, t - e_t])
        poss = np.minimum.reduce([a + e_a, (1.0 - a) + e_a, b + e_b, (1.0 - b) + e_b, t + e_t])
        exact = (den != 0.0) & (a >= 0.0) & (a <= 1.0) & (b >= 0.0) & (b <= 1.0) & (t > 0.0)
        # den within its bound of 0: nothing known -- unless every term is exactly 0, which both skip
        unknown = ~known & ~((den == 0.0) & (e_den == 0.0))
        sure = np.where(known, sure, -INF)
        poss = np.where(known, poss, np.where(unknown, INF, -INF))
        z = np.zeros_like(t)
        return dict(t=np.where(den != 0.0, t, INF), exact=exact, sure=sure > 0.0, poss=poss >= 0.0, t_lo=np.where(known, t - e_t, 0.0),
                    t_hi=t + e_t, e_t=np.where(known, e_t, 0.0), u=z, v=z, e_u=z, e_v=z)


def _sphere_block(T, o, d):
    S = T.spheres[None]
    oc = o[:, None, :] - S[..., 0:3]
    dd = np.broadcast_to(d[:, None, :], oc.shape)
    r = S[..., 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        A, B, C = _dot(dd, dd), 2.0 * _dot(oc, dd), _dot(oc, oc) - r * r
        disc = B * B - 4.0 * A * C
        c_abs = _dot(oc, oc) + r * r  # the absolute values of C's terms
        e_disc = g(K_SPHERE, U64) * (B * B + 4.0 * A * c_abs)
        root = np.sqrt(np.maximum(disc, 0.0))
        e_root = np.minimum(e_disc / np.maximum(root, 1e-300), np.sqrt(e_disc))
        tm = -0.5 * (B + np.where(B < 0.0, -root, root))
        x0, x1 = tm / A, np.where(tm != 0.0, C / tm, tm / A)
        lo, hi = np.minimum(x0, x1), np.maximum(x0, x1)
        out = []
        for x in (lo, hi):
            e_x = U32 * np.abs(x) + e_root / A + g(K_SPHERE, U64) * (np.abs(B) + root) / A + g(K_SPHERE, U64) * c_abs / np.maximum(np.abs(tm), 1e-300) * (tm != 0.0)
            ok = (A != 0.0)
            sure = ok & (disc - e_disc > 0.0) & (x - e_x > 0.0)
            poss = ok & (disc + e_disc >= 0.0) & (x + e_x > 0.0)
            exact = ok & (disc >= 0.0) & (x > 0.0)
            z = np.zeros_like(x)
            out.append(dict(t=np.where(ok & (disc >= 0.0), x, INF), exact=exact, sure=sure, poss=poss, t_lo=x - e_x, t_hi=x + e_x, e_t=e_x, u=z, v=z, e_u=z, e_v=z))
    return out


def _box_block(T, o, d):
    """-> (entry candidate, exit candidate, face numbers of both, face_sure of both)"""
    Bx = T.boxes[None]
    R = Bx[..., 0:9].reshape(1, -1, 3, 3)
    oc = o[:, None, :] - Bx[..., 9:12]
    dd = np.broadcast_to(d[:, None, :], oc.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ol = np.einsum("nbki,nbi->nbk", np.broadcast_to(R, oc.shape[:2] + (3, 3)), oc)
        e_ol = g(K_OL) * np.einsum("nbki,nbi->nbk", np.abs(np.broadcast_to(R, oc.shape[:2] + (3, 3))), np.abs(oc))
        dl = np.einsum("nbki,nbi->nbk", np.broadcast_to(R, oc.shape[:2] + (3, 3)), dd)
        e_dl = g(K_DL) * np.einsum("nbki,nbi->nbk", np.abs(np.broadcast_to(R, oc.shape[:2] + (3, 3))), np.abs(dd))
        par = dl == 0.0
        murky = (np.abs(dl) <= e_dl) & (e_dl > 0.0)  # the float32 value may be 0 or of either sign: nothing known
        t1, t2 = (-1.0 - ol) / dl, (1.0 - ol) / dl
        e1_ = _quot_err(-1.0 - ol, e_ol + U32 * np.abs(-1.0 - ol), dl, e_dl, K_SLAB - 1)
        e2_ = _quot_err(1.0 - ol, e_ol + U32 * np.abs(1.0 - ol), dl, e_dl, K_SLAB - 1)
        lo, hi = np.where(dl > 0.0, t1, t2), np.where(dl > 0.0, t2, t1)
        e_lo, e_hi = np.where(dl > 0.0, e1_, e2_), np.where(dl > 0.0, e2_, e1_)
        lo, hi = np.where(par, -INF, lo), np.where(par, INF, hi)
        e_lo, e_hi = np.where(par, 0.0, e_lo), np.where(par, 0.0, e_hi)
        # a parallel slab: inside it or never
        in_m = np.minimum(ol + 1.0, 1.0 - ol)
        par_exact_out = (par & (in_m < 0.0)).any(-1)
        par_sure_in = np.where(par, in_m - e_ol > 0.0, True).all(-1)
        par_poss_in = np.where(par, in_m + e_ol >= 0.0, True).all(-1)
        tn, tf = lo.max(-1), hi.min(-1)
        an, af = lo.argmax(-1), hi.argmin(-1)
        e_in, e_out = e_lo.max(-1), e_hi.max(-1)
        unknown = murky.any(-1) | ~np.isfinite(e_in) | ~np.isfinite(e_out)
        gap = tf - tn
        hit_exact = ~par_exact_out & (tn <= tf)
        hit_sure = ~unknown & par_sure_in & (gap - (e_in + e_out) > 0.0)
        hit_poss = unknown | (par_poss_in & (gap + (e_in + e_out) >= 0.0))
        # which face: decided when the runner-up plane is farther off than the two bounds
        lo_s, hi_s = np.sort(lo, -1), np.sort(hi, -1)
        face_in_sure = ~unknown & ((lo_s[..., 2] - lo_s[..., 1]) > 2.0 * e_in)
        face_out_sure = ~unknown & ((hi_s[..., 1] - hi_s[..., 0]) > 2.0 * e_out)
        dan, daf = np.take_along_axis(dl, an[..., None], -1)[..., 0], np.take_along_axis(dl, af[..., None], -1)[..., 0]
        nb = np.arange(T.boxes.shape[0])[None, :]
        face_in = T.first_box + 6 * nb + 2 * an + (dan > 0.0)
        face_out = T.first_box + 6 * nb + 2 * af + (daf < 0.0)
        z = np.zeros_like(tn)
        e_in_k, e_out_k = np.where(unknown, 0.0, e_in), np.where(unknown, 0.0, e_out)
        ent = dict(t=np.where(hit_exact, tn, INF), exact=hit_exact & (tn > 0.0), sure=hit_sure & (tn - e_in > 0.0),
                   poss=hit_poss & (unknown | (tn + e_in > 0.0)), t_lo=np.where(unknown, 0.0, tn - e_in), t_hi=tn + e_in, e_t=e_in_k, u=z, v=z, e_u=z, e_v=z)
        ext = dict(t=np.where(hit_exact, tf, INF), exact=hit_exact & (tf > 0.0), sure=hit_sure & (tf - e_out > 0.0),
                   poss=hit_poss & (unknown | (tf + e_out > 0.0)), t_lo=np.where(unknown, 0.0, tf - e_out), t_hi=tf + e_out, e_t=e_out_k, u=z, v=z, e_u=z, e_v=z)
    return ent, ext, face_in, face_out, face_in_sure, face_out_sure


class Result:
    """Per ray: t, prim, u, v (exact; prim -1 and t inf: a miss), e_u, e_v, prim_decided (False: a box face on an edge -- compare
    prim // 6 only), t_lo, t_hi (the band), t_sure, t_poss, ambiguous, n_close, r (the exact hit's relative t bound, 0 on a miss)."""


def cast(T, o, d, block=None):
    o, d = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
    n = o.shape[0]
    m = max(1, T.tris.shape[0])
    block = block or max(1, min(n, 3_000_000 // m))
    keys = ("t", "prim", "u", "v", "e_u", "e_v", "prim_decided", "t_lo", "t_hi", "t_sure", "t_poss", "ambiguous", "n_close", "r", "e_t")
    acc = {k: [] for k in keys}
    for b0 in range(0, n, block):
        ob, db = o[b0:b0 + block], d[b0:b0 + block]
        cols, prims, decided = [], [], []
        k = ob.shape[0]
        if T.quads.shape[0]:
            cols.append(_quad_block(T, ob, db)); prims.append(np.broadcast_to(np.arange(T.quads.shape[0])[None], (k, T.quads.shape[0]))); decided.append(np.ones((k, T.quads.shape[0]), bool))
        if T.spheres.shape[0]:
            for c in _sphere_block(T, ob, db):
                cols.append(c); prims.append(np.broadcast_to(T.first_sphere + np.arange(T.spheres.shape[0])[None], (k, T.spheres.shape[0]))); decided.append(np.ones((k, T.spheres.shape[0]), bool))
        if T.boxes.shape[0]:
            ent, ext, f_in, f_out, s_in, s_out = _box_block(T, ob, db)
            cols += [ent, ext]; prims += [f_in, f_out]; decided += [s_in, s_out]
        if T.tris.shape[0]:
            cols.append(_tri_block(T, ob, db)); prims.append(np.broadcast_to(T.first_tri + np.arange(T.tris.shape[0])[None], (k, T.tris.shape[0]))); decided.append(np.ones((k, T.tris.shape[0]), bool))
        C = {key: np.concatenate([c[key] for c in cols], 1) for key in cols[0]}
        P, D = np.concatenate(prims, 1), np.concatenate(decided, 1)
        rows = np.arange(k)
        te = np.where(C["exact"], C["t"], INF)
        j = te.argmin(1)
        hit = np.isfinite(te[rows, j])
        acc["t"].append(te[rows, j])
        acc["prim"].append(np.where(hit, P[rows, j], -1))
        for key in ("u", "v", "e_u", "e_v"):
            acc[key].append(np.where(hit, C[key][rows, j], 0.0))
        acc["prim_decided"].append(D[rows, j] | ~hit)
        acc["e_t"].append(np.where(hit, C["e_t"][rows, j], 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            acc["r"].append(np.where(hit, C["e_t"][rows, j] / te[rows, j], 0.0))
        ts = np.where(C["sure"], C["t"], INF)
        js = ts.argmin(1)
        tp = np.where(C["poss"], np.where(np.isfinite(C["t"]), C["t"], 0.0), INF)
        jp = np.where(C["poss"], C["t_lo"], INF).argmin(1)
        t_hi = np.where(C["sure"], C["t_hi"], INF).min(1)
        t_lo = np.where(C["poss"], C["t_lo"], INF).min(1)
        t_sure, t_poss = ts[rows, js], tp[rows, jp]
        es = np.where(np.isfinite(t_sure), C["e_t"][rows, js], 0.0)
        ep = np.where(np.isfinite(t_poss), C["e_t"][rows, jp], 0.0)
        with np.errstate(invalid="ignore"):
            amb = np.where(np.isfinite(t_sure) & np.isfinite(t_poss), np.abs(t_sure - t_poss) > es + ep, np.isfinite(t_sure) != np.isfinite(t_poss))
        acc["t_lo"].append(t_lo); acc["t_hi"].append(t_hi); acc["t_sure"].append(t_sure); acc["t_poss"].append(t_poss)
        acc["ambiguous"].append(amb)
        acc["n_close"].append((C["poss"] & (C["t_lo"] <= t_hi[:, None])).sum(1))
    r = Result()
    for key in keys:
        setattr(r, key, np.concatenate(acc[key]))
    return r


# ---- seeded ray sets ----
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _f32(o, d):
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def rays_uniform(T, n, seed):
    """origins uniform in the bounding box, directions uniform on the sphere"""
    rng = np.random.default_rng(seed)
    lo, hi = T.bbox
    return _f32(lo + rng.random((n, 3)) * (hi - lo), _unit(rng.standard_normal((n, 3))))


def _tri_points(T, rng, n, bary):
    i = rng.integers(0, T.tris.shape[0], n)
    return i, T.tris[i, 0:3] + bary[:, :1] * T.tris[i, 3:6] + bary[:, 1:2] * T.tris[i, 6:9]


def _aimed(T, rng, target):
    lo, hi = T.bbox
    o = lo + rng.random(target.shape) * (hi - lo)
    return _f32(o, _unit(target - o))


def rays_interior(T, n, seed):
    """aimed at points well inside random triangles (barycentrics >= 0.1 each)"""
    rng = np.random.default_rng(seed)
    b = rng.dirichlet((1.0, 1.0, 1.0), n) * 0.7 + 0.1
    return _aimed(T, rng, _tri_points(T, rng, n, b[:, 1:3])[1])


def rays_edge(T, n, seed):
    """aimed at points of random triangles' edges"""
    rng = np.random.default_rng(seed)
    s, e = rng.random(n), rng.integers(0, 3, n)
    b = np.where((e == 0)[:, None], np.stack([s, 0 * s], 1), np.where((e == 1)[:, None], np.stack([0 * s, s], 1), np.stack([s, 1 - s], 1)))
    return _aimed(T, rng, _tri_points(T, rng, n, b)[1])


def rays_vertex(T, n, seed):
    """aimed at random triangles' vertices"""
    rng = np.random.default_rng(seed)
    b = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])[rng.integers(0, 3, n)]
    return _aimed(T, rng, _tri_points(T, rng, n, b)[1])


def _surface(T, n, seed, spawn):
    rng = np.random.default_rng(seed)
    bc = rng.dirichlet((1.0, 1.0, 1.0), n) * 0.7 + 0.1
    i, p = _tri_points(T, rng, n, bc[:, 1:3])
    nrm = _unit(np.cross(T.tris[i, 3:6], T.tris[i, 6:9]))
    tan = _unit(T.tris[i, 3:6])
    d = _unit(rng.standard_normal((n, 3)))
    graze = _unit(tan * np.cos(rng.random((n, 1)) * 6.283) + np.cross(nrm, tan) * 0.7 + nrm * (rng.random((n, 1)) - 0.5) * 2e-3)
    d = np.where((np.arange(n) % 4 == 0)[:, None], graze, d)
    p = p.astype(np.float32).astype(np.float64)
    if spawn:  # (1 + the greatest coordinate) * 1e-4 along the normal, to the side the ray leaves on
        p = p + nrm * np.sign(_dot(d, nrm))[:, None] * (1.0 + np.abs(p).max(1, keepdims=True)) * 1e-4
    return _f32(p, d)


def rays_surface(T, n, seed):
    """origins on random triangles as the renderer spawns a ray there -- the float32 point of the triangle, pushed off along the
    normal by the renderer's ray epsilon to the side the ray leaves on -- directions over both hemispheres, a quarter grazing"""
    return _surface(T, n, seed, True)


def rays_on_surface(T, n, seed):
    """the same origins WITHOUT the push: the origin's own triangle is met at t = 0 +- rounding, which float32 cannot tell from
    a hit (a seam case like the edges: no cap on the ambiguous share, no promise of no leaks)"""
    return _surface(T, n, seed, False)


def rays_axis(T, n, seed):
    """directions with one or two zero components, half of the zeros -0.0 (the reciprocals are +-inf)"""
    rng = np.random.default_rng(seed)
    o, d = rays_uniform(T, n, seed + 1)
    keep = rng.random((n, 3)) < 0.5
    keep[np.arange(n), rng.integers(0, 3, n)] = True            # at least one component stays
    keep[np.arange(n), (keep.argmax(1) + 1 + rng.integers(0, 2, n)) % 3] = False  # at least one goes
    d = np.where(keep, d, np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0))).astype(np.float32)
    d = d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return _f32(o, d)


def rays_box_planes(T, n, seed):
    """origins exactly on a plane of a BVH child box (from the node table), inside that box's face, with a zero direction
    component on that axis: (plane - o) * (1 / 0) = 0 * inf on that axis of that child's slab test"""
    rng = np.random.default_rng(seed)
    nodes = T.bvh
    planes = nodes[:, :24].view(np.float32).reshape(-1, 2, 3, 4)  # [node][lo/hi][axis][child]
    refs = nodes[:, 24:28]
    nd, ch = np.nonzero(refs != 0xffffffff)
    pick = rng.integers(0, nd.shape[0], n)
    nd, ch = nd[pick], ch[pick]
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    lo, hi = planes[nd, 0, :, ch].astype(np.float64), planes[nd, 1, :, ch].astype(np.float64)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    o[np.arange(n), axis] = planes[nd, side, axis, ch]
    d = _unit(rng.standard_normal((n, 3))).astype(np.float32)
    d[np.arange(n), axis] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
    d = d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return _f32(o, d)


MESH_SETS = {"uniform": rays_uniform, "interior": rays_interior, "edge": rays_edge, "vertex": rays_vertex, "surface": rays_surface,
             "on_surface": rays_on_surface, "axis": rays_axis, "box_planes": rays_box_planes}
CAPPED = ("uniform", "interior")           # at most AMBIGUOUS_CAP of these rays may be ambiguous (mesh scenes)
NO_LEAKS = ("uniform", "interior", "surface")
AMBIGUOUS_CAP = 0.02


# ---- what a float32 implementation's answer has to satisfy ----
def leaks(m, t):
    """rays whose reported t (inf: a miss) is more than the exact hit's own t bound away from the exact t, or that report a hit
    where exact geometry has none (a phantom) or none where it has one"""
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(t) & np.isfinite(m.t), np.abs(t - m.t) > m.e_t, np.isfinite(t) != np.isfinite(m.t))


def band_failures(T, m, t, prim, u, v):
    """-> {check: indices of the rays that fail it}; t, prim, u, v: an implementation's answers (prim < 0: a miss)"""
    prim = np.asarray(prim, np.int64)
    t = np.where(prim >= 0, np.asarray(t, np.float64), INF)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    clear = ~m.ambiguous
    both = clear & (prim >= 0) & (m.prim >= 0)
    is_box = (m.prim >= T.first_box) & (m.prim < T.first_tri)
    same = np.where(m.prim_decided | ~is_box, prim == m.prim, (prim - T.first_box) // 6 == (m.prim - T.first_box) // 6)
    tri = both & (prim == m.prim) & (m.prim >= T.first_tri)
    out = {"t outside the band": ~((t >= m.t_lo) & (t <= m.t_hi)),
           "hit / miss differs from exact on a ray that is not ambiguous": clear & ((prim >= 0) != (m.prim >= 0)),
           "another primitive than exact, no runner-up within the bound": both & (m.n_close <= 1) & ~same,
           "barycentrics outside their bound": tri & ((np.abs(u - m.u) > m.e_u) | (np.abs(v - m.v) > m.e_v)),
           "a leak on a ray that is not ambiguous": clear & leaks(m, t)}
    return {k: np.nonzero(x)[0] for k, x in out.items()}
