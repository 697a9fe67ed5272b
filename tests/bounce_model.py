"""Model of include/pgsd_bounce.h: pg_bounce as the header defines it -- the COMPOSITION of the calls that exist, in its order.

Test infrastructure; the product never imports it.  It restates nothing: the fraction is fraction_model.FractionModel.query,
the pdfs and the PCG32 sample are the oracle's (OracleTree.pdf / sample, rng_next_f32), the warp is
warp_model.WarpModel.sample_warp, the estimate is radiance_model.RadianceModel.estimate.  What is the model's own is the
selection rule and the order of the steps.
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po
from radiance_model import RadianceModel
from warp_model import WarpModel

F = np.float32
NONE, PDF, SAMPLE, CHOOSE = 0, 1, 2, 3


def select(mode, xi, f):
    """sel of every lane: NONE -> 0, PDF -> 1, SAMPLE -> 2, CHOOSE -> xi > f ? 2 : 1 (xi == f and a NaN xi select 1); a mode
    byte > 3 is NONE."""
    mode = np.asarray(mode, np.uint8)
    mode = np.where(mode > CHOOSE, NONE, mode)
    with np.errstate(invalid="ignore"):
        chosen = np.where(np.asarray(xi, F) > np.asarray(f, F), SAMPLE, PDF)
    return np.where(mode == CHOOSE, chosen, mode).astype(np.uint8)


class BounceModel:
    """tree: the OracleTree that holds sdTree_prev.  fraction: a FractionModel of that tree (the learned fraction enabled) or
    None (f = f_const, the context's constant).  weights: the radiance table (uint64 per quadtree) or None."""

    def __init__(self, tree, fraction=None, f_const=0.5, weights=None, cols=None):
        self.tree = tree
        self.fraction = fraction
        self.f_const = F(f_const)
        self.warp = WarpModel(tree)
        self.rad = None if weights is None else RadianceModel(tree.export() if cols is None else cols, weights)

    def modes(self, n, mode):
        md = np.full(n, CHOOSE, np.uint8) if mode is None else np.asarray(mode, np.uint8)
        return np.where(md > CHOOSE, NONE, md).astype(np.uint8)

    def bounce(self, p, dir_nee, nee_active, dir_io, mode=None, u_select=None, state=None, inc=None, u=None):
        """{"select", "fraction", "pdf_nee", "pdf", "dir", "L_dir", "L_mean", "live"}; `state` advances in place (one draw per
        CHOOSE lane when u_select is None, then the draws of the lanes that sample); dir_io is not written: "dir" is its
        state behind the call.  L_dir / L_mean are None without a radiance table."""
        p = np.asarray(p, F)
        n = p.shape[1]
        nee = np.ones(n, bool) if nee_active is None else np.asarray(nee_active) != 0
        md = self.modes(n, mode)
        live = nee | (md != NONE)
        # 1. pg_fraction_query with the live lanes active
        if self.fraction is not None:
            f = self.fraction.query(p, live.astype(np.uint8))
        else:
            f = np.full(n, self.f_const, F)
        # 2. the selection
        if u_select is not None:
            xi = np.asarray(u_select, F)
        else:
            assert u is None and state is not None, "a drawn selection needs the PCG32 form"
            ch = md == CHOOSE
            st = np.ascontiguousarray(state[ch])
            xi = np.zeros(n, F)
            xi[ch] = po.rng_next_f32(st, np.ascontiguousarray(inc[ch]))
            state[ch] = st
        sel = select(md, xi, f)
        # 3. pg_guide_bounce(select = sel) / pg_guide_bounce_warp: the reference's three calls on one position
        pdf_nee = self.tree.pdf(p, dir_nee, nee.astype(np.uint8))
        pdf_wo = self.tree.pdf(p, dir_io, (sel == PDF).astype(np.uint8))
        samples = (sel == SAMPLE).astype(np.uint8)
        if u is not None:
            d_s, pdf_s = self.warp.sample_warp(p, u, samples)
        else:
            d_s, pdf_s = self.tree.sample(p, state, inc, samples)
        d = np.where(sel == SAMPLE, d_s, np.asarray(dir_io, F)).astype(F)
        pdf = np.where(sel == SAMPLE, pdf_s, np.where(sel == PDF, pdf_wo, F(1))).astype(F)
        # 4. pg_radiance_query on the direction as it stands now
        L_dir = L_mean = None
        if self.rad is not None:
            L_dir, L_mean = self.rad.estimate(p, d, (sel != NONE).astype(np.uint8))
        return {"select": sel, "fraction": f, "pdf_nee": pdf_nee, "pdf": pdf, "dir": d, "L_dir": L_dir, "L_mean": L_mean,
                "live": live}


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------
N = 50_001
TIES0 = 30_000              # first lane of the block of ties (three lanes per tie: f, its predecessor, its successor)
TIES = 300
OUT0 = 20_000               # first lane of the block of positions outside the root box
OUT = 128
THETA0 = F(np.log(0.3 / 0.7))   # the start value of a context enabled with fraction0 = 0.3: what lanes without a leaf get


def thetas(n_trees):
    """Per-leaf thetas spread over [-20, 20], both ends included."""
    if n_trees == 1:
        return np.array([0.75], F)
    t = np.linspace(-20.0, 20.0, n_trees).astype(F)
    t[0], t[-1] = F(-20), F(20)
    return t[(np.arange(n_trees) * 7919) % n_trees].astype(F) if n_trees > 2 else t


def fraction_state(n_trees):
    """A fractionLoadState / FractionModel.load_state dict with thetas(n_trees) and a distinct Adam state."""
    k = np.arange(n_trees)
    return {"theta": thetas(n_trees), "m": (F(0.01) * (k % 7)).astype(F), "v": (F(0.001) * (k % 5)).astype(F),
            "p1": np.full(n_trees, 0.9, F), "p2": np.full(n_trees, 0.999, F), "steps": np.ones(n_trees, np.uint32)}


def make_inputs(base):
    """base: test_gpu_radiance.make_inputs() (positions with the outside / face / split-plane / NaN lanes, directions with the
    non-finite head and the grid directions, a mask with holes, three uniforms).  Adds the NEE directions, the modes (all four
    values mixed, a few bytes > 3), u_select, and the warp's u."""
    import synth
    n = base["p"].shape[1]
    assert n == N
    r = synth.uniform(n, 25, 4)
    mode = np.where(r[0] < 0.1, NONE, np.where(r[0] < 0.25, PDF, np.where(r[0] < 0.4, SAMPLE, CHOOSE))).astype(np.uint8)
    mode[np.arange(7, n, 1013)] = np.array([4, 7, 255, 128], np.uint8)[np.arange(len(range(7, n, 1013))) % 4]
    mode[:16] = CHOOSE                          # the outside / NaN positions and the non-finite directions choose
    mode[TIES0:TIES0 + 3 * TIES] = CHOOSE
    p = np.array(base["p"], F)
    k = np.arange(OUT)
    p[k % 3, OUT0 + k] = np.where(k % 2 == 0, F(100) + F(0.001) * (k + 1), F(-0.5) * (k + 1)).astype(F)   # one axis outside
    p[2, OUT0:OUT0 + 8] = np.nan
    out = {"p": p, "dir_io": base["d"], "nee_active": base["active"], "dir_nee": synth.directions_uniform(n, 26),
           "mode": mode, "u_select": r[1].copy(), "u": np.ascontiguousarray(r[2:4])}
    out["u_select"][11] = np.nan
    for a in out.values():
        a.setflags(write=False)
    return out


def with_ties(u_select, f):
    """u_select with the block of ties: lane TIES0 + 3 k holds f of that lane, + 1 its fp32 predecessor, + 2 its successor
    (each lane's own f)."""
    u = np.array(u_select, F)
    k = np.arange(TIES0, TIES0 + 3 * TIES)
    ff = np.asarray(f, F)[k]
    u[k] = np.where(k % 3 == TIES0 % 3, ff, np.where(k % 3 == (TIES0 + 1) % 3, np.nextafter(ff, F(-1)), np.nextafter(ff, F(2))))
    return u


def check_conditions(which, inp, res, outside):
    """The conditions on the inputs (pgsd_bounce's issue): no branch of a test is empty.  res: BounceModel.bounce's dict."""
    md = np.where(inp["mode"] > CHOOSE, NONE, inp["mode"])
    ch = md == CHOOSE
    sel = res["select"]
    assert set(np.unique(md)) == {NONE, PDF, SAMPLE, CHOOSE} and (inp["mode"] > CHOOSE).sum() >= 4
    if which != "initial":
        assert (sel[ch] == PDF).mean() >= 0.2 and (sel[ch] == SAMPLE).mean() >= 0.2, ((sel[ch] == PDF).mean(), (sel[ch] == SAMPLE).mean())
    if res["L_dir"] is not None:
        on = sel != NONE
        assert (res["L_dir"][on] > 0).mean() >= 0.05, (res["L_dir"][on] > 0).mean()
    c = po.dir_to_canonical(np.asarray(inp["dir_io"], F)).astype(np.float64) * 128
    assert ((c == np.round(c)).all(axis=0)).sum() >= 1000
    assert outside.sum() >= 100
