"""The bookkeeping of a path vertex (pgo_vertex_probe: vertex_bookkeeping of oracle/pg_oracle_render.c, the function the render
pass calls at every vertex) against tests/vertex_model.py, a float64 statement of the reference's lines with derived float32
brackets: broad synthetic sets at every feature level and every (guided, record, store_nee), known answers on the edges, and
six chained bounces whose final radiance and whose records' incident radiance (process_records) are held to the model's sums.
tests/test_gpu_vertex.py holds the device to the oracle bit for bit on the same inputs, and to the model directly."""
import functools

import numpy as np
import pytest

import bsdf_model as BM
import bsdf_sets as BS
import vertex_model as VM
from oracle import pg_oracle as po

F32 = np.float32
LANES = 4099
FRACS = (0.0, 0.25, 0.5, 1.0)
RR_DEPTH = 5
SWITCHES = [(g, r, s) for g in (0, 1) for r in (0, 1) for s in (0, 1)]
V, AN, DD, DL, DM, ST, NL, HL = VM.F_VALID, VM.F_ACTIVE_NEXT, VM.F_DS_DELTA, VM.F_DELTA, VM.F_DO_MIS, VM.F_SMP_TREE, VM.F_NEE_LIVE, VM.F_HAS_LE
IGNORED = 4 | 8 | 256   # F_ACTIVE_EM, F_NEED_SHADOW, F_BSDF_MIS: stage_a's own, which the bookkeeping does not read
NAN = float("nan")
INF = float("inf")


def rows():
    return BS.table()[0]


def probe_oracle(I, P, level):
    return po.vertex_probe(rows(), I, level, *P.args())


def _unit(v):
    return v / np.sqrt((v * v).sum(-1))[:, None]


def _log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def draw(n, level, guided, seed):
    """n lanes of every consistent class: the classes as stage_a sets them (ACTIVE_NEXT needs VALID; NEE_LIVE, DELTA and DO_MIS
    need ACTIVE_NEXT; DO_MIS = ACTIVE_NEXT, not DELTA and guided; SMP_TREE needs DO_MIS; HAS_LE needs VALID; a row that is a
    smooth conductor or dielectric at this level samples a delta lobe), pdfs log-uniform over 1e-6 .. 1e6, and NaN in the
    fields an unset NEE_LIVE or HAS_LE gates on a third of those lanes"""
    rng = np.random.default_rng(seed)
    table = rows()
    mat = rng.integers(0, table.shape[0], n).astype(np.int32)
    kind, _ = BM.effective_rows(table, mat, level)
    coin = lambda p: rng.random(n) < p
    valid = coin(0.9)
    active_next = valid & coin(0.85)
    delta = active_next & (coin(0.15) | (kind == BM.CONDUCTOR) | (kind == BM.DIELECTRIC))
    do_mis = active_next & ~delta & bool(guided)
    tree = do_mis & coin(0.5)
    live = active_next & coin(0.6)
    has_le = valid & coin(0.3)
    flags = (valid * V | active_next * AN | coin(0.2) * DD | delta * DL | do_mis * DM | tree * ST | live * NL | has_le * HL
             | (do_mis & ~tree) * 256 | coin(0.5) * 4 | coin(0.5) * 8).astype(np.uint32)
    pdf = lambda: _log_uniform(rng, 1e-6, 1e6, n)
    I = {
        "thr": _log_uniform(rng, 1e-3, 10.0, (n, 3)), "L": rng.uniform(0, 10, (n, 3)), "ior": rng.choice([1.0, 1.5, 1 / 1.5, 2.419], n),
        "depth": rng.integers(0, 12, n).astype(np.uint32), "flags": flags, "Le": rng.uniform(0, 5, (n, 3)),
        "p": rng.uniform(-10, 10, (n, 3)), "n": _unit(rng.normal(size=(n, 3))), "wi": _unit(rng.normal(size=(n, 3))),
        "refl": rng.uniform(0, 1, (n, 3)), "mat": mat, "em_w": rng.uniform(0, 20, (n, 3)), "bv_em": rng.uniform(0, 2, (n, 3)),
        "bp_em": pdf(), "ds_pdf": pdf(), "bsdf_w": rng.uniform(0, 1.5, (n, 3)), "bsdf_pdf": pdf(),
        "eta": rng.choice([1.0, 1.5, 1 / 1.5], n), "wo": _unit(rng.normal(size=(n, 3))), "pdf_nee": pdf(), "pdf_tree": pdf(),
        "occluded": coin(0.25).astype(np.int32),
        "rng_state": rng.integers(0, 2 ** 63, n).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64),
        "rng_inc": rng.integers(0, 2 ** 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1),
    }
    I["ng"] = _unit(I["n"] + rng.normal(scale=0.2, size=(n, 3)))   # a smooth-shaded triangle: the geometric normal is another
    junk = coin(1 / 3)
    for k in ("em_w", "bv_em", "bp_em", "ds_pdf"):
        I[k] = np.where((~live & junk).reshape((n,) + (1,) * (I[k].ndim - 1)), NAN, I[k])
    I["Le"] = np.where((~has_le & junk)[:, None], NAN, I["Le"])
    return {k: np.ascontiguousarray(v, dict((a, b) for a, b, _ in po.VERTEX_LANES)[k]) for k, v in I.items()}


def subset(I, lanes):
    return {k: np.ascontiguousarray(v[lanes]) for k, v in I.items()}


@functools.lru_cache(maxsize=None)
def broad(level, switches):
    """the broad set of one (level, (guided, record, store_nee)): [(lanes' columns, Params)], a quarter of the 4099 lanes per f"""
    guided, record, store_nee = switches
    I = draw(LANES, level, guided, 1000 + 10 * level + 4 * guided + 2 * record + store_nee)
    return [(subset(I, np.arange(k, LANES, 4)), VM.Params(f, guided, record, store_nee, RR_DEPTH)) for k, f in enumerate(FRACS)]


def check_set(pieces, level, probe, what, C=None):
    """every piece of a set against the model -> (ambiguous lanes, lanes, {quantity: worst ratio})"""
    amb_n, n, worst = 0, 0, {}
    for I, P in pieces:
        bad, ratio, amb = VM.judge(rows(), I, P, level, probe(I, P, level), C)
        assert not bad, "%s, f = %g: %s" % (what, P.frac, {k: v[:6] for k, v in bad.items()})
        amb_n, n = amb_n + int(amb.sum()), n + amb.shape[0]
        for k, r in ratio.items():
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    return amb_n, n, worst


@pytest.mark.parametrize("switches", SWITCHES)
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_oracle_against_the_model(level, switches):
    amb, n, worst = check_set(broad(level, switches), level, probe_oracle, "level %d %s" % (level, switches))
    print("level %d, guided, record, store_nee = %s: %d lanes, %.3f %% ambiguous; worst ratios %s" % (
        level, switches, n, 100.0 * amb / n, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert amb <= VM.AMBIGUOUS_CAP * n
    assert max(worst.values()) < 64.0   # (a bracket that misses a term; BAND_C, four times the worst, is far below)


def test_the_broad_sets_hold_every_class():
    for level in range(4):
        flags = np.concatenate([I["flags"] for sw in SWITCHES for I, _ in broad(level, sw)]).astype(np.int64)
        classes = {int(c) for c in np.unique(flags & ~IGNORED)}
        for want in (0, V, V | HL, V | AN, V | AN | DL, V | AN | NL, V | AN | NL | DD, V | AN | DM, V | AN | DM | ST, V | AN | DM | ST | NL | HL,
                     V | AN | DL | NL | DD | HL):
            assert want in classes, (level, want)
        assert not ((flags & AN) != 0)[(flags & V) == 0].any() and not ((flags & ST) != 0)[(flags & DM) == 0].any()


# ---- known answers ---------------------------------------------------------------------------------------------------------
BASE = dict(thr=(0.5, 1, 2), L=(1, 2, 3), ior=1.0, depth=0, flags=V | AN | NL | DM, Le=(0, 0, 0), p=(1, 2, 3), n=(0, 0, 1), ng=(0, 0, 1),
            wi=(0, 0, 1), refl=(0.5, 0.5, 0.5), mat=0, em_w=(4, 4, 4), bv_em=(0.25, 0.25, 0.25), bp_em=1.0, ds_pdf=1.0,
            bsdf_w=(0.5, 0.5, 0.5), bsdf_pdf=0.25, eta=1.0, wo=(0, 0, 1), pdf_nee=1.0, pdf_tree=1.0, occluded=0,
            rng_state=0x853C49E6748FEA9B, rng_inc=0xDA3E39CB94B95BDB)
PLAIN = VM.Params(0.5, 1, 1, 1, RR_DEPTH)


def lanes_of(cases):
    """[{column: value} over BASE] -> the columns"""
    full = [dict(BASE, **c) for c in cases]
    return {k: np.ascontiguousarray(np.array([c[k] for c in full]), t).reshape((len(full), w) if w > 1 else (len(full),))
            for k, t, w in po.VERTEX_LANES}


def state_with(lo, hi):
    """a sampler state whose next draw lies in [lo, hi) -> (state, the draw as a float32)"""
    st = np.arange(1, 4097, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    rr, _ = VM.pcg32_draw(st, np.full(st.shape, BASE["rng_inc"], np.uint64))
    k = int(np.nonzero((rr >= lo) & (rr < hi))[0][0])
    return int(st[k]), F32(rr[k])


def lum(r, g, b):
    return F32(r) * F32(0.212671) + F32(g) * F32(0.715160) + F32(b) * F32(0.072169)


def run(cases, P=PLAIN, level=3, probe=probe_oracle, judged=True):
    I = lanes_of(cases)
    out = probe(I, P, level)
    if judged:   # (where the model has an answer at all: finite inputs)
        bad, _, _ = VM.judge(rows(), I, P, level, out)
        assert not bad, bad
    return I, out


def close(got, want):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=4 * 2.0 ** -24, atol=0)


def check_edges_of_the_mixture(probe=probe_oracle):
    cases = [dict(),                                               # 0 the plain lane
             dict(bsdf_pdf=0.0, pdf_tree=0.0),                     # 1 0 / 0: weight 0, the path ends
             dict(pdf_tree=INF),                                   # 2
             dict(flags=V | AN | NL, pdf_tree=7.0),                # 3 no mixture: the sample's own pdf and weight
             dict(flags=V | AN | NL | DM | ST, wo=(0, 0.6, 0.8), ng=(0, 0.6, 0.8), bsdf_pdf=123.0, bsdf_w=(9, 9, 9))]   # 4 a tree lane
    I, out = run(cases, probe=probe)
    close(out["L"][0], (1.25, 2.5, 4.0))                       # mix = 1, mis = 1 / 2, Lr = thr / 2
    close(out["prev_pdf"][0], 0.625)
    close(out["r_bsdf"][:, 0], [0.2] * 3)
    close(out["thr"][0], (0.1, 0.2, 0.4))
    close(out["r_nee"][0], lum(0.5, 0.5, 0.5))
    assert (out["r_tb"][:, 0] == I["thr"][0]).all() and (out["r_tr"][:, 0] == out["L"][0]).all() and out["r_wp"][0] == out["prev_pdf"][0]
    assert out["go"][0] == 1 and out["ray_of"][0] == 0
    assert out["prev_pdf"][1] == 0 and (out["r_bsdf"][:, 1] == 0).all() and (out["thr"][1] == 0).all() and out["go"][1] == 0
    assert out["prev_pdf"][2] == INF and (out["r_bsdf"][:, 2] == 0).all() and out["go"][2] == 0
    assert out["prev_pdf"][3] == F32(0.25) and (out["r_bsdf"][:, 3] == F32(0.5)).all()
    pdf = 0.8 / np.pi                                              # diffuse at cos = 0.8, refl 1 / 2, whatever the sample said
    close(out["prev_pdf"][4], 0.5 * pdf + 0.5)
    close(out["r_bsdf"][:, 4], [0.5 * pdf / (0.5 * pdf + 0.5)] * 3)
    # f = 1: (1 - f) inf is not a number, and neither is woPdf; not positive, so the weight is zero
    _, o1 = run([dict(pdf_tree=INF)], VM.Params(1.0, 1, 1, 1, RR_DEPTH), probe=probe, judged=False)
    assert np.isnan(o1["prev_pdf"][0]) and (o1["r_bsdf"][:, 0] == 0).all() and o1["go"][0] == 0
    # unguided: the emitter pdf is the BSDF's (mis = 1 / 2 with bp_em = 1 whatever pdf_nee is)
    _, o2 = run([dict(flags=V | AN | NL, pdf_nee=1e6)], VM.Params(0.5, 0, 1, 1, RR_DEPTH), probe=probe)
    close(o2["L"][0], (1.25, 2.5, 4.0))
    _, o3 = run([dict(flags=V | AN | NL | DM, pdf_nee=3.0, bp_em=1.0)], VM.Params(0.25, 1, 1, 1, RR_DEPTH), probe=probe)
    mis = 1.0 / (1.0 + (0.25 + 0.75 * 3.0) ** 2)                   # f multiplies the BSDF's pdf, 1 - f the tree's
    close(o3["L"][0], np.array([1, 2, 3]) + np.array([0.5, 1, 2]) * mis)
    close(o3["prev_pdf"][0], 0.25 * 0.25 + 0.75)


def test_edges_of_the_mixture():
    check_edges_of_the_mixture()


def check_edges_of_the_emitter_sample(probe=probe_oracle):
    cases = [dict(thr=(0, 1, 2)),                                  # 0 a dead channel: 0 / 0 in nee, scrubbed
             dict(thr=(0, 1, 2), em_w=(INF, 4, 4)),                # 1 ... with 0 inf = NaN in Lr_dir
             dict(thr=(NAN, 1, 2)),                                # 2
             dict(ds_pdf=0.0), dict(ds_pdf=INF), dict(bp_em=INF),  # 3 4 5: no weight
             dict(occluded=1),                                     # 6
             dict(flags=V | AN | DM, em_w=(NAN,) * 3, bv_em=(NAN,) * 3, bp_em=NAN, ds_pdf=NAN, Le=(NAN,) * 3),   # 7 garbage behind unset flags
             dict(flags=V | AN | DM | NL | HL, Le=(1, 1, 1)),       # 8
             dict(flags=V | AN | DM | NL | DD),                     # 9 a delta light, live
             dict(flags=V | AN | DM | DD, em_w=(NAN,) * 3),         # 10 ... not live
             dict(em_w=(INF, 4, 4))]                               # 11 an infinity is not scrubbed
    I, out = run(cases, probe=probe, judged=False)
    half = lum(0, 0.5, 0.5)
    for k in (0, 1, 2):
        close(out["r_nee"][k], half)
        close(out["L"][k][1:], (2.5, 4.0))
    assert out["L"][0][0] == 1 and np.isnan(out["L"][1][0]) and np.isnan(out["L"][2][0]) and np.isnan(out["r_tb"][0, 2])
    for k in (3, 4, 5, 6, 7, 10):
        assert (out["L"][k] == I["L"][k]).all() and out["r_nee"][k] == 0, k
    close(out["L"][8], (2.25, 3.5, 5.0))
    close(out["L"][9], (1.5, 3.0, 5.0))                           # mis = 1: Lr = thr
    close(out["r_nee"][9], lum(1, 1, 1))
    assert out["L"][11][0] == INF and out["r_nee"][11] == INF
    _, o2 = run([dict(flags=V | AN | DM | NL | DD)], level=2, probe=probe)   # no directional light below level 3: the heuristic
    close(o2["L"][0], (1.25, 2.5, 4.0))
    _, o3 = run([dict()], VM.Params(0.5, 1, 1, 0, RR_DEPTH), probe=probe)   # store_nee = 0
    assert o3["r_nee"][0] == 0 and o3["r_wp"][0] == o3["prev_pdf"][0]


def test_edges_of_the_emitter_sample():
    check_edges_of_the_emitter_sample()


def check_roulette_and_advance(probe=probe_oracle):
    st, rr = state_with(0.3, 0.7)
    plain = dict(flags=V | AN, bsdf_w=(1, 1, 1), rng_state=st, depth=RR_DEPTH)
    up, down = np.nextafter(rr, F32(1)), np.nextafter(rr, F32(0))
    st95, rr95 = state_with(float(F32(0.95)), 1.0)
    st_mid, _ = state_with(0.05, 0.08)
    cases = [dict(plain, thr=(rr, 0, 0)), dict(plain, thr=(0, up, 0)), dict(plain, thr=(0, 0, down)),   # 0 1 2: rr == rr_prob, either side
             dict(plain, thr=(1e-3,) * 3, depth=RR_DEPTH - 1), dict(plain, thr=(1e-3,) * 3),             # 3 4
             dict(plain, thr=(2, 2, 2)), dict(plain, thr=(2, 2, 2), rng_state=st95),                     # 5 6: rr_prob = 0.95
             dict(plain, thr=(0.01,) * 3, ior=2.0, eta=1.5, rng_state=st_mid),                           # 7 ior^2, and ior' not ior
             dict(flags=0, Le=(NAN,) * 3),                                                               # 8 an invalid lane
             dict(plain, p=(1e6, -3, 2)),                                                                # 9
             dict(plain, wo=(1, 0, 0)), dict(plain, wo=(0, 0.6, -0.8)),                                  # 10 11: ng . wo = 0, < 0
             dict(plain, flags=V | AN | DL, depth=0)]                                                    # 12
    I, out = run(cases, probe=probe)
    assert list(out["go"][:9]) == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert (out["thr"][5] == 2).all() and (out["thr"][1] == I["thr"][1]).all()      # not divided by the roulette's probability
    assert out["ior"][7] == 3 and out["ray_of"][8] == 0xFFFFFFFF and (out["L"][8] == I["L"][8]).all()
    assert (out["r_bsdf"][:, 8] == F32(po.VERTEX_RECORD_FILL["r_bsdf"])).all() and out["r_wp"][8] == F32(po.VERTEX_RECORD_FILL["r_wp"])
    mag = lambda m: (F32(1) + F32(m)) * F32(1e-4)
    assert (out["ray_o"][9] == np.array([1e6, -3, F32(2) + mag(1e6)], F32)).all()
    assert (out["ray_o"][10] == np.array([1, 2, F32(3) + mag(3)], F32)).all()
    assert (out["ray_o"][11] == np.array([1, 2, F32(3) - mag(3)], F32)).all()
    assert (out["ray_d"][11] == I["wo"][11]).all() and out["delta"][12] == 1 and out["delta"][0] == 0
    assert (out["prev_pdf"][:8] == F32(0.25)).all()
    _, o2 = run([cases[7]], level=2, probe=probe)                                     # level 2: ior stays, and 0.04 < rr
    assert o2["ior"][0] == 2 and o2["go"][0] == 0
    _, o3 = run(cases[:2] + [cases[8]], VM.Params(0.5, 1, 0, 1, RR_DEPTH), probe=probe)   # record = 0: nothing is written
    for k, fill in po.VERTEX_RECORD_FILL.items():
        assert (o3[k] == np.asarray(fill).astype(o3[k].dtype)).all(), k


def test_roulette_and_advance():
    check_roulette_and_advance()


def test_the_model_sampler_is_the_sampler_of_the_tree_queries():
    """the model's PCG32 and the one pgo_rng_next_f32 steps (pinned by the SD-tree's sampling tests) are two statements of one
    generator: the same floats and the same states over a few draws of 4096 streams"""
    st, inc = po.rng_seed(4096, 77)
    own = st.copy()
    for _ in range(4):
        f, own = VM.pcg32_draw(own, inc)
        assert (po.rng_next_f32(st, inc) == f.astype(F32)).all() and (own == st).all()


# ---- six chained bounces ---------------------------------------------------------------------------------------------------
BOUNCES, CHAIN_LANES = 6, 257


def chain(probe, level=3):
    """six bounces of one set of lanes, each call's outputs the next call's state -> per bounce (columns, outputs)"""
    P = VM.Params(0.5, 1, 1, 1, 3)
    steps, state = [], None
    for k in range(BOUNCES):
        I = draw(CHAIN_LANES, level, 1, 7000 + k)
        tree = (I["flags"] & ST) != 0
        I["flags"] = np.where(tree, I["flags"] & ~np.uint32(ST), I["flags"]).astype(np.uint32)   # (the BSDF has its own tests)
        for key in ("em_w", "bv_em", "bp_em", "ds_pdf", "Le"):
            I[key] = np.nan_to_num(I[key], nan=0.5).astype(F32)
        I["depth"][:] = k
        if state is None:
            I["thr"][:], I["L"][:], I["ior"][:] = 1, 0, 1
        else:
            prev_I, prev = state
            I["thr"], I["L"], I["ior"], I["rng_state"], I["rng_inc"] = prev["thr"], prev["L"], prev["ior"], prev["rng_out"], prev_I["rng_inc"]
            I["p"] = prev["ray_o"]
            I["flags"] = np.where(prev["go"] != 0, I["flags"], 0).astype(np.uint32)   # a path that ended: no lane any more
        out = probe(I, P, level)
        steps.append((I, out))
        state = (I, out)
    return P, steps


def check_chain(probe):
    level = 3
    P, steps = chain(probe, level)
    n = CHAIN_LANES
    thr, L, ior = np.ones((n, 3)), np.zeros((n, 3)), np.ones(n)
    mass = np.zeros((n, 3))
    thr_k, L_k, w_k = [], [], []
    none = VM.Bsdf(np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3)), np.zeros(n))
    for I, out in steps:
        # the model's own path state in float64, never rounded; the decisions are the implementation's (judged on the broad sets)
        A = VM.evaluate(I, P, level, none)
        f = lambda k: np.asarray(I[k], np.float64)
        Le = np.where(((I["flags"] & HL) != 0)[:, None], f("Le"), 0.0)
        # (evaluate() reads float32 columns: the emitter sample's share, linear in thr, is rescaled to the model's throughput)
        with np.errstate(all="ignore"):
            gain = np.where(f("thr") != 0, (A.q["L"] - f("L") - Le) / f("thr"), 0.0)
        L = L + (Le + thr * gain)
        mass += np.abs(Le) + np.abs(thr * gain)
        thr_k.append(thr.copy()), L_k.append(L.copy()), w_k.append(A.q["weight"].copy())
        thr = thr * A.q["weight"]
    final = steps[-1][1]["L"].astype(np.float64)
    # every term carries the 7 roundings per bounce of its throughput and the 14 of the add; four times that, as the bands
    tol = 4 * VM.EPS * (7 * BOUNCES + 14) * mass
    worst = float((np.abs(final - L) / np.maximum(tol, 1e-300)).max())
    print("final radiance over %d bounces: worst |difference| / tolerance %.3f" % (BOUNCES, worst))
    assert worst <= 1.0
    assert (mass.sum(-1) > 0).mean() > 0.5 and sum(int(o["go"].sum()) for _, o in steps[2:]) > n // 8   # paths that live
    # ---- the records through process_records: incident radiance (L_final - L_k) / (thr_k w_k) ----
    S = n * BOUNCES
    slot = lambda k: np.arange(n) * BOUNCES + k
    rec = {"active": np.zeros(S, np.uint8), "position": np.zeros((3, S), F32), "direction": np.zeros((2, S), F32),
           "bsdf": np.ones((3, S), F32), "throughputBsdf": np.ones((3, S), F32), "throughputRadiance": np.zeros((3, S), F32),
           "radiance_nee": np.ones((3, S), F32), "direction_nee": np.zeros((2, S), F32), "woPdf": np.ones(S, F32)}
    want = np.zeros(S)
    tol_r = np.zeros(S)
    lw = np.array(VM.LUMINANCE)
    for k, (I, out) in enumerate(steps):
        on = out["ray_of"] != 0xFFFFFFFF
        assert (out["ray_of"][on] == np.nonzero(on)[0]).all()
        g = slot(k)[on]
        rec["active"][g] = 1
        rec["bsdf"][:, g], rec["throughputBsdf"][:, g], rec["throughputRadiance"][:, g] = out["r_bsdf"][:, on], out["r_tb"][:, on], out["r_tr"][:, on]
        rec["position"][0, g] = g     # (the entry's own number, to find it again behind the compaction)
        with np.errstate(all="ignore"):
            o = (L - L_k[k]) / thr_k[k]
            o = np.where(np.isnan(o), 0.0, o)
            r = o / w_k[k]
            r = np.where(np.isnan(r), 0.0, r)
            # the difference of two sums of `mass` loses what the sums' roundings are; the two quotients two more roundings
            dr = (4 * VM.EPS * (7 * BOUNCES + 14) * 2 * mass / np.abs(thr_k[k] * w_k[k]) + 4 * VM.EPS * (7 + 6 + 2) * np.abs(r))
            dr = np.where(np.isfinite(dr), dr, 0.0)
        want[slot(k)] = (r * lw).sum(-1)
        tol_r[slot(k)] = (dr * lw).sum(-1) + 4 * VM.EPS * 5 * (np.abs(r) * lw).sum(-1)
    got = po.process_records(n, BOUNCES, np.ascontiguousarray(steps[-1][1]["L"].T), rec)
    where = got["position"][0].astype(np.int64)
    assert where.shape[0] == int(rec["active"].sum())          # every recorded vertex is kept (radiance_nee and woPdf are ones)
    ratio = np.abs(got["radiance"].astype(np.float64) - want[where]) / np.maximum(tol_r[where], 1e-300)
    ratio = np.where(got["radiance"] == want[where], 0.0, ratio)
    print("incident radiance of %d recorded vertices: worst |difference| / tolerance %.3f, %d of them non-zero" % (
        where.shape[0], float(ratio.max()), int((got["radiance"] != 0).sum())))
    assert ratio.max() <= 1.0 and (got["radiance"] != 0).sum() > where.shape[0] // 4


def test_six_chained_bounces():
    check_chain(probe_oracle)
