#!/usr/bin/env python3
"""What pg_nee_resample (include/ext/lights/pg_nee.h) costs beside the sequence a host issues today for the same method, one run,
one JSON line on stdout and a table in --out:

  fused     pg_nee_resample, M candidates, the common outputs (no candidate arrays);
  sequence  M times: pg_lights_sample on the lanes' streams (a KD descent and a selection of its own), then element-wise passes in
            torch that gather the light's record, draw the point (with the triangle's fold), form the direction, the two cosines,
            target, source and weight, draw zeta and update the reservoir.  After the M candidates one more pass forms W.  The
            host's passes use torch's own generator and functions: the sequence is timed, not compared;
  sample    pg_lights_sample alone, the same build: what one descent and one selection cost.

on workload.s1_balanced_tree() (SURVEY's S1) at --lanes uniform positions (default 2^22) and uniform normals, for L lights placed
uniformly in the box (parallelograms and triangles, one- and two-sided), the rows built from 2^22 synthetic records (the lights'
delta 0.1: the selection takes the tree branch on 90 % of the lanes).  Every library call is marshalled once and launched through
the C ABI; HIP events around whole calls; `--warmup` rounds, then `--launches` rounds in which every call of every M is timed one
after the other (interleaved, so a drift of the device's clocks meets them alike).  Medians with minimum and maximum.

No threshold is asserted here: the numbers are a finding.  Not measured: the call inside a renderer.

    python3 tools/nee_timing.py [--lanes N] [--lights 64,1024] [--launches 20] [--warmup 5] [--out profiles/nee/timing.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

MS = (1, 4, 8, 16)
DELTA = 0.1
RECORDS = 1 << 22


def light_table(torch, Wk, L):
    """L lights in the box as lightsSetGeometry's dict, and the records the host's passes gather: (L, 16) float32 on the device"""
    u = Wk.s_uniform(L, 21, 12)
    o = (u[0:3].T * 100.0).contiguous()
    a = ((u[3:6].T - 0.5) * 20.0).contiguous()
    b = ((u[6:9].T - 0.5) * 20.0).contiguous()
    rad, tri, two = 0.5 + 7.5 * u[9], u[10] < 0.5, u[11] < 0.5
    c = torch.linalg.cross(a, b)
    ln = c.norm(dim=1)
    inv_a = 1.0 / torch.where(tri, 0.5 * ln, ln)
    rec = torch.cat([o, a, b, c / ln[:, None], inv_a[:, None], rad[:, None], tri[:, None].float(), two[:, None].float()], dim=1)
    table = {"origin": o.numpy(), "edge_a": a.numpy(), "edge_b": b.numpy(), "radiance": rad.numpy(), "triangle": tri.numpy(),
             "two_sided": two.numpy()}
    return table, rec.contiguous().cuda()


def measure(torch, g, n, L, launches, warmup):
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    lib, h = g._lib, g._h
    P = Wk.s_positions_uniform(n, 3, device="cuda")
    Nrm = Wk.s_directions_uniform(n, 4, device="cuda").to(torch.float32).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")  # noqa: E731

    def ck(rc):
        N.check(h, rc)

    # ---- the lights: geometry, and rows built from synthetic records
    table, rec = light_table(torch, Wk, L)
    g.lightsSetGeometry(table)
    g.lightsEnable(L, delta=DELTA)
    ur = Wk.s_uniform(RECORDS, 9, 2, device="cuda")
    g.lightsRecord({"position": Wk.s_positions_uniform(RECORDS, 8, device="cuda"),
                    "light": (ur[0] * L).to(torch.int32).clamp_(max=L - 1).contiguous(), "value": (4.0 * ur[1]).contiguous()})
    g.lightsBuild()
    learned = g.lightsStatus()[1]
    del ur

    # ---- the fused call
    smp = PCG32Sampler(g, n, seed=7)
    out = {"light": i32(n), "point": f32(3, n), "weight": f32(n), "dir": f32(3, n), "dist": f32(n), "target": f32(n), "source": f32(n),
           "index": i32(n)}
    args = N.pg_nee_args(p=P.data_ptr(), normal=Nrm.data_ptr(), rng_state=smp.state.data_ptr(), rng_inc=smp.inc.data_ptr(),
                         **{k + "_out": v.data_ptr() for k, v in out.items()})
    prm = {M: N.pg_nee_params(M) for M in MS}

    def fused(M):
        ck(lib.pg_nee_resample(h, n, C.byref(prm[M]), C.byref(args), s))

    # ---- the sequence of today's calls
    smp_q = PCG32Sampler(g, n, seed=7)
    light, pmf = i32(n), f32(n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    res = {"wsum": f32(n), "kt": f32(n), "ks": f32(n), "ky": f32(3, n), "kj": i32(n), "kk": i32(n)}

    def lights_sample():
        ck(lib.pg_lights_sample(h, n, P.data_ptr(), None, smp_q.state.data_ptr(), smp_q.inc.data_ptr(), None, light.data_ptr(),
                                pmf.data_ptr(), s))

    def host_candidate(k):
        r = rec.index_select(0, light.long())                                  # (n, 16): the gather of the light's record
        e = torch.rand((2, n), device="cuda", generator=gen)
        fold = (r[:, 14] != 0) & (e[0] + e[1] > 1.0)
        e = torch.where(fold, 1.0 - e, e)
        y = (r[:, 0:3].T + e[0] * r[:, 3:6].T) + e[1] * r[:, 6:9].T
        v = y - P
        d2 = (v * v).sum(dim=0)
        w = v / torch.sqrt(d2)
        cs = (Nrm * w).sum(dim=0)
        cl = -(r[:, 9:12].T * w).sum(dim=0)
        cl = torch.where(r[:, 15] != 0, cl.abs(), cl)
        geo = torch.where((d2 > 0) & (cs > 0) & (cl > 0), cs * cl / d2, 0.0)
        tgt = r[:, 13] * geo
        src = pmf * r[:, 12]
        ratio = tgt / src
        wk = torch.where((src > 0) & (tgt > 0) & torch.isfinite(ratio), ratio, 0.0)
        zeta = torch.rand(n, device="cuda", generator=gen)
        res["wsum"] += wk
        keep = (wk > 0) & (zeta * res["wsum"] < wk)
        res["kk"].copy_(torch.where(keep, k, res["kk"]))
        res["kj"].copy_(torch.where(keep, light, res["kj"]))
        torch.where(keep, tgt, res["kt"], out=res["kt"])
        torch.where(keep, src, res["ks"], out=res["ks"])
        torch.where(keep, y, res["ky"], out=res["ky"])

    def sequence(M):
        res["wsum"].zero_(); res["kt"].zero_(); res["ks"].zero_(); res["kk"].fill_(-1); res["kj"].fill_(-1)
        for k in range(M):
            lights_sample()
            host_candidate(k)
        return torch.where(res["kk"] >= 0, res["wsum"] / M / res["kt"], 0.0)

    def samples_only(M):
        for _ in range(M):
            lights_sample()

    calls = {"pg_lights_sample": lights_sample}
    for M in MS:
        calls["fused_%d" % M] = (lambda M=M: fused(M))
        calls["sequence_%d" % M] = (lambda M=M: sequence(M))
        calls["sequence_%d_library_calls_only" % M] = (lambda M=M: samples_only(M))
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    fused(8)
    torch.cuda.synchronize()
    r = {"n_lights": L, "learned_leaves": int(learned), "kept_share_at_8": round(float((out["index"] >= 0).float().mean()), 4),
         "ms": {k: {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}}
    one = r["ms"]["pg_lights_sample"]["median"]
    for M in MS:
        m_f, m_s = r["ms"]["fused_%d" % M]["median"], r["ms"]["sequence_%d" % M]["median"]
        m_l = r["ms"]["sequence_%d_library_calls_only" % M]["median"]
        r["M_%d" % M] = {"fused_to_sequence": round(m_f / m_s, 3), "fused_to_library_calls_only": round(m_f / m_l, 3),
                         "fused_to_one_lights_sample": round(m_f / one, 3)}
    g.lightsDisable()
    g.lightsSetGeometry(None)
    return r


def table(out):
    rows = ["# tools/nee_timing.py: pg_nee_resample beside the M-fold sequence of pg_lights_sample and the host's element-wise passes in",
            "# torch, on S1 (%d KD leaves), %d lanes, the lights' delta %g, rows built from %d synthetic records;"
            % (out["forest"]["kd_leaves"], out["lanes"], DELTA, RECORDS),
            "# median ms (min - max) of %d interleaved rounds behind %d warm-ups.  Not measured: the call inside a renderer."
            % (out["launches"], out["warmup"]),
            "# L | M | fused | sequence | sequence, its M pg_lights_sample calls alone | fused / sequence | fused / those calls alone | "
            "fused / one pg_lights_sample"]
    cell = lambda v: "%.4f (%.4f - %.4f)" % (v["median"], v["min"], v["max"])  # noqa: E731
    for L in out["lights"]:
        r = out["n_lights_%d" % L]
        rows.append("# L = %d: %d learned leaves, a candidate kept on %.4f of the lanes at M = 8, one pg_lights_sample %s"
                    % (L, r["learned_leaves"], r["kept_share_at_8"], cell(r["ms"]["pg_lights_sample"])))
        for M in MS:
            q = r["M_%d" % M]
            rows.append(" | ".join([str(L), str(M), cell(r["ms"]["fused_%d" % M]), cell(r["ms"]["sequence_%d" % M]),
                                    cell(r["ms"]["sequence_%d_library_calls_only" % M]), "%.3f" % q["fused_to_sequence"],
                                    "%.3f" % q["fused_to_library_calls_only"], "%.3f" % q["fused_to_one_lights_sample"]]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--lights", default="64,1024")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import SDTree

    g = SDTree(0)
    g.load(Wk.s1_balanced_tree())
    st = g.stats()
    lights = [int(x) for x in a.lights.split(",")]
    out = {"lanes": a.lanes, "lights": lights, "launches": a.launches, "warmup": a.warmup,
           "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes)},
           "library": os.environ.get("PGSD_LIBRARY", "libpgsd.so")}
    for L in lights:
        out["n_lights_%d" % L] = measure(torch, g, a.lanes, L, a.launches, a.warmup)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(out))


if __name__ == "__main__":
    main()
