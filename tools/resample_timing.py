#!/usr/bin/env python3
"""What pg_resample_cosine (include/pg_resample.h) costs beside the sequence a host would issue for the same method with the
calls the library had before it, one run, one JSON line on stdout and a table in --out:

  fused     pg_resample_cosine, M candidates, alpha 0.5, delta 0.1, the common outputs (no candidate arrays);
  sequence  M times: an element-wise pass in torch that draws xi and the cosine candidate of every lane (concentric disk,
            Duff's frame) and sets select = xi > alpha ? 2 : 1; pg_guide_bounce(select) -- the tree's sample for the lanes that
            selected it, the tree's pdf of the cosine candidate for the others, no emitter sample on any lane; and an
            element-wise pass that forms c, s, t, w, draws zeta and updates the reservoir.  After the M candidates one more
            pass forms W.  The host's passes use torch's own generator and functions: the sequence is timed, not compared.

on workload.s1_balanced_tree() (SURVEY's S1) at --lanes uniform positions (default 2^22), uniform normals.  Every library call
is marshalled once and launched through the C ABI; HIP events around whole candidates' worth of work; `--warmup` rounds, then
`--launches` rounds in which the fused call and the sequence of every M are timed one after the other (interleaved, so a drift
of the device's clocks meets them alike).  Medians with minimum and maximum.

Gathered bytes per lane are counted as the depth counters count them (pg_descent.hpp: 16 per KD grid entry or node, 16 per
jump-table entry, 32 per quadtree record), from instrumented launches of pg_sample and pg_pdf on the same positions:
  KD part = pg_sample's bytes - 32 * its quadtree levels;   per candidate 0.5 * pg_sample's quadtree bytes + 0.5 * pg_pdf's;
  fused(M) = KD part + 8 (the head) + M * that.      The fraction is bytes * lanes / median time / 8 TB/s.

No threshold is asserted here: the numbers are a finding.

    python3 tools/resample_timing.py [--lanes N] [--launches 20] [--warmup 5] [--out profiles/resample/timing.txt]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

MS = (1, 4, 8, 16)
ALPHA, DELTA = 0.5, 0.1


def measure(torch, g, bmin, bmax, n, launches, warmup):
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    st = g.stats()
    L, h = g._lib, g._h
    lo = torch.tensor(bmin, dtype=torch.float32, device="cuda")[:, None]
    hi = torch.tensor(bmax, dtype=torch.float32, device="cuda")[:, None]
    P = (lo + Wk.s_uniform(n, 3, 3, device="cuda") * (hi - lo)).contiguous()
    Nrm = Wk.s_directions_uniform(n, 4, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")  # noqa: E731

    def ck(rc):
        N.check(h, rc)

    # ---- gathered bytes, from the instrumented stand-alone calls
    g.enableDepthCounters(True)
    g.readDepthCounters(True)
    d_s, _ = g.sample(P, PCG32Sampler(g, n, seed=3))
    torch.cuda.synchronize()
    dc = g.readDepthCounters(True)
    sample_bytes, sample_quad = dc.layout_bytes / n, 32.0 * dc.quad_levels / n
    g.pdf(P, Wk.s_directions_uniform(n, 5, device="cuda"))
    torch.cuda.synchronize()
    dc = g.readDepthCounters(True)
    g.enableDepthCounters(False)
    kd_bytes = sample_bytes - sample_quad
    pdf_quad = dc.layout_bytes / n - kd_bytes
    per_candidate = ALPHA * pdf_quad + (1.0 - ALPHA) * sample_quad

    # ---- the fused call
    smp = PCG32Sampler(g, n, seed=7)
    d_out, w_out, t_out, s_out = f32(3, n), f32(n), f32(n), f32(n)
    i_out = torch.empty(n, dtype=torch.int32, device="cuda")
    args = N.pg_resample_args(p=P.data_ptr(), normal=Nrm.data_ptr(), rng_state=smp.state.data_ptr(), rng_inc=smp.inc.data_ptr(),
                              dir_out=d_out.data_ptr(), weight_out=w_out.data_ptr(), target_out=t_out.data_ptr(),
                              source_out=s_out.data_ptr(), index_out=i_out.data_ptr())
    prm = {M: N.pg_resample_params(M, ALPHA, DELTA, 0) for M in MS}

    def fused(M):
        ck(L.pg_resample_cosine(h, n, C.byref(prm[M]), C.byref(args), s))

    # ---- the sequence of the calls the library had before
    smp_q = PCG32Sampler(g, n, seed=7)
    dir_io, d_nee, pdf_nee, pdf = f32(3, n), Nrm, f32(n), f32(n)
    nee_off = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sel = torch.empty(n, dtype=torch.uint8, device="cuda")
    sign = torch.where(torch.signbit(Nrm[2]), -1.0, 1.0)
    a_ = -1.0 / (sign + Nrm[2])
    b_ = Nrm[0] * Nrm[1] * a_
    fs = torch.stack([1.0 + sign * Nrm[0] * Nrm[0] * a_, sign * b_, -sign * Nrm[0]])
    ft = torch.stack([b_, sign + Nrm[1] * Nrm[1] * a_, -Nrm[1]])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)

    def host_candidate_in():
        u = torch.rand((3, n), device="cuda", generator=gen)
        x, y = 2.0 * u[1] - 1.0, 2.0 * u[2] - 1.0
        q13 = x.abs() < y.abs()
        r, rp = torch.where(q13, y, x), torch.where(q13, x, y)
        phi = (math.pi / 4) * rp / torch.where(r == 0, 1.0, r)
        phi = torch.where(q13, math.pi / 2 - phi, phi)
        px, py = r * torch.cos(phi), r * torch.sin(phi)
        pz = torch.sqrt(torch.clamp(1.0 - (px * px + py * py), min=0.0)).clamp_(min=1e-10)
        torch.add(torch.add(fs * px, ft * py), Nrm * pz, out=dir_io)
        sel.copy_(torch.where(u[0] > ALPHA, 2, 1))

    def guide_bounce():
        ck(L.pg_guide_bounce(h, n, P.data_ptr(), d_nee.data_ptr(), nee_off.data_ptr(), sel.data_ptr(), dir_io.data_ptr(),
                             smp_q.state.data_ptr(), smp_q.inc.data_ptr(), pdf_nee.data_ptr(), pdf.data_ptr(), None, None, s))

    res = {"wsum": f32(n), "kt": f32(n), "ks": f32(n), "kd": f32(3, n), "kk": torch.empty(n, dtype=torch.int32, device="cuda")}

    def host_candidate_out(k):
        d = (Nrm * dir_io).sum(dim=0)
        c = torch.where(d > 0, d * (1.0 / math.pi), 0.0)
        src = ALPHA * c + (1.0 - ALPHA) * pdf
        tgt = c * (DELTA / (4 * math.pi) + (1.0 - DELTA) * pdf)
        ratio = tgt / src
        w = torch.where((src > 0) & (tgt > 0) & torch.isfinite(ratio), ratio, 0.0)
        zeta = torch.rand(n, device="cuda", generator=gen)
        res["wsum"] += w
        keep = (w > 0) & (zeta * res["wsum"] < w)
        res["kk"].copy_(torch.where(keep, k, res["kk"]))
        torch.where(keep, tgt, res["kt"], out=res["kt"])
        torch.where(keep, src, res["ks"], out=res["ks"])
        torch.where(keep, dir_io, res["kd"], out=res["kd"])

    def sequence(M):
        res["wsum"].zero_(); res["kt"].zero_(); res["ks"].zero_(); res["kk"].fill_(-1)
        for k in range(M):
            host_candidate_in()
            guide_bounce()
            host_candidate_out(k)
        return torch.where(res["kk"] >= 0, res["wsum"] / M / res["kt"], 0.0)

    def bounces_only(M):
        for _ in range(M):
            guide_bounce()

    calls = {}
    for M in MS:
        calls["fused_%d" % M] = (lambda M=M: fused(M))
        calls["sequence_%d" % M] = (lambda M=M: sequence(M))
        calls["sequence_%d_library_calls_only" % M] = (lambda M=M: bounces_only(M))
    host_candidate_in()
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
    out = {"lanes": n, "alpha": ALPHA, "delta": DELTA,
           "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes), "jump_bits": int(st.jump_bits),
                      "mean_quad_leaf_depth": round(st.mean_quad_leaf_depth, 3)},
           "kept_share": round(float((i_out >= 0).float().mean()), 4),
           "gathered_bytes_per_lane": {"kd": round(kd_bytes, 2), "head": 8, "sampling_walk": round(sample_quad, 2),
                                       "pdf_walk": round(pdf_quad, 2), "per_candidate": round(per_candidate, 2)},
           "ms": {k: {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}}
    for M in MS:
        m_f, m_s = out["ms"]["fused_%d" % M]["median"], out["ms"]["sequence_%d" % M]["median"]
        m_l = out["ms"]["sequence_%d_library_calls_only" % M]["median"]
        gathered = kd_bytes + 8 + M * per_candidate
        out["M_%d" % M] = {"fused_to_sequence": round(m_f / m_s, 3), "fused_to_library_calls_only": round(m_f / m_l, 3),
                           "fused_gathered_bytes_per_lane": round(gathered, 1),
                           "fused_fraction_of_8TBs": round(gathered * n / (m_f * 1e-3) / 8e12, 4)}
    return out


def table(out):
    rows = ["# tools/resample_timing.py: pg_resample_cosine beside the M-fold sequence of pg_guide_bounce and the host's element-wise",
            "# passes in torch, on S1 (%d KD leaves, %d quadtree nodes, jump tables of %d bits), %d lanes, alpha %g, delta %g;"
            % (out["forest"]["kd_leaves"], out["forest"]["quad_nodes"], out["forest"]["jump_bits"], out["lanes"], out["alpha"], out["delta"]),
            "# median ms (min - max) of %d interleaved rounds behind %d warm-ups; kept a candidate: %.4f of the lanes" % (
                out["launches"], out["warmup"], out["kept_share"]),
            "# gathered bytes per lane: " + json.dumps(out["gathered_bytes_per_lane"]),
            "# M | fused | sequence | sequence, its M library calls alone | fused / sequence | fused / library calls alone | fused: gathered bytes per lane | fused: fraction of 8 TB/s"]
    cell = lambda v: "%.4f (%.4f - %.4f)" % (v["median"], v["min"], v["max"])  # noqa: E731
    for M in MS:
        r = out["M_%d" % M]
        rows.append(" | ".join([str(M), cell(out["ms"]["fused_%d" % M]), cell(out["ms"]["sequence_%d" % M]),
                                cell(out["ms"]["sequence_%d_library_calls_only" % M]), "%.3f" % r["fused_to_sequence"],
                                "%.3f" % r["fused_to_library_calls_only"], "%.1f" % r["fused_gathered_bytes_per_lane"],
                                "%.4f" % r["fused_fraction_of_8TBs"]]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import radiance_timing as rt   # S1 on the device

    g, bmin, bmax, _ = rt.s1_forest(torch)
    out = measure(torch, g, bmin, bmax, a.lanes, a.launches, a.warmup)
    out.update(launches=a.launches, warmup=a.warmup, library=os.environ.get("PGSD_LIBRARY", "libpgsd.so"))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(out))


if __name__ == "__main__":
    main()
