#!/usr/bin/env python3
"""What pg_resample_lobe (include/ext/guiding/pg_resample_lobe.h) costs, one run, one JSON line on stdout and a table in --out:

  lobe      pg_resample_lobe, M candidates, alpha 0.5, delta 0.1, the common outputs (no candidate arrays);
  cosine    pg_resample_cosine of the same build on the same tree, positions, normals and M: what the diffuse call costs;
  host      what a host issues today for the same method: SDTree.resampleCosine(return_candidates=True) and then
            element-wise passes in torch over the (M, n) candidate arrays -- the tree's density back out of the candidates'
            source, the GGX density and the lobe b of every candidate, the new targets and weights, a reservoir pass over
            the M rows with torch's own generator, and W.  Timed, not compared: its candidates come from another mixture.

on workload.s1_balanced_tree() (SURVEY's S1, a trained tree) at --lanes uniform positions (default 2^22), uniform normals, the
viewer uniform over the hemisphere of the normal, roughness uniform in [0.02, 0.5], specular uniform in [0, 1].  Every library
call of `lobe` and `cosine` is marshalled once and launched through the C ABI; HIP events around each; `--warmup` rounds, then
`--launches` rounds in which the three are timed one after the other for every M (interleaved, so a drift of the device's
clocks meets them alike).  Medians with minimum and maximum.

No threshold is asserted here: the numbers are a finding.

    python3 tools/resample_lobe_timing.py [--lanes N] [--launches 20] [--warmup 5] [--out profiles/resample_lobe/timing.txt]
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


def host_passes(torch, info, fs, ft, Nrm, wil, rough, spec, M, gen):
    """the element-wise passes of `host` over the (M, n) candidate arrays of resampleCosine -> (direction (3, n), W (n,))"""
    n = Nrm.shape[1]
    w = info["cand_dir"]                                                      # (M, 3, n)
    wl = torch.stack([(w * fs).sum(dim=1), (w * ft).sum(dim=1), (w * Nrm).sum(dim=1)])         # (3, M, n)
    c = torch.clamp(wl[2], min=0.0) * (1.0 / math.pi)
    src = info["cand_source"]
    q = (src - ALPHA * c) * (1.0 / (1.0 - ALPHA))                             # the tree's density, back out of the source
    hv = wl + wil[:, None, :]
    hv = hv / torch.sqrt((hv * hv).sum(dim=0))
    t_ = (hv[0] / rough) ** 2 + (hv[1] / rough) ** 2 + hv[2] ** 2
    D = 1.0 / (math.pi * rough * rough * t_ * t_)
    xy = (rough * wil[0]) ** 2 + (rough * wil[1]) ** 2
    G1 = 2.0 / (1.0 + torch.sqrt(1.0 + xy / (wil[2] * wil[2])))
    ok = (wl[2] > 0) & ((hv * wil[:, None, :]).sum(dim=0) > 0) & ((hv * wl).sum(dim=0) > 0)
    gd = torch.where(ok, D * G1 / (4.0 * wil[2]), 0.0)
    b = spec * gd + (1.0 - spec) * c
    tgt = b * (DELTA / (4 * math.pi) + (1.0 - DELTA) * q)
    ratio = tgt / src
    wk = torch.where((src > 0) & (tgt > 0) & torch.isfinite(ratio), ratio, 0.0)
    cum = torch.cumsum(wk, dim=0)
    zeta = torch.rand((M, n), device=w.device, generator=gen)
    keep = (wk > 0) & (zeta * cum < wk)
    idx = torch.where(keep, torch.arange(M, device=w.device)[:, None], -1).max(dim=0).values
    pick = idx.clamp(min=0)[None, :]
    kt = torch.gather(tgt, 0, pick)[0]
    kd = torch.gather(w, 0, pick[:, None, :].expand(1, 3, n))[0]
    return kd, torch.where(idx >= 0, cum[-1] / M / kt, 0.0)


def measure(torch, g, bmin, bmax, n, launches, warmup, ms_):
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    st = g.stats()
    L, h = g._lib, g._h
    lo = torch.tensor(bmin, dtype=torch.float32, device="cuda")[:, None]
    hi = torch.tensor(bmax, dtype=torch.float32, device="cuda")[:, None]
    P = (lo + Wk.s_uniform(n, 3, 3, device="cuda") * (hi - lo)).contiguous()
    Nrm = Wk.s_directions_uniform(n, 4, device="cuda")
    Wi = Wk.s_directions_uniform(n, 5, device="cuda")
    Wi = torch.where((Wi * Nrm).sum(dim=0) < 0, -Wi, Wi).contiguous()       # towards the viewer: above the surface
    u = Wk.s_uniform(n, 6, 2, device="cuda")
    rough, spec = (0.02 + 0.48 * u[0]).contiguous(), u[1].contiguous()
    s = torch.cuda.current_stream().cuda_stream
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")  # noqa: E731

    def ck(rc):
        N.check(h, rc)

    # ---- the two fused calls
    smp = PCG32Sampler(g, n, seed=7)
    d_out, w_out, t_out, s_out = f32(3, n), f32(n), f32(n), f32(n)
    i_out = torch.empty(n, dtype=torch.int32, device="cuda")
    common = dict(p=P.data_ptr(), normal=Nrm.data_ptr(), rng_state=smp.state.data_ptr(), rng_inc=smp.inc.data_ptr(),
                  dir_out=d_out.data_ptr(), weight_out=w_out.data_ptr(), target_out=t_out.data_ptr(), source_out=s_out.data_ptr(),
                  index_out=i_out.data_ptr())
    args_cos = N.pg_resample_args(**common)
    args_lobe = N.pg_resample_lobe_args(wi=Wi.data_ptr(), roughness=rough.data_ptr(), specular=spec.data_ptr(), **common)
    prm = {M: N.pg_resample_params(M, ALPHA, DELTA, 0) for M in ms_}

    def lobe(M):
        ck(L.pg_resample_lobe(h, n, C.byref(prm[M]), C.byref(args_lobe), s))

    def cosine(M):
        ck(L.pg_resample_cosine(h, n, C.byref(prm[M]), C.byref(args_cos), s))

    # ---- the host's sequence
    smp_h = PCG32Sampler(g, n, seed=7)
    sign = torch.where(torch.signbit(Nrm[2]), -1.0, 1.0)
    a_ = -1.0 / (sign + Nrm[2])
    b_ = Nrm[0] * Nrm[1] * a_
    fs = torch.stack([1.0 + sign * Nrm[0] * Nrm[0] * a_, sign * b_, -sign * Nrm[0]])
    ft = torch.stack([b_, sign + Nrm[1] * Nrm[1] * a_, -Nrm[1]])
    wil = torch.stack([(Wi * fs).sum(dim=0), (Wi * ft).sum(dim=0), (Wi * Nrm).sum(dim=0)])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)

    def host(M):
        _, _, info = g.resampleCosine(P, Nrm, smp_h, M, ALPHA, DELTA, return_candidates=True)
        return host_passes(torch, info, fs, ft, Nrm, wil, rough, spec, M, gen)

    calls = {}
    for M in ms_:
        calls["lobe_%d" % M] = (lambda M=M: lobe(M))
        calls["cosine_%d" % M] = (lambda M=M: cosine(M))
        calls["host_%d" % M] = (lambda M=M: host(M))
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    lobe(max(ms_))
    torch.cuda.synchronize()
    kept = round(float((i_out >= 0).float().mean()), 4)
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
           "kept_share": kept,
           "ms": {k: {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}}
    for M in ms_:
        m_l, m_c, m_h = (out["ms"]["%s_%d" % (k, M)]["median"] for k in ("lobe", "cosine", "host"))
        out["M_%d" % M] = {"lobe_to_cosine": round(m_l / m_c, 3), "lobe_to_host": round(m_l / m_h, 3)}
    return out


def table(out, ms_):
    rows = ["# tools/resample_lobe_timing.py: pg_resample_lobe beside pg_resample_cosine of the same build, and beside what a host issues",
            "# today (resampleCosine with candidate arrays, then element-wise passes in torch), on S1 (%d KD leaves, %d quadtree nodes,"
            % (out["forest"]["kd_leaves"], out["forest"]["quad_nodes"]),
            "# jump tables of %d bits), %d lanes, alpha %g, delta %g, roughness uniform in [0.02, 0.5], specular uniform in [0, 1];"
            % (out["forest"]["jump_bits"], out["lanes"], out["alpha"], out["delta"]),
            "# median ms (min - max) of %d interleaved rounds behind %d warm-ups; kept a candidate: %.4f of the lanes; library %s"
            % (out["launches"], out["warmup"], out["kept_share"], out["library"]),
            "# M | pg_resample_lobe | pg_resample_cosine | host sequence | lobe / cosine | lobe / host sequence"]
    cell = lambda v: "%.4f (%.4f - %.4f)" % (v["median"], v["min"], v["max"])  # noqa: E731
    for M in ms_:
        r = out["M_%d" % M]
        rows.append(" | ".join([str(M), cell(out["ms"]["lobe_%d" % M]), cell(out["ms"]["cosine_%d" % M]), cell(out["ms"]["host_%d" % M]),
                                "%.3f" % r["lobe_to_cosine"], "%.3f" % r["lobe_to_host"]]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--candidates", type=int, nargs="*", default=list(MS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import radiance_timing as rt   # S1 on the device

    g, bmin, bmax, _ = rt.s1_forest(torch)
    ms_ = tuple(a.candidates)
    out = measure(torch, g, bmin, bmax, a.lanes, a.launches, a.warmup, ms_)
    out.update(launches=a.launches, warmup=a.warmup, library=os.path.basename(os.environ.get("PGSD_LIBRARY", "libpgsd.so")))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(out, ms_))


if __name__ == "__main__":
    main()
