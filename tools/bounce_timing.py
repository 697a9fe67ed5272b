#!/usr/bin/env python3
"""What pg_bounce (include/pgsd_bounce.h) costs beside the sequence of calls it stands for, one run, one JSON line on stdout:
pg_bounce with all outputs against pg_fraction_query + pg_guide_bounce + pg_radiance_query of the same build on the same
inputs, and the same for the warp form (pg_guide_bounce_warp).  The element-wise pass `select = u > f ? 2 : 1` that a host of
the sequence runs between the first two calls is timed too and reported separately: it is not part of the sum.

  s1     workload.s1_balanced_tree() at its stated size, with loaded weights and thetas;
  bench  the forest bench.py's default line times its steps on: veach-ajar at 1920 x 1080, six rendered training iterations
         with the radiance weights on; thetas loaded.

--lanes uniform positions in the forest's box, uniform directions, every lane with an emitter sample and mode CHOOSE (default
2^22); per-leaf thetas spread over [-3, 3], so that waves mix the two selections as they would in a render.  Every call is
marshalled once and launched through the C ABI directly (the host's work between two events is one ctypes call for each of
them).  HIP events around single launches: `--warmup` launches of each call, then `--launches` rounds in which the calls are
timed one after the other (interleaved, so a drift of the device's clocks meets them alike).  Per call: minimum, median, maximum.

The expectation the numbers are held against: pg_bounce stays below the sum -- two of three KD descents and two of three loads
of the tree's head are gone.

    python3 tools/bounce_timing.py [--forest s1|bench|both] [--lanes N] [--launches 20] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def thetas(n_trees):
    import numpy as np
    k = np.arange(n_trees)
    return (-3.0 + 6.0 * ((k * 7919) % 1024) / 1023.0).astype(np.float32)


def load_thetas(g):
    import numpy as np
    n = int(g.sizes().n_roots)
    g.fractionEnable()
    g.fractionLoadState({"theta": thetas(n), "m": np.zeros(n, np.float32), "v": np.zeros(n, np.float32), "p1": np.ones(n, np.float32),
                         "p2": np.ones(n, np.float32), "steps": np.zeros(n, np.uint32)})


def measure(torch, g, bmin, bmax, n, launches, warmup):
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    st = g.stats()
    L, h = g._lib, g._h
    lo = torch.tensor(bmin, dtype=torch.float32, device="cuda")[:, None]
    hi = torch.tensor(bmax, dtype=torch.float32, device="cuda")[:, None]
    P = (lo + Wk.s_uniform(n, 3, 3, device="cuda") * (hi - lo)).contiguous()
    D_nee = Wk.s_directions_uniform(n, 4, device="cuda")
    D0 = Wk.s_directions_uniform(n, 5, device="cuda")
    U = Wk.s_uniform(n, 6, 3, device="cuda").contiguous()
    u_select, u_warp = U[0].contiguous(), U[1:3].contiguous()
    f32 = lambda: torch.empty(n, dtype=torch.float32, device="cuda")  # noqa: E731
    frac, sel = g.fractionQuery(P), None
    select_pass = lambda: torch.where(u_select > frac, 2, 1).to(torch.uint8)  # noqa: E731
    sel = select_pass()
    # one dir_io per chain: a chain's estimate reads what its own guide bounce wrote
    dirs = {k: D0.clone() for k in ("seq", "seq_warp", "fused", "fused_drawn", "fused_warp", "fused_no_radiance")}
    smp = {k: PCG32Sampler(g, n, seed=7) for k in ("seq", "fused", "fused_drawn", "fused_no_radiance")}
    out_f, pn, pw, Ld, Lm = f32(), f32(), f32(), f32(), f32()
    sel_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def bounce_args(dir_io, sampler=None, u=None, given=True, radiance=True):
        a = N.pg_bounce_args(p=P.data_ptr(), dir_nee=D_nee.data_ptr(), dir_io=dir_io.data_ptr(), select_out=sel_out.data_ptr(),
                             fraction_out=out_f.data_ptr(), pdf_nee_out=pn.data_ptr(), pdf_out=pw.data_ptr())
        if given:
            a.u_select = u_select.data_ptr()
        if sampler is not None:
            a.rng_state, a.rng_inc = sampler.state.data_ptr(), sampler.inc.data_ptr()
        if u is not None:
            a.u = u.data_ptr()
        if radiance:
            a.L_dir_out, a.L_mean_out = Ld.data_ptr(), Lm.data_ptr()
        return a

    A = {"pg_bounce": bounce_args(dirs["fused"], smp["fused"]),
         "pg_bounce_drawn": bounce_args(dirs["fused_drawn"], smp["fused_drawn"], given=False),
         "pg_bounce_warp": bounce_args(dirs["fused_warp"], u=u_warp),
         "pg_bounce_no_radiance": bounce_args(dirs["fused_no_radiance"], smp["fused_no_radiance"], radiance=False)}

    def ck(rc):
        N.check(h, rc)

    calls = {
        "pg_fraction_query": lambda: ck(L.pg_fraction_query(h, n, P.data_ptr(), None, out_f.data_ptr(), s)),
        "host_select_pass": select_pass,
        "pg_guide_bounce": lambda: ck(L.pg_guide_bounce(h, n, P.data_ptr(), D_nee.data_ptr(), None, sel.data_ptr(), dirs["seq"].data_ptr(),
                                                        smp["seq"].state.data_ptr(), smp["seq"].inc.data_ptr(), pn.data_ptr(),
                                                        pw.data_ptr(), None, None, s)),
        "pg_radiance_query": lambda: ck(L.pg_radiance_query(h, n, P.data_ptr(), dirs["seq"].data_ptr(), None, Ld.data_ptr(), Lm.data_ptr(), s)),
        "pg_guide_bounce_warp": lambda: ck(L.pg_guide_bounce_warp(h, n, P.data_ptr(), D_nee.data_ptr(), None, sel.data_ptr(),
                                                                  dirs["seq_warp"].data_ptr(), u_warp.data_ptr(), pn.data_ptr(),
                                                                  pw.data_ptr(), None, None, s)),
        "pg_radiance_query_after_warp": lambda: ck(L.pg_radiance_query(h, n, P.data_ptr(), dirs["seq_warp"].data_ptr(), None, Ld.data_ptr(),
                                                                       Lm.data_ptr(), s)),
    }
    for k, a in A.items():
        calls[k] = (lambda a=a: ck(L.pg_bounce(h, n, C.byref(a), s)))
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
    out = {"lanes": n,
           "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes), "jump_bits": int(st.jump_bits),
                      "mean_quad_leaf_depth": round(st.mean_quad_leaf_depth, 3)},
           "select_2_share": round(float((sel == 2).float().mean()), 4),
           "L_dir_positive_share": round(float((Ld > 0).float().mean()), 4),
           "ms": {k: {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}}
    m = {k: v["median"] for k, v in out["ms"].items()}
    out["sequence_median_ms"] = round(m["pg_fraction_query"] + m["pg_guide_bounce"] + m["pg_radiance_query"], 4)
    out["sequence_warp_median_ms"] = round(m["pg_fraction_query"] + m["pg_guide_bounce_warp"] + m["pg_radiance_query_after_warp"], 4)
    out["bounce_below_sequence"] = bool(m["pg_bounce"] < out["sequence_median_ms"])
    out["bounce_drawn_below_sequence"] = bool(m["pg_bounce_drawn"] < out["sequence_median_ms"])
    out["bounce_warp_below_sequence"] = bool(m["pg_bounce_warp"] < out["sequence_warp_median_ms"])
    out["bounce_to_sequence"] = round(m["pg_bounce"] / out["sequence_median_ms"], 3)
    out["bounce_warp_to_sequence"] = round(m["pg_bounce_warp"] / out["sequence_warp_median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forest", default="both", choices=["s1", "bench", "both"])
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import radiance_timing as rt   # the two forests, built with the radiance weights on

    out = {"launches": a.launches, "warmup": a.warmup, "library": os.environ.get("PGSD_LIBRARY", "libpgsd.so")}
    for name, make in (("s1", rt.s1_forest), ("bench", rt.bench_forest)):
        if a.forest in (name, "both"):
            g, bmin, bmax, keep = make(torch)
            load_thetas(g)
            out[name] = measure(torch, g, bmin, bmax, a.lanes, a.launches, a.warmup)
            del g, keep
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
