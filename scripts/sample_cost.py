"""What psamd_sample costs on the default N = 2^20 uniform cloud, 16^3 cells (one MI355X).

    python scripts/sample_cost.py [--reps R] [--warmup W] [--out profiles/sample_cost.txt]

The protocol of deposit_cost.py: one built frame (a cloud filled and stepped twice, init_iframe, build_grid); on it psamd_sample of
a random lattice at refine 1, 2 and 4, float and float4, at the export's positions (the points form) and by export order.  Beside
them in the same run: psamd_probe ACC | PHI on the same positions, psamd_export_live(POS), and the same interpolation written in
torch on the context's stream (the export, the index arithmetic, eight gathers, the weighted sum) -- the yardstick.  Every figure
is a host clock around the call plus psamd_synchronize, with an idle stream before it, after warm-up calls.  Before the timing
the two forms are checked to give the same bytes and the torch form to agree within fp32 rounding."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402


def timed(g, call, reps, warmup):
    """microseconds of call() + synchronize from an idle stream: (median, min, max)"""
    us = []
    for rep in range(warmup + reps):
        g.synchronize()
        t0 = time.perf_counter()
        call()
        g.synchronize()
        if rep >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": float(np.median(us)), "us_min": float(np.min(us)), "us_max": float(np.max(us))}


def torch_sample(pos4, F, G, cell_size, k):
    """the trilinear interpolation on psamd_deposit's lattice in torch: index arithmetic, eight gathers, a weighted sum"""
    M = G * k
    q = torch.stack([-pos4[:, 1], pos4[:, 0], -pos4[:, 2]], 1)
    u = (q * (k / cell_size) + ((G // 2) * k - 0.5)).clamp(0.0, M - 1.0)
    fl = u.floor()
    f = u - fl
    n0 = fl.long()
    n1 = (n0 + 1).clamp(max=M - 1)
    n, w = (n0, n1), (1.0 - f, f)
    flat = F.reshape(M ** 3, -1)
    out = torch.zeros((pos4.shape[0], flat.shape[1]), dtype=torch.float32, device=pos4.device)
    for d3 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                idx = (n[d3][:, 2] * M + n[d1][:, 0]) * M + n[d2][:, 1]
                out += ((w[d1][:, 0] * w[d2][:, 1]) * w[d3][:, 2])[:, None] * flat[idx]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_cost.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 1 << 20
    g = ps.ParticleSystem(ps.default_config(device=0))
    G, cs = int(g.sizes.grid_dim), float(g.cfg.cell_size)
    g.fill_particles(g.uniform_cloud(n, 12345), age=np.float32(2.0), fert_age=np.float32(1e6))
    g.step(2)
    g.init_iframe()
    g.build_grid()
    g.synchronize()
    ex = g.export_live(ps.EXPORT_POS)
    live, slots, pos4 = int(ex["count"]), g.owned_slots(), ex["pos4"].contiguous()
    res = {"n": n, "grid_dim": G, "live": live, "owned_slots": slots, "reps": a.reps, "warmup": a.warmup}
    stream = torch.cuda.ExternalStream(g.stream(), device=dev)

    def call(fn, spec):
        return lambda: fn(g.h, C.byref(spec)) == 0 or sys.exit("the call failed: " + g.lib.psamd_last_error(g.h).decode())
    rec = torch.zeros(C.sizeof(ps.SampleResult), dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    epos = torch.empty((slots, 4), dtype=torch.float32, device=dev)
    espec = ps.Export(fields=ps.EXPORT_POS, capacity=slots, pos4=epos.data_ptr())
    for k in (1, 2, 4):
        M = G * k
        for vec4 in (False, True):
            name = "refine_%d_%s" % (k, "float4" if vec4 else "float")
            F = torch.randn((M, M, M, 4) if vec4 else (M, M, M), generator=gen, dtype=torch.float32, device=dev)
            by_points, r = g.sample(F, pos4=pos4, result=True)
            by_order = g.sample(F)
            assert torch.equal(by_points.view(torch.int32), by_order[:live].view(torch.int32)), "the two forms differ"
            assert r["served"] == live, r
            ref = torch_sample(pos4, F, G, cs, k)
            worst = float((ref - by_points.reshape(live, -1)).abs().max().item())
            assert worst < 1e-4, worst
            out = torch.empty((slots, 4) if vec4 else (slots,), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            common = dict(refine=k, field=F.data_ptr(), capacity=M ** 3, out=out.data_ptr(), scale=1.0, result_dev=rec.data_ptr())
            points = ps.SampleSpec(flags=int(vec4), pos4=pos4.data_ptr(), max_count=live, **common)
            order = ps.SampleSpec(flags=int(vec4) | ps.SAMPLE_EXPORT_ORDER, max_count=slots, **common)

            def in_torch():
                call(g.lib.psamd_export_live, espec)()
                with torch.cuda.stream(stream):
                    torch_sample(epos[:live], F, G, cs, k)
            res[name] = {"points": timed(g, call(g.lib.psamd_sample, points), a.reps, a.warmup),
                         "order": timed(g, call(g.lib.psamd_sample, order), a.reps, a.warmup),
                         "torch": timed(g, in_torch, a.reps, a.warmup), "torch_max_abs_difference": worst}
    res["export_pos"] = timed(g, call(g.lib.psamd_export_live, espec), a.reps, a.warmup)
    out4 = torch.empty((live, 4), dtype=torch.float32, device=dev)
    g.probe(pos4[:1024])                                          # (the probes' scratch grows outside the timing)
    g.probe(pos4)
    probe = ps.ProbeSpec(fields=ps.PROBE_ACC | ps.PROBE_PHI, pos4=pos4.data_ptr(), max_count=live, out4=out4.data_ptr())
    res["probe"] = timed(g, call(g.lib.psamd_probe, probe), max(a.reps // 5, 3), max(a.warmup // 5, 1))
    g.calc_forces()
    g.synchronize()
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        f.write("psamd_sample at N = 2^20 (default configuration, %d^3 cells, uniform cloud of 2^20 filled and stepped twice, %d live in\n"
                "%d owned slots), one MI355X; written by scripts/sample_cost.py.  All figures from one run on one built frame: host clock\n"
                "around the call plus psamd_synchronize, the stream idle before it, median of %d calls after %d warm-ups.  points: %d\n"
                "entries at the export's positions (memset, one kernel, the record); order: PSAMD_SAMPLE_EXPORT_ORDER over the owned slots\n"
                "(memset, the tiles' live counts, one kernel, the record); torch: psamd_export_live(POS) and the same interpolation in torch\n"
                "on the context's stream (index arithmetic, eight gathers, the weighted sum).  Before the timing the two forms gave the same\n"
                "bytes and the torch form agreed within 1e-4.  psamd_probe ACC | PHI on the same positions and the export alone beside them.\n\n"
                % (G, live, slots, a.reps, a.warmup, live))
        f.write("%-24s %12s %12s %12s %14s\n" % ("lattice", "points us", "order us", "torch us", "torch / order"))
        for k in (1, 2, 4):
            for kind in ("float", "float4"):
                r = res["refine_%d_%s" % (k, kind)]
                f.write("%-24s %12.1f %12.1f %12.1f %14.2f\n" % ("refine %d %s" % (k, kind), r["points"]["us_median"], r["order"]["us_median"],
                                                              r["torch"]["us_median"], r["torch"]["us_median"] / r["order"]["us_median"]))
        f.write("%-24s %12.1f\n" % ("export_live POS", res["export_pos"]["us_median"]))
        f.write("%-24s %12.1f\n" % ("probe ACC | PHI", res["probe"]["us_median"]))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
