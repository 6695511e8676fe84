#!/usr/bin/env python
"""sGDML stage launches beyond 48 atoms (GPU box): ms per sc_gdml_stage launch and per geometry, the share of
sc_dense_mono_step in a full HK step, and -- from rocprofv3 kernel statistics of runs with --stage-only -- the times of
the three kernels behind one launch and the FP64 rate of the Hessian kernel.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_N -o run -- python tools/gdml_large_timing.py --sizes N --stage-only
    python tools/gdml_large_timing.py --sizes 48,49,64,100,128 --stats-dir 'DIR_{N}' --out profiles/r5_gdml_large_timing.jsonl
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semiclassical_amd import propagators as PR  # noqa: E402
from semiclassical_amd._lib import lib, check, ptr  # noqa: E402
from semiclassical_amd.gdml import MolecularGDMLPotential  # noqa: E402
from semiclassical_amd.synthetic import sgdml_model, ArrayFchk  # noqa: E402

# 170 atoms are not timed: the initial-condition sampler's (2 pi)^D overflows a double beyond D ~ 386
NTRAJ = {48: 4000, 49: 4000, 64: 4000, 100: 2000, 128: 1500, 170: 1000}     # the stage Hessians take n 4 (3N)^2 8 bytes
PIPE_TFLOPS = 77.0                                                   # measured FP64 MFMA rate, profiles/r4_mfma_f64.txt
KERNELS = ("gdml_big_scalars_kernel", "gdml_big_operands_kernel", "gdml_big_hessian_kernel", "gdml_stage_kernel",
           "stage_point_kernel", "stage_consume_kernel")


def kernel_stats(pattern, N):
    """{kernel: (calls, total ns)} from a rocprofv3 --stats run of this tool with --sizes N --stage-only"""
    files = glob.glob(os.path.join(pattern.replace("{N}", str(N)), "**", "*kernel_stats.csv"), recursive=True)
    out = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in row["Name"]:
                    c, t = out.get(k, (0, 0.0))
                    out[k] = (c + int(row["Calls"]), t + float(row["TotalDurationNs"]))
    return out


def hessian_flops(N, M):
    """MFMA flops of the Hessian kernel per geometry: 32 x 32 blocks of the upper super-tiles, two products per point"""
    st = (3 * N + 63) // 64
    blocks = 0
    for sr in range(st):
        for sc in range(sr, st):
            for wr in range(2):
                for wc in range(2):
                    if sr == sc and wr > wc:
                        continue
                    if 64 * sr + 32 * wr < 3 * N and 64 * sc + 32 * wc < 3 * N:
                        blocks += 1
    return blocks * 32 * 32 * 2 * 2 * ((M + 3) // 4 * 4)


def measure(N, M, n, reps, stage_only):
    torch.set_default_dtype(torch.float64)
    model_, pos = sgdml_model(N, M, N)
    pot = MolecularGDMLPotential(model_, ArrayFchk(np.repeat(np.full(N, 12.0 * 1822.888), 3), np.zeros(3 * N), model_["z"]))
    q0 = torch.from_numpy(pos.reshape(-1))
    G = torch.diag(torch.full((3 * N,), 40.0))
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(q0, 0.0 * q0, G, ntraj=n, generator=torch.Generator().manual_seed(7))
    prop.step(pot, 0.1)                      # allocates the scratch, warms the kernels
    s = prop._stream()
    model = pot._gdml_model(prop.device)
    # host clock around synchronised batches of launches (the launches of one call are back to back on one stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        check(lib.sc_gdml_stage_scratch(model, ptr(getattr(prop, "_gdml_scratch", None)), prop._state, prop._dense, 0.0, 0,
                                        ptr(prop._epart), s))
    torch.cuda.synchronize()
    stage_ms = (time.perf_counter() - t0) * 1e3 / reps
    rec = {"N": N, "D": 3 * N, "M": M, "n": n, "route": "single-workgroup (N <= 48)" if N <= 48 else "multi-kernel (N > 48)",
           "stage_launch_ms": round(stage_ms, 4), "stage_ms_per_geometry": round(stage_ms / n, 7),
           "scratch_bytes": int(lib.sc_gdml_scratch_bytes(N, M))}
    if not stage_only:
        steps = 3
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            prop.step(pot, 0.1)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / steps
        rec["hk_step_ms"] = round(step_ms, 3)
        rec["dense_mono_share_of_step"] = round(max(0.0, step_ms - 4 * stage_ms) / step_ms, 3)
        # work per geometry against the 48-atom kernel: descriptor rows + Hessian rank-M sums, M Dd + (3N)^2 M
        rec["work_units_per_geometry"] = M * N * (N - 1) // 2 + (3 * N) ** 2 * M
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="48,49,64,100,128")
    ap.add_argument("--M", type=int, default=200)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--stage-only", action="store_true", help="only the stage launches (the rocprofv3 runs)")
    ap.add_argument("--stats-dir", default=None, help="rocprofv3 output directories, {N} = atom count")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for N in (int(x) for x in a.sizes.split(",")):
        rec = measure(N, a.M, NTRAJ.get(N, 1000), a.reps, a.stage_only)
        if a.stats_dir:
            ks = kernel_stats(a.stats_dir, N)
            launches = a.reps + 4                # the warm-up step's four stages + the timed launches
            for k, (calls, ns) in ks.items():
                rec[f"{k}_ms_per_launch"] = round(ns / 1e6 / launches, 4)
            if "gdml_big_hessian_kernel" in ks:
                t = ks["gdml_big_hessian_kernel"][1] / 1e9 / launches
                rate = hessian_flops(N, a.M) * rec["n"] / t / 1e12
                rec["hessian_fp64_tflops"] = round(rate, 2)
                rec["hessian_fraction_of_pipe"] = round(rate / PIPE_TFLOPS, 3)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if recs and "work_units_per_geometry" in recs[0]:
        base = {r["N"]: r for r in recs}
        if 48 in base and 49 in base:
            r48, r49 = base[48], base[49]
            ratio = (r49["stage_ms_per_geometry"] / r49["work_units_per_geometry"]) / \
                    (r48["stage_ms_per_geometry"] / r48["work_units_per_geometry"])
            summary = {"summary": "49-atom route vs 48-atom kernel, stage time per geometry per work unit", "ratio": round(ratio, 2)}
            recs.append(summary)
            print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
