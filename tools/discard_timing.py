#!/usr/bin/env python
"""Wall time of run() without a discard mask and under one (discard_nonsymplectic).

    python tools/discard_timing.py [out.jsonl] [--parent DIR]

Cases: the headline (separable D = 60, n = 1e5, 200 steps: three-step visits) and the 5-mode AS model (n = 1e5, 200 steps: ONE
launch without a mask, step by step under one).  Each case three ways in the same session:
  (a) parent    the parent commit's Python over the parent commit's library: DIR is a checkout of that commit with its library
                built (git worktree add DIR HEAD~1 && python DIR/semiclassical_amd/build.py); skipped without --parent
  (b) no_mark   this tree, no mark ever made: no mask exists, the launches of the parent
  (c) all_kept  this tree, a mark at step 0 at a tolerance nobody exceeds: the mask is all ones, every step pays the masked path
Every (case, way) runs in a process of its own (two versions of the package cannot share one): warmed up once at a small size,
then timed over three runs from fresh initial conditions; the median is reported together with the three figures -- (b) against
(a) is judged by their spread."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("headline_as60", "hk_as60", 100000, 200), ("whole_loop_as5", "hk_as5_chi002", 100000, 200)]
WAYS = ("parent", "no_mark", "all_kept")


def worker(tree, name, n, nt, mark):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from tests import cases, engine_cases
    from semiclassical_amd import propagators as PR
    assert os.path.dirname(os.path.dirname(os.path.abspath(PR.__file__))) == os.path.abspath(tree)
    g = cases.load(name)

    def one(n, nt):
        pot, dt = engine_cases.engine_potential(g), float(g["dt"])
        prop = PR.HermanKlukPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]))
        prop.initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), ntraj=n, seed=5)
        slots = torch.zeros((nt, 5), dtype=torch.float64, device=prop.device)
        prop._remember_nac(pot)
        if mark:
            prop.discard_nonsymplectic(1.0)          # M(0) = 1: nobody exceeds anything
        prop.synchronize()
        t = time.perf_counter()
        prop.run(pot, dt, nt, slots=slots)
        prop.synchronize()
        elapsed = time.perf_counter() - t
        assert not mark or prop.kept_count() == n
        return elapsed, slots[:, :4].cpu().numpy()
    one(min(n, 1000), 4)
    runs, sums = zip(*[one(n, nt) for _ in range(3)])
    print(json.dumps({"ms_per_step_runs": [1e3 * t / nt for t in runs], "ms_per_step": 1e3 * float(np.median(runs)) / nt,
                      "checksum": float(np.abs(sums[0]).sum())}))


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--worker":
        tree, name, n, nt, mark = argv[1:6]
        return worker(tree, name, int(n), int(nt), mark == "1")
    parent = None
    if "--parent" in argv:
        i = argv.index("--parent")
        parent = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "discard_timing.jsonl")
    rows = []
    for label, name, n, nt in CASES:
        row = {"case": label, "fixture": name, "n": n, "steps": nt}
        for way in WAYS:
            if way == "parent" and parent is None:
                continue
            tree = parent if way == "parent" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, name, str(n), str(nt), "1" if way == "all_kept" else "0"]
            done = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=900)
            if done.returncode != 0:
                sys.exit(f"{label} / {way} failed with status {done.returncode}:\n{done.stderr[-4000:]}")       # nothing more is started
            res = json.loads(done.stdout.strip().splitlines()[-1])
            row.update({f"ms_per_step_{way}": res["ms_per_step"], f"ms_per_step_{way}_runs": res["ms_per_step_runs"],
                        f"checksum_{way}": res["checksum"]})
        if parent is not None:
            row["no_mark_vs_parent_pct"] = 100.0 * (row["ms_per_step_no_mark"] / row["ms_per_step_parent"] - 1.0)
        row["all_kept_vs_no_mark_pct"] = 100.0 * (row["ms_per_step_all_kept"] / row["ms_per_step_no_mark"] - 1.0)
        row["all_kept_minus_no_mark_us_per_step"] = 1e3 * (row["ms_per_step_all_kept"] - row["ms_per_step_no_mark"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
