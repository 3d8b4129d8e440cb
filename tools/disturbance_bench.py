#!/usr/bin/env python3
"""GPU: what the per-instance disturbance at the plant step (tiny_batch_set_disturbance) costs when it adds nothing -- an ALL-ZERO
sequence makes a PD form solve exactly the problems the form without it solves (x1 + 0.0 is x1 bit for bit unless x1 is -0.0, which
the iteration counts would show), so the times differ by what the PD form costs.  Launch times from the library's "timing" option
(device events around the launches of a solve).
    python tools/disturbance_bench.py --workload rocket|hover --dist none|zero --steps N [--package DIR] [--launches L] [--batch 65536]
--workload rocket   BASELINE config 4 as tools/bench_configs.py config4 runs it: (6,3,10), box and thrust cone, the closed loop along the
                    reference trajectory.  --steps 90: the fused episode, each from the reset state and the same x0, two untimed episodes
                    first; --steps 1: one warm step per launch (advance_x0), timed once the episode has run --warmup steps
--workload hover    the headline shape as bench.py sets it up: (12,4,10) quadrotor hover, the box, every instance from the same x0;
                    --steps 20: fused launches of 20 MPC steps, each from the reset state
--dist none         nothing installed (the only form a tree without the feature has: --package DIR imports tinympc_amd from DIR, e.g. a
                    checkout of the parent commit built next to this one)
--dist zero         an all-zero sequence of --steps rows per timed launch installed (for --steps 1: warmup + launches rows)
--expand-only N     no solve: time N calls of the TINY_BROADCAST setter, whose helper kernel expands [n_steps][nx] to [n_steps][batch][nx]
                    (wall clock around the synchronous call, which also allocates and frees)
Prints one JSON line: the median, minimum and maximum launch time in ms over the timed launches, the iterations accumulated and the
read-backs that say which form ran.  profiles/disturbance.md keeps the numbers and how the runs were interleaved."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("rocket", "hover"), default="rocket")
    ap.add_argument("--dist", choices=("none", "zero"), default="none")
    ap.add_argument("--steps", type=int, default=90)
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--launches", type=int, default=0, help="timed launches (default: 5 episodes / 50 warm steps)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--expand-only", type=int, default=0)
    ap.add_argument("--opt", action="append", default=[], help="solver option name=value")
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import tinympc_amd as tm
    B = a.batch
    if a.workload == "rocket":
        prob, extra = tm.load_problem("rocket_landing_20hz")
        m = extra["mpc"]
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        rng = np.random.default_rng(20260923)
        x0 = 1.1 * np.array(m["xinit"]) * (1 + 0.05 * rng.uniform(-1, 1, (B, nx)))
        xinit, xg = np.array(m["xinit"], dtype=float), np.array(m["xg"], dtype=float)
        traj = np.stack([xinit + (xg - xinit) * float(i) / (m["NTOTAL"] - 1) for i in range(m["NTOTAL"])])
        s = tm.TinyBatchSolver.from_problem(prob, B)
        s.set_bound_constraints(np.array(m["x_min"]), np.array(m["x_max"]), np.full((nu, 1), m["u_min"]), np.full((nu, 1), m["u_max"]))
        cx, cu = np.array(m["state_cone"]["c"], dtype=float).ravel(), np.array(m["input_cone"]["c"], dtype=float).ravel()
        s.set_cone_constraints(m["state_cone"]["A"], m["state_cone"]["q"], cx, m["input_cone"]["A"], m["input_cone"]["q"], cu)
        s.update_settings(abs_pri_tol=m["abs_pri_tol"], max_iter=m["max_iter"], en_state_soc=0, en_input_soc=1)
        uref = np.zeros((nu, N - 1))
        uref[2, :] = m["uref_z"]

        def start():
            s.reset()
            s.set_u_ref(uref, broadcast=True)
            s.set_reference_trajectory(traj)              # examples/rocket_landing_mpc.cpp:111-113 (window k .. k+N-1)
            s.set_x0(x0)
    else:
        prob, extra = tm.load_problem("quadrotor_20hz")
        h = extra["hover"]
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        s = tm.TinyBatchSolver.from_problem(prob, B)
        s.set_bound_constraints(np.full((nx, 1), h["x_min"]), np.full((nx, 1), h["x_max"]), np.full((nu, 1), h["u_min"]), np.full((nu, 1), h["u_max"]))
        s.update_settings(max_iter=h["max_iter"])
        xref = np.tile(np.array(h["xref"], dtype=np.float64).reshape(nx, 1), (1, N))
        hx0 = np.array(h["x0"], dtype=np.float64)

        def start():
            s.reset()
            s.set_x_ref(xref, broadcast=True)
            s.set_x0(hx0, broadcast=True)
    if a.expand_only:
        seq = np.zeros((max(a.steps, 1), nx))
        s.set_disturbance(seq)                            # (the helper's first launch loads its code)
        t = []
        for _ in range(a.expand_only):
            t0 = time.perf_counter()
            s.set_disturbance(seq)
            t.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps(dict(expand_only=a.expand_only, steps=seq.shape[0], batch=B, nx=nx, doubles=int(seq.shape[0] * B * nx), median_ms=float(np.median(t)),
                              min_ms=float(min(t)), max_ms=float(max(t)))), flush=True)
        s.close()
        return
    s.set_option("advance_x0", 1)
    if a.steps > 1:
        s.set_option("steps_per_launch", a.steps)
    for kv in a.opt:
        k, v = kv.split("=")
        s.set_option(k, int(v))
    launches = a.launches or (5 if a.steps > 1 else 50)
    rows = a.steps if a.steps > 1 else a.warmup + launches
    if a.dist == "zero":
        s.set_disturbance(np.zeros((rows, nx)))           # (one all-zero sequence for all: expanded on the device)
    ms = []
    if a.steps > 1:
        for e in range(2 + launches):                     # every episode is the same work; the first two settle the dispatch
            start()
            if a.dist == "zero":
                s.set_option("disturbance_step", 0)
            s.set_option("timing", 1)
            s.solve_async()
            t = float(np.sum(s.timing_ms()))
            if e >= 2:
                ms.append(t)
    else:
        start()
        for _ in range(a.warmup):
            s.solve_async()
        s.synchronize()
        s.set_option("timing", launches)
        for _ in range(launches):
            s.solve_async()
        s.synchronize()
        ms = list(s.timing_ms())
        assert len(ms) == launches, len(ms)
    ms = np.array(ms)
    it = s.status()["iter"]
    total = s.reduce_stats()[7]                           # iterations accumulated since the last reset
    out = dict(workload=a.workload, dist=a.dist, steps=a.steps, opts=a.opt, batch=B, launches=launches, median_ms=float(np.median(ms)), min_ms=float(ms.min()),
               max_ms=float(ms.max()), accumulated_iters=float(total), last_iter_mean=float(it.mean()), last_iter_max=int(it.max()), kernel_path=s.kernel_path(),
               stretches=int(s.get_option("step_regroup_stretches")), uniform_bounds=int(s.get_option("last_uniform_bounds")))
    if a.dist == "zero":
        out.update(last_disturbance=int(s.get_option("last_disturbance")), disturbance_step=int(s.get_option("disturbance_step")))
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
