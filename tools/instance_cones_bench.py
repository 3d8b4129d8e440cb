#!/usr/bin/env python3
"""GPU: what per-instance cone coefficients (tiny_batch_set_instance_cone_coefficients) cost on the rocket landing -- BASELINE config 4 as
tools/bench_configs.py config4 runs it: 65 536 instances, (6,3,10), the box and the input (thrust) cone on, the 90-step closed loop along
the reference trajectory fused into one launch under the library's default dispatch.  Launch times from the library's "timing" option
(device events around the launches of a solve).
    python tools/instance_cones_bench.py --coef shared|instance --steps 90|1 [--package DIR] [--launches 5] [--batch 65536]
--coef shared    the example's coefficients through tiny_batch_set_cone_constraints (the only form a tree without the feature has:
                 --package DIR imports tinympc_amd from DIR, e.g. a checkout of the parent commit built next to this one)
--coef instance  every instance its own coefficients, holding the same numbers: every form solves the SAME problems in the same number
                 of iterations, and the times differ by what reading the coefficients per tile (and always dividing) costs
--steps 90       the fused episode, each from the reset state and the same x0 (every timed launch is the same work); two untimed
                 episodes first, as the bench entry has them (the first tells the default dispatch what lock step costs the batch)
--steps 1        one warm step per launch (advance_x0), timed once the episode has run --warmup steps
--state-cone     the glide-slope cone on as well (config4_both_cones)
Prints one JSON line: the median, minimum and maximum launch time in ms over --launches timed launches, the iterations accumulated and
the read-backs that say which form ran.  profiles/instance_cones.md keeps the numbers and how the runs were interleaved."""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coef", choices=("shared", "instance"), default="shared")
    ap.add_argument("--steps", type=int, default=90)
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--launches", type=int, default=0, help="timed launches (default: 5 episodes / 50 warm steps)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--state-cone", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="solver option name=value")
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import tinympc_amd as tm
    prob, extra = tm.load_problem("rocket_landing_20hz")
    m = extra["mpc"]
    nx, nu, N, B = prob["nx"], prob["nu"], prob["N"], a.batch
    rng = np.random.default_rng(20260923)
    x0 = 1.1 * np.array(m["xinit"]) * (1 + 0.05 * rng.uniform(-1, 1, (B, nx)))
    xinit, xg = np.array(m["xinit"], dtype=float), np.array(m["xg"], dtype=float)
    traj = np.stack([xinit + (xg - xinit) * float(i) / (m["NTOTAL"] - 1) for i in range(m["NTOTAL"])])
    s = tm.TinyBatchSolver.from_problem(prob, B)
    s.set_bound_constraints(np.array(m["x_min"]), np.array(m["x_max"]), np.full((nu, 1), m["u_min"]), np.full((nu, 1), m["u_max"]))
    cx, cu = np.array(m["state_cone"]["c"], dtype=float).ravel(), np.array(m["input_cone"]["c"], dtype=float).ravel()
    s.set_cone_constraints(m["state_cone"]["A"], m["state_cone"]["q"], cx, m["input_cone"]["A"], m["input_cone"]["q"], cu)
    if a.coef == "instance":
        s.set_instance_cone_coefficients(np.tile(cx, (B, 1)), np.tile(cu, (B, 1)))
    s.update_settings(abs_pri_tol=m["abs_pri_tol"], max_iter=m["max_iter"], en_state_soc=int(a.state_cone), en_input_soc=1)
    uref = np.zeros((nu, N - 1))
    uref[2, :] = m["uref_z"]
    s.set_option("advance_x0", 1)
    if a.steps > 1:
        s.set_option("steps_per_launch", a.steps)
    for kv in a.opt:
        k, v = kv.split("=")
        s.set_option(k, int(v))

    def start():
        s.reset()
        s.set_u_ref(uref, broadcast=True)
        s.set_reference_trajectory(traj)              # examples/rocket_landing_mpc.cpp:111-113 (window k .. k+N-1)
        s.set_x0(x0)
    launches = a.launches or (5 if a.steps > 1 else 50)
    ms = []
    if a.steps > 1:
        for e in range(2 + launches):                 # every episode is the same work; the first two settle the dispatch
            start()
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
    total = s.reduce_stats()[7]                       # iterations accumulated since the last reset
    out = dict(coef=a.coef, steps=a.steps, state_cone=int(a.state_cone), opts=a.opt, batch=B, launches=launches, median_ms=float(np.median(ms)), min_ms=float(ms.min()),
               max_ms=float(ms.max()), accumulated_iters=float(total), last_iter_mean=float(it.mean()), last_iter_max=int(it.max()), kernel_path=s.kernel_path(),
               stretches=int(s.get_option("step_regroup_stretches")), uniform_bounds=int(s.get_option("last_uniform_bounds")))
    if a.coef == "instance":
        out["last_instance_cones"] = int(s.get_option("last_instance_cones"))
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
