#!/usr/bin/env python3
"""GPU: what per-instance half-spaces (tiny_batch_set_instance_tv_linear_constraints) cost on the quadrotor -- 65 536 instances,
(12,4,10), one time-varying state and one input half-space per knot: the constraints of examples/quadrotor_tv_linear_constraints.cpp
(altitude ceiling z <= z_lim(i), total thrust <= 6), boxes off as the example has them.  Launch times from the library's "timing" option
(device events around the launches of a solve).
    python tools/instance_halfspaces_bench.py --sets shared|instance --steps 20|1 [--package DIR] [--launches 60] [--batch 65536]
--sets shared    the example's set through tiny_batch_set_tv_linear_constraints (the only form a tree without the feature has: --package
                 DIR imports tinympc_amd from DIR, e.g. a checkout of the parent commit built next to this one)
--sets instance  every instance its own set, holding the same numbers: every form solves the SAME problems in the same number of
                 iterations, and the times differ by what reading the tables costs
--ceiling 0.1    the altitude ceiling starts this far above the hover height of the reference, so that the half-spaces bind along the way
--steps 20       fused closed-loop launches of 20 MPC steps, each from the reset state and the same x0 (every timed launch is the same work);
--steps 1        one warm step per launch (advance_x0), timed once the episode has run --warmup steps
Prints one JSON line: the median, minimum and maximum launch time in ms over --launches timed launches, the iterations accumulated and
the read-backs that say which form ran.  profiles/instance_halfspaces.md keeps the numbers and how the runs were interleaved."""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", choices=("shared", "instance"), default="shared")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ceiling", type=float, default=0.1)
    ap.add_argument("--opt", action="append", default=[], help="solver option name=value")
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import tinympc_amd as tm
    prob, extra = tm.load_problem("quadrotor_20hz")
    h = extra["hover"]
    nx, nu, N, B = prob["nx"], prob["nu"], prob["N"], a.batch
    s = tm.TinyBatchSolver.from_problem(prob, B)
    xref = np.array(h["xref"], dtype=np.float64)
    ax = np.zeros((1, nx))
    ax[0, 2] = 1.0
    tAx, tAu = np.tile(ax, (N, 1)), np.tile(np.ones((1, nu)), (N - 1, 1))
    tbx = (xref[2] + a.ceiling * (1.0 + np.arange(N) / N)).reshape(1, N)
    tbu = np.full((1, N - 1), 6.0)
    if a.sets == "shared":
        s.set_tv_linear_constraints(tAx, tbx, tAu, tbu)
    else:
        s.set_instance_tv_linear_constraints(*[np.ascontiguousarray(np.broadcast_to(v, (B,) + v.shape)) for v in (tAx, tbx, tAu, tbu)])
    s.update_settings(max_iter=h["max_iter"], en_state_bound=0, en_input_bound=0, en_tv_state_linear=1, en_tv_input_linear=1)
    if a.steps > 1:
        s.set_option("steps_per_launch", a.steps)
    else:
        s.set_option("advance_x0", 1)
    for kv in a.opt:
        k, v = kv.split("=")
        s.set_option(k, int(v))
    s.set_x_ref(np.tile(xref.reshape(nx, 1), (1, N)), broadcast=True)
    rng = np.random.default_rng(2)
    x0 = np.array(h["x0"], dtype=np.float64)[None] + rng.normal(0, 0.05, (B, nx))
    s.set_x0(x0)

    def launch():
        if a.steps > 1:                              # every fused launch is the same work: the first --steps steps of the episode, from rest
            s.reset()
            s.set_x0(x0)
        s.solve_async()
    for _ in range(a.warmup if a.steps == 1 else 3):
        launch()
    s.synchronize()
    s.set_option("timing", a.launches)
    for _ in range(a.launches):
        launch()
    s.synchronize()
    ms = s.timing_ms()
    assert len(ms) == a.launches, len(ms)
    it = s.status()["iter"]
    total = s.reduce_stats()[7]                       # iterations accumulated since the last reset (fused: of the last launch's steps)
    out = dict(sets=a.sets, steps=a.steps, opts=a.opt, batch=B, launches=a.launches, median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
               accumulated_iters=float(total), last_iter_mean=float(it.mean()), last_iter_max=int(it.max()), kernel_path=s.kernel_path(),
               tlslack_active=float(np.mean(np.any(s.get("gl_tv") != 0.0, axis=(1, 2)))) if B <= 4096 else None)
    if a.sets == "instance":
        out["last_instance_linear"] = int(s.get_option("last_instance_linear"))
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
