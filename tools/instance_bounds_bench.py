#!/usr/bin/env python3
"""GPU: what a per-instance box (tiny_batch_set_instance_bounds) costs on the hover workload -- 65 536 quadrotor instances, (12,4,10),
launch times from the library's "timing" option (device events around the launches of a solve).
    python tools/instance_bounds_bench.py --box shared|uniform|varying --steps 20|1 [--package DIR] [--launches 60] [--batch 65536]
--box shared    the hover box through tiny_batch_set_bound_constraints (the only form a tree without the feature has: --package DIR
                imports tinympc_amd from DIR, e.g. a checkout of the parent commit built next to this one)
--box uniform   every instance its own knot-invariant box: the hover box widened by an instance-specific factor in [1, 1 + --widen]
--box varying   ... and by a knot-specific factor 1 + 1e-9 knot on top (no bound pair repeats along the horizon)
--widen 0       (the default) every instance's box holds the hover box's numbers, so that every form solves the SAME problems in the same
                number of iterations and the times differ by what reading the box costs; > 0: boxes that really differ (other iteration counts)
--steps 20      fused closed-loop launches of 20 MPC steps, each from the reset state and the same x0 (every timed launch is the same work);
--steps 1       one warm step per launch (advance_x0), timed once the episode has run --warmup steps
Prints one JSON line: the median, minimum and maximum launch time in ms over --launches timed launches (after as many untimed ones as
the episode needs to settle), the iterations of the last launch and the read-backs that say which form ran.  profiles/instance_bounds.md
keeps the numbers and how the runs were interleaved."""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", choices=("shared", "uniform", "varying"), default="shared")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--widen", type=float, default=0.0)
    ap.add_argument("--opt", action="append", default=[], help="solver option name=value (e.g. prefetch=0: the shared box on the plain launch form)")
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import tinympc_amd as tm
    prob, extra = tm.load_problem("quadrotor_20hz")
    h = extra["hover"]
    nx, nu, N, B = prob["nx"], prob["nu"], prob["N"], a.batch
    s = tm.TinyBatchSolver.from_problem(prob, B)
    box = [np.full((nx, N), float(h["x_min"])), np.full((nx, N), float(h["x_max"])), np.full((nu, N - 1), float(h["u_min"])), np.full((nu, N - 1), float(h["u_max"]))]
    if a.box == "shared":
        s.set_bound_constraints(*box)
    else:
        rng = np.random.default_rng(1)
        wide = 1.0 + a.widen * rng.uniform(0, 1, (B, 1, 1))
        knots = 1.0 + 1e-9 * np.arange(N).reshape(1, 1, N) if a.box == "varying" else np.ones((1, 1, N))
        s.set_instance_bounds(*[v[None] * wide * knots[:, :, :v.shape[1]] for v in box])
    s.update_settings(max_iter=h["max_iter"])
    if a.steps > 1:
        s.set_option("steps_per_launch", a.steps)
    else:
        s.set_option("advance_x0", 1)
    for kv in a.opt:
        k, v = kv.split("=")
        s.set_option(k, int(v))
    s.set_x_ref(np.tile(np.array(h["xref"], dtype=np.float64).reshape(nx, 1), (1, N)), broadcast=True)
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
    opt = lambda k: int(s.get_option(k))
    out = dict(box=a.box, steps=a.steps, opts=a.opt, batch=B, launches=a.launches, median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
               accumulated_iters=float(total), last_iter_mean=float(it.mean()), last_iter_max=int(it.max()), kernel_path=s.kernel_path(), last_uniform_bounds=opt("last_uniform_bounds"),
               last_prefetch=opt("last_prefetch"), last_half_rows=opt("last_half_rows"))
    if a.box != "shared":
        out["last_instance_bounds"] = opt("last_instance_bounds")
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
