#!/usr/bin/env python3
"""GPU: what a plant model of its own at the plant step (tiny_batch_set_plant) costs when it changes nothing -- with the MODEL installed as
the plant a PP form solves exactly the problems the form without it solves (bit for bit under the default dpp_mode), so the times differ
by what the PP form costs -- and what the host-in-the-loop form it replaces costs.  Launch times from the library's "timing" option
(device events around the launches of a solve); the host form is wall clock, read-backs and upload included.
    python tools/plant_bench.py --workload rocket|hover --plant none|shared|own|host --steps N [--noise A|generated|host [--noise-form diagonal|factor]] [--estimator G [--estimator-shared 1]] [--score device|host] [--actuator neutral|device|host] [--package DIR] [--launches L] [--batch 65536]
--workload rocket   BASELINE config 4 as tools/disturbance_bench.py runs it: (6,3,10), box and thrust cone, the closed loop along the
                    reference trajectory.  --steps 90: the fused episode; --steps 1: one warm step per launch (advance_x0)
--workload hover    the headline shape as bench.py sets it up: (12,4,10) quadrotor hover; --steps 20: fused launches of 20 MPC steps
--plant none        nothing installed (the only form a tree without the feature has: --package DIR imports tinympc_amd from DIR)
--plant shared      the model installed as ONE plant for all (TINY_BROADCAST)
--plant own         the model installed per instance ([batch] copies)
--plant host        nothing installed: per MPC step one single-step solve, x and u read back, x0 <- A x0 + B u0 + f in numpy, set_x0;
                    --steps MPC steps per episode, wall clock per episode
--state-log 1       with option "state_log" on
--noise A           measurement noise installed (tiny_batch_set_measurement_noise): every entry A * U(-1, 1), one row per MPC step of the
                    run, the counter rewound per episode.  A = 0: an all-zero sequence -- fl(x + 0) = x, so a PM form solves exactly the
                    problems the PP form with the model as plant solves, and the times differ by what the PM form costs
                    (profiles/measurement_noise.md).  With --plant none the PM form steps by the model's own block
--noise generated   a DISTURBANCE sequence of one row per MPC step generated on the device (tiny_batch_generate_disturbance: seed 7, one scale for
                    all -- --noise-form diagonal: --noise-scale on every entry; factor: a lower-triangular nx x nx factor), installed six
                    times; install_* is the wall clock of the synchronous call over the last five, install_gbs the block's bytes over the
                    median.  The run then goes on under that sequence, the counter rewound per episode (profiles/noise_generator.md)
--noise host        the only route a tree without the generator has to the same state: numpy.random.default_rng(7).standard_normal of
                    the block's shape, scaled (factor: multiplied by the factor) in numpy, and tiny_batch_set_disturbance(TINY_HOST);
                    install_* is the wall clock of all three, draw_ms / scale_ms / set_ms their medians
--estimator G       a state estimator installed (tiny_batch_set_estimator): every instance its own gain G * I (--estimator-shared 1: one for all), the estimate put at x0 at the start
                    of every episode.  With --noise 0 the innovation is zero at every step, so a PE form solves exactly the problems the PM
                    form solves, and the times differ by what the PE form costs (profiles/estimator.md)
--score device      a closed-loop score installed (tiny_batch_set_score): every instance its own weights, the workload's reference as the target and
                    limits at 0.8 of the workload's box, no log on; per episode the four arrays are read back (tiny_batch_get_score).  The
                    launch time is what the PS form costs over the form without it; wall_ms is the episode with its read-back
                    (profiles/score.md)
--score host        what it took before: nothing installed, "state_log" and "step_log" on, both logs pulled to the host after the
                    episode and scored there in numpy (the same arithmetic, vectorised over the instances); wall_ms is the episode with all
                    of that.  Both need --steps > 1
--delay D [--compensate]  a transport delay of D MPC steps in front of the actuator's stages (tiny_batch_set_actuator_delay: the PQ forms), every
                    instance the same and the queue emptied before every episode; with --compensate option "delay_compensation" (the PX forms)
--actuator neutral  an actuator model installed (tiny_batch_set_actuator) that changes nothing: every instance its own gain of ones, no other
                    stage.  The applied control is the command bit for bit, so a PA form solves exactly the problems the same form without
                    it solves (--plant shared: the PP form; with --noise 0 --estimator G --score device: the PE + PS form), and the times
                    differ by what the PA form costs (profiles/actuator.md)
--actuator device   the whole model per instance: limits at 0.8 of the workload's input box, a lag (alpha 0.7), a gain of 0.9 and a noise
                    sequence generated on the device (1 % of the box), the counter rewound per episode; with --score device wall_ms is the
                    episode with its four arrays read back
--actuator host     what it took before (with --plant host): per MPC step one single-step solve, the same four stages, the plant step and
                    the cost in numpy, set_x0; wall clock per episode
Prints one JSON line: the median, minimum and maximum time in ms over the timed launches (episodes), the iterations accumulated and
the read-backs that say which form ran.  profiles/plant.md is where the numbers go."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("rocket", "hover"), default="rocket")
    ap.add_argument("--plant", choices=("none", "shared", "own", "host"), default="none")
    ap.add_argument("--steps", type=int, default=90)
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--launches", type=int, default=0, help="timed launches (default: 5 episodes / 50 warm steps)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--state-log", type=int, default=0)
    ap.add_argument("--noise", default=None, help="a number: measurement noise of this amplitude (0: an all-zero sequence); generated | host: a disturbance sequence from the device's generator / drawn in numpy")
    ap.add_argument("--noise-form", choices=("diagonal", "factor"), default="diagonal")
    ap.add_argument("--noise-scale", type=float, default=0.01)
    ap.add_argument("--estimator", type=float, default=None, help="a state estimator with the gain G * I per instance")
    ap.add_argument("--estimator-shared", type=int, default=0, help="1: ONE gain for all (TINY_BROADCAST) instead of [batch] copies")
    ap.add_argument("--score", choices=("device", "host"), default=None, help="a closed-loop score on the device, or both logs pulled and scored in numpy")
    ap.add_argument("--actuator", choices=("neutral", "device", "host"), default=None, help="an actuator model: one that changes nothing, the whole model, or its stages in numpy (with --plant host)")
    ap.add_argument("--delay", type=int, default=0, help="a transport delay of D MPC steps in front of the actuator's stages, every instance the same (tiny_batch_set_actuator_delay)")
    ap.add_argument("--compensate", action="store_true", help="with --delay: option delay_compensation, every step solves from the model's prediction over the queue")
    a = ap.parse_args()
    if a.compensate and a.delay <= 0:
        ap.error("--compensate needs --delay D")
    if a.delay < 0 or a.delay > 8:
        ap.error("--delay: 0 .. 8 MPC steps (TINY_MAX_DELAY)")
    noise_source = a.noise if a.noise in ("generated", "host") else None
    a.noise = None if (a.noise is None or noise_source) else float(a.noise)
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
            s.set_reference_trajectory(traj)
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
    A, Bm = np.asarray(prob["A"], dtype=float).reshape(nx, nx), np.asarray(prob["B"], dtype=float).reshape(nx, nu)
    f = np.zeros(nx) if prob.get("f") is None else np.asarray(prob["f"], dtype=float).reshape(nx)
    launches = a.launches or (5 if a.steps > 1 or a.plant == "host" else 50)
    ms = []
    box = m if a.workload == "rocket" else h
    act_lo, act_hi = 0.8 * float(np.min(box["u_min"])) * np.ones((B, nu)), 0.8 * float(np.max(box["u_max"])) * np.ones((B, nu))
    act_alpha, act_gain, act_scale = np.full((B, nu), 0.7), np.full((B, nu), 0.9), 0.01 * float(np.max(box["u_max"])) * np.ones(nu)
    if a.plant == "host":
        host_cost = None
        for e in range(1 + launches):
            start()
            s.synchronize()
            t0 = time.perf_counter()
            if a.actuator == "host":
                a_state, host_cost = np.zeros((B, nu)), np.zeros(B)
                rows = np.random.default_rng(7).standard_normal((a.steps, B, nu)) * act_scale
            for k in range(a.steps):
                x0h = s.get("x0")
                s.solve()
                u0 = s.get("u")[:, :, 0]
                s.get("x")                                # (the read-back a host-side plant that also looks at the prediction pays)
                if a.actuator == "host":
                    lim = np.where(u0 < act_lo, act_lo, np.where(u0 > act_hi, act_hi, u0))
                    a_state = act_alpha * (lim - a_state) + a_state
                    u0 = a_state * act_gain + rows[k]
                xn = x0h @ A.T + u0 @ Bm.T + f
                if a.actuator == "host":
                    host_cost += np.sum(xn * xn, axis=1) + np.sum(u0 * u0, axis=1)
                s.set_x0(xn)
            s.synchronize()
            if e >= 1:
                ms.append(1e3 * (time.perf_counter() - t0))
    else:
        s.set_option("advance_x0", 1)
        if a.steps > 1:
            s.set_option("steps_per_launch", a.steps)
        if a.state_log:
            s.set_option("state_log", 1)
        if a.plant == "shared":
            s.set_plant(A, Bm, f)
        elif a.plant == "own":
            s.set_plant(np.broadcast_to(A, (B, nx, nx)), np.broadcast_to(Bm, (B, nx, nu)), np.broadcast_to(f, (B, nx)))
        if a.noise is not None:
            rows = a.steps if a.steps > 1 else a.warmup + launches
            s.set_measurement_noise(a.noise * np.random.default_rng(7).uniform(-1.0, 1.0, (rows, B, nx)))
        install = None
        if noise_source:
            rows = a.steps if a.steps > 1 else a.warmup + launches
            factor = a.noise_form == "factor"
            scale = a.noise_scale * (np.tril(np.ones((nx, nx))) / np.sqrt(np.arange(1, nx + 1))[:, None] if factor else np.ones(nx))
            install = dict(total=[], draw=[], scale=[], set=[])
            for r in range(6):
                s.synchronize()
                t0 = time.perf_counter()
                if noise_source == "generated":
                    s.generate_disturbance(7, rows, scale, factor=factor)
                    t1 = t2 = t0
                else:
                    g = np.random.default_rng(7).standard_normal((rows, B, nx))
                    t1 = time.perf_counter()
                    w = g @ scale.T if factor else g * scale
                    t2 = time.perf_counter()
                    s.set_disturbance(w)
                t3 = time.perf_counter()
                if r >= 1:
                    for k, v in (("total", t3 - t0), ("draw", t1 - t0), ("scale", t2 - t1), ("set", t3 - t2)):
                        install[k].append(1e3 * v)
        if a.estimator is not None:
            s.set_estimator(a.estimator * np.eye(nx) if a.estimator_shared else np.ascontiguousarray(np.broadcast_to(a.estimator * np.eye(nx), (B, nx, nx))))
        if a.actuator == "neutral":
            s.set_actuator(gain=np.ones((B, nu)))
        elif a.actuator == "device":
            s.set_actuator(act_lo, act_hi, act_alpha, act_gain)
            s.generate_actuation_noise(7, a.steps if a.steps > 1 else a.warmup + launches, act_scale)
        if a.delay > 0:
            s.set_actuator_delay(np.full(B, a.delay, dtype=np.int32), a.delay)
            s.set_option("delay_compensation", int(a.compensate))
        wall, scored = [], None
        if a.score is not None:
            lim = m if a.workload == "rocket" else h
            target = np.concatenate([xg if a.workload == "rocket" else np.array(h["xref"], dtype=float).reshape(nx), np.zeros(nu)])
            hi = 0.8 * np.concatenate([np.broadcast_to(np.asarray(lim["x_max"], dtype=float).ravel(), (nx,)), np.broadcast_to(np.asarray(lim["u_max"], dtype=float).ravel(), (nu,))])
            lo = 0.8 * np.concatenate([np.broadcast_to(np.asarray(lim["x_min"], dtype=float).ravel(), (nx,)), np.broadcast_to(np.asarray(lim["u_min"], dtype=float).ravel(), (nu,))])
            setup = (np.random.default_rng(11).uniform(0.5, 2.0, (B, nx + nu)),) + tuple(np.ascontiguousarray(np.broadcast_to(v, (B, nx + nu))) for v in (target, lo, hi))
            if a.score == "device":
                s.set_score(*setup)
            else:
                s.set_option("state_log", 1)
                s.set_option("step_log", 1)

        def host_score(states, u0):
            w, tg, l, u = setup
            cost, worst, count, first = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
            for k in range(len(states)):
                z = np.concatenate([states[k], u0[k]], axis=1)
                for c in range(nx + nu):
                    d = z[:, c] - tg[:, c]
                    cost = cost + (w[:, c] * d) * d
                e = np.maximum(np.max(np.maximum(z - u, l - z), axis=1), 0.0)
                worst = np.maximum(worst, e)
                first = np.where((e > 0.0) & (first < 0), k, first).astype(np.int32)
                count += e > 0.0
            return cost, worst, count, first
        if a.steps > 1:
            for e in range(2 + launches):                 # every episode is the same work; the first two settle the dispatch
                start()
                if a.score == "device":
                    s.reset_score()
                s.synchronize()
                t0 = time.perf_counter()
                if a.noise is not None:
                    s.set_option("measurement_step", 0)
                if noise_source:
                    s.set_option("disturbance_step", 0)
                if a.actuator == "device":
                    s.set_option("actuation_step", 0)
                    s.set_actuator_state(np.zeros(nu))
                if a.delay > 0:
                    s.set_actuator_queue(np.zeros((a.delay, nu)))
                if a.estimator is not None:
                    s.set_estimate(s.get("x0"))
                s.set_option("timing", 1)
                s.solve_async()
                t = float(np.sum(s.timing_ms()))
                if a.score == "device":
                    scored = s.get_score()
                elif a.score == "host":
                    scored = host_score(s.state_log(a.steps), s.step_log(a.steps)[1])
                if e >= 2:
                    ms.append(t)
                    wall.append(1e3 * (time.perf_counter() - t0))
        else:
            start()
            if a.estimator is not None:
                s.set_estimate(s.get("x0"))
            for _ in range(a.warmup):
                s.solve_async()
            s.synchronize()
            s.set_option("timing", launches)
            for _ in range(launches):
                s.solve_async()
            s.synchronize()
            ms = list(s.timing_ms())
    ms = np.array(ms)
    it = s.status()["iter"]
    total = s.reduce_stats()[7]                           # iterations accumulated since the last reset
    out = dict(workload=a.workload, plant=a.plant, steps=a.steps, state_log=a.state_log, batch=B, launches=launches, median_ms=float(np.median(ms)), min_ms=float(ms.min()),
               max_ms=float(ms.max()), accumulated_iters=float(total), last_iter_mean=float(it.mean()), last_iter_max=int(it.max()), kernel_path=s.kernel_path(),
               uniform_bounds=int(s.get_option("last_uniform_bounds")))
    if "tiny_batch_set_plant" in tm.BATCH_SYMBOLS:
        out.update(plant_kind=int(s.get_option("plant")), last_plant=int(s.get_option("last_plant")))
    if a.noise is not None:
        out.update(noise=a.noise, measurement_noise=int(s.get_option("measurement_noise")), last_measurement_noise=int(s.get_option("last_measurement_noise")))
    if noise_source and a.plant != "host":
        med = float(np.median(install["total"]))
        out.update(noise_source=noise_source, noise_form=a.noise_form, disturbance=int(s.get_option("disturbance")), last_disturbance=int(s.get_option("last_disturbance")),
                   install_median_ms=med, install_min_ms=float(min(install["total"])), install_max_ms=float(max(install["total"])),
                   install_gbs=float(int(s.get_option("disturbance")) * B * nx * 8 / (med * 1e6)))
        if noise_source == "host":
            out.update(draw_ms=float(np.median(install["draw"])), scale_ms=float(np.median(install["scale"])), set_ms=float(np.median(install["set"])))
        elif "disturbance_generated" in open(os.path.join(a.package, "include", "tinympc_amd.h")).read():
            out.update(disturbance_generated=int(s.get_option("disturbance_generated")))
    if a.estimator is not None:
        out.update(estimator_gain=a.estimator, estimator=int(s.get_option("estimator")), last_estimator=int(s.get_option("last_estimator")))
    if a.actuator is not None and a.plant != "host":
        out.update(actuator=a.actuator, actuator_kind=int(s.get_option("actuator")), actuator_lag=int(s.get_option("actuator_lag")), last_actuator=int(s.get_option("last_actuator")),
                   actuation_noise=int(s.get_option("actuation_noise")))
        if wall:
            out.update(wall_median_ms=float(np.median(wall)), wall_min_ms=float(min(wall)), wall_max_ms=float(max(wall)))
    if a.delay > 0:
        out.update(delay=a.delay, compensate=int(a.compensate), actuator_delay=int(s.get_option("actuator_delay")), last_actuator=int(s.get_option("last_actuator")))
    if a.actuator == "host":
        out.update(actuator="host", host_cost_median=float(np.median(host_cost)))
    if a.score is not None and a.steps > 1:
        out.update(score=a.score, score_kind=int(s.get_option("score")), last_score=int(s.get_option("last_score")), wall_median_ms=float(np.median(wall)), wall_min_ms=float(min(wall)),
                   wall_max_ms=float(max(wall)), cost_median=float(np.median(scored[0])), violated_share=float(np.mean(scored[2] > 0)))
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
