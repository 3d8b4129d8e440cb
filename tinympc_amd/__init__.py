"""tinympc_amd -- MI355X-native batched TinyMPC ADMM solver (host-side mirror of the C ABI).

The product is ``libtinympc_amd.so`` (hand-written HIP for gfx950 + a C ABI, ``include/tinympc_amd.h``).
This package is a thin ctypes mirror of the reference's operator interface for the hot path
(``tiny_setup / tiny_set_bound_constraints / tiny_set_cone_constraints / tiny_update_settings /
tiny_set_x0 / tiny_set_x_ref / tiny_set_u_ref / tiny_solve``, reference
``src/tinympc/tiny_api.hpp:10-54``) with a leading batch axis.  There is no CPU fallback: if the
shared library is missing the import fails, and without a GPU ``TinyBatchSolver`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TINYMPC_AMD_LIB") or os.path.join(_HERE, "libtinympc_amd.so")   # override: A/B experiments
CSRC = os.path.join(_HERE, "csrc")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)

OK, ERR_DIM, ERR_NULL, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_HIP, ERR_ARG = 0, 1, -1, -2, -3, -4, -5
HOST, DEVICE, BROADCAST = 0, 1, 2
MAX_DELAY = 8                                      # TINY_MAX_DELAY: the longest transport delay of tiny_batch_set_actuator_delay, in MPC steps
NOISE_FACTOR = 4                                 # TinyNoiseSpec.flags: scale is an nx x nx factor


class NoiseSpec(C.Structure):
    """TinyNoiseSpec (include/tinympc_amd.h)"""
    _fields_ = [("seed", C.c_ulonglong), ("id_base", C.c_longlong), ("id_stride", C.c_longlong), ("n_steps", C.c_int), ("flags", C.c_int),
                ("scale", C.POINTER(C.c_double)), ("mean", C.POINTER(C.c_double))]


# TinyField (include/tinympc_amd.h)
FIELDS = ("x0", "Xref", "Uref", "x", "u", "vnew", "znew", "g", "y", "v", "z", "vcnew", "zcnew", "gc", "yc",
          "q", "r", "p", "d", "vlnew", "zlnew", "gl", "yl", "vlnew_tv", "zlnew_tv", "gl_tv", "yl_tv")
FIELD_ID = {n: i for i, n in enumerate(FIELDS)}
STATE_FIELDS = {"Xref", "x", "vnew", "g", "v", "vcnew", "gc", "q", "p", "vlnew", "gl", "vlnew_tv", "gl_tv"}

PLAN_BYTES = 19 * 4 + 4 + 5 * 8 + 1024 * 4      # sizeof(TinyBatchPlan): 19 ints, padding, 5 doubles, the histogram
# every extern "C" symbol include/tinympc_amd.h declares (checked by tests/test_abi_symbols.py)
BATCH_SYMBOLS = (
    "tiny_batch_device_count", "tiny_batch_setup", "tiny_batch_setup_hetero", "tiny_batch_get_cache_instance",
    "tiny_batch_destroy", "tiny_batch_set_bound_constraints", "tiny_batch_set_instance_bounds", "tiny_batch_get_instance_bounds",
    "tiny_batch_set_cone_constraints", "tiny_batch_set_linear_constraints", "tiny_batch_set_tv_linear_constraints",
    "tiny_batch_set_instance_linear_constraints", "tiny_batch_set_instance_tv_linear_constraints", "tiny_batch_get_instance_linear_constraints",
    "tiny_batch_set_instance_cone_coefficients", "tiny_batch_get_instance_cone_coefficients",
    "tiny_batch_set_disturbance", "tiny_batch_get_disturbance", "tiny_batch_set_plant", "tiny_batch_get_plant", "tiny_batch_get_state_log",
    "tiny_batch_set_measurement_noise", "tiny_batch_get_measurement_noise",
    "tiny_batch_generate_disturbance", "tiny_batch_generate_measurement_noise", "tiny_noise_generate",
    "tiny_batch_set_estimator", "tiny_batch_get_estimator", "tiny_batch_set_estimate", "tiny_batch_get_estimate", "tiny_batch_get_estimate_log",
    "tiny_batch_set_score", "tiny_batch_get_score_setup", "tiny_batch_get_score", "tiny_batch_reset_score",
    "tiny_batch_set_actuator", "tiny_batch_get_actuator", "tiny_batch_set_actuator_state", "tiny_batch_get_actuator_state",
    "tiny_batch_set_actuation_noise", "tiny_batch_get_actuation_noise", "tiny_batch_generate_actuation_noise", "tiny_actuation_noise_generate",
    "tiny_batch_get_actuation_log",
    "tiny_batch_set_actuator_delay", "tiny_batch_get_actuator_delay", "tiny_batch_set_actuator_queue", "tiny_batch_get_actuator_queue",
    "tiny_batch_update_settings", "tiny_batch_get_cache", "tiny_batch_set",
    "tiny_batch_get", "tiny_batch_reset", "tiny_batch_solve", "tiny_batch_solve_async", "tiny_batch_synchronize",
    "tiny_batch_get_status", "tiny_batch_reduce_stats", "tiny_batch_set_option", "tiny_batch_set_stream",
    "tiny_batch_phase", "tiny_batch_get_timing", "tiny_batch_get_step_log", "tiny_batch_set_reference_trajectory", "tiny_batch_last_error", "tiny_batch_supported_dims", "tiny_batch_algorithmic_bytes", "tiny_batch_kernel_path",
    "tiny_jit_compile", "tiny_jit_prebuild", "tiny_jit_used", "tiny_batch_allreduce_stats", "tiny_batch_stats_message",
    "tiny_rccl_unique_id", "tiny_rccl_comm_init_rank", "tiny_rccl_comm_destroy", "tiny_rccl_comm_count", "tiny_rccl_available", "tiny_reduce_stats_messages",
    "tiny_batch_get_option", "tiny_predict_split", "tiny_step_regroup_plan", "tiny_batch_get_plan", "tiny_batch_set_plan", "tiny_batch_set_cache", "tiny_batch_set_adaptive_rho", "tiny_batch_set_sensitivity", "tiny_batch_set_cache_state", "tiny_batch_get_cache_state",
    "tiny_batch_compute_sensitivity", "tiny_batch_get_sensitivity", "tiny_batch_get_sensitivity_instance")
GROUP_SYMBOLS = (
    "tiny_group_setup", "tiny_group_destroy", "tiny_group_shards", "tiny_group_shard", "tiny_group_shard_indices",
    "tiny_group_uses_rccl", "tiny_group_last_error", "tiny_group_set_bound_constraints", "tiny_group_set_instance_bounds", "tiny_group_set_cone_constraints",
    "tiny_group_set_linear_constraints", "tiny_group_set_tv_linear_constraints", "tiny_group_set_instance_linear_constraints",
    "tiny_group_set_instance_tv_linear_constraints", "tiny_group_set_instance_cone_coefficients", "tiny_group_set_disturbance", "tiny_group_set_plant", "tiny_group_set_measurement_noise", "tiny_group_generate_disturbance", "tiny_group_generate_measurement_noise", "tiny_group_set_estimator", "tiny_group_set_estimate", "tiny_group_set_score",
    "tiny_group_set_actuator", "tiny_group_set_actuator_state", "tiny_group_set_actuation_noise", "tiny_group_generate_actuation_noise", "tiny_group_set_actuator_delay", "tiny_group_set_actuator_queue", "tiny_group_update_settings",
    "tiny_group_set_option", "tiny_group_set", "tiny_group_get", "tiny_group_reset", "tiny_group_solve",
    "tiny_group_solve_async", "tiny_group_synchronize", "tiny_group_get_status", "tiny_group_allreduce_stats")
REFERENCE_SYMBOLS = (
    "tiny_setup", "tiny_set_bound_constraints", "tiny_set_cone_constraints", "tiny_set_linear_constraints",
    "tiny_set_tv_linear_constraints", "tiny_precompute_and_set_cache",
    "tiny_solve", "solve", "tiny_update_settings", "tiny_set_default_settings", "tiny_set_x0", "tiny_set_x_ref",
    "tiny_set_u_ref", "tiny_solve_batch", "tiny_destroy", "tiny_initialize_sensitivity_matrices", "tiny_compute_sensitivity",
    "tiny_codegen", "tiny_codegen_with_sensitivity", "codegen_create_directories", "codegen_data_header", "codegen_data_source",
    "codegen_example",
    # the phase functions of admm.hpp:12-34
    "update_linear_cost", "backward_pass_grad", "forward_pass", "update_slack", "update_dual", "termination_condition",
    "project_soc", "project_hyperplane")
PHASES = {"update_linear_cost": 1, "backward_pass_grad": 2, "forward_pass": 3, "update_slack": 4, "update_dual": 5,
          "termination_condition": 6}


class TinyMPCError(RuntimeError):
    pass


def build(force: bool = False, report=None) -> str:
    """Compile libtinympc_amd.so for gfx950 with hipcc (cross-compiles without a GPU).  make decides by mtime which
    translation units are stale; what it did is reported -- every object either REBUILT by this call or REUSED (up to date) --
    on `report` (a callable taking one line; default: stderr) and kept in csrc/_gen/build_report.json, so that a build check can
    tell a fresh compile from a shipped library.  force (or TINYMPC_AMD_BUILD_FORCE=1): `make clean` first."""
    import glob
    import json
    import time
    say = report or (lambda line: print(line, file=sys.stderr, flush=True))
    force = force or bool(os.environ.get("TINYMPC_AMD_BUILD_FORCE"))
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    watched = lambda: {p: os.path.getmtime(p) for p in glob.glob(os.path.join(CSRC, "_gen", "*.o")) + ([LIB_PATH] if os.path.exists(LIB_PATH) else [])}
    before, t0 = watched(), time.time()
    subprocess.check_call(["make", "-C", CSRC, "-j", str(min(16, os.cpu_count() or 1))], stdout=subprocess.DEVNULL)
    after = watched()
    rebuilt = sorted(os.path.basename(p) for p, m in after.items() if before.get(p) != m)
    reused = sorted(os.path.basename(p) for p, m in after.items() if before.get(p) == m)
    mode = "forced full rebuild" if force else ("rebuilt" if len(reused) == 0 else ("incremental" if rebuilt else "reused (every object up to date)"))
    say("tinympc_amd.build: %s -- %d object(s) compiled now%s, %d reused, %.1f s" %
        (mode, len(rebuilt), (" (" + ", ".join(rebuilt[:8]) + (", ..." if len(rebuilt) > 8 else "") + ")") if rebuilt else "", len(reused), time.time() - t0))
    pre = prebuild_jit(say)
    try:
        with open(os.path.join(CSRC, "_gen", "build_report.json"), "w") as f:
            json.dump({"build_mode": mode, "rebuilt": rebuilt, "reused": reused, "seconds": time.time() - t0, "when": time.time(), "jit_prebuilt": pre}, f, indent=1)
    except OSError:
        pass
    return LIB_PATH


def prebuild_jit(say=None, jobs=None):
    """The prebuilt store of run-time instantiated kernels (csrc/jit_prebuilt.txt -> tinympc_amd/jit_prebuilt/*.co): every listed name
    that is not there yet is compiled by a process of its own (hipRTC of the toolchain this build runs on; needs no GPU), files the list
    no longer names are removed.  Returns {"compiled": n, "reused": m, "failed": [...]}."""
    import concurrent.futures
    say = say or (lambda line: print(line, file=sys.stderr, flush=True))
    listing = os.path.join(CSRC, "jit_prebuilt.txt")
    store = os.path.join(_HERE, "jit_prebuilt")
    if not os.path.exists(listing):
        return {"compiled": 0, "reused": 0, "failed": []}
    names = [ln.strip() for ln in open(listing) if ln.strip() and not ln.startswith("#")]
    os.makedirs(store, exist_ok=True)
    code = ("import sys, json; sys.path.insert(0, %r); import tinympc_amd as tm\n"
            "try:\n    print('@@' + json.dumps(tm.jit_prebuild(sys.argv[1])))\nexcept Exception as e:\n    print('@@' + json.dumps([-1, repr(e)]))" % os.path.dirname(_HERE))
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_PREBUILT", None)

    def one(name):
        p = subprocess.run([sys.executable, "-c", code, name], capture_output=True, text=True, env=env)
        for ln in p.stdout.splitlines():
            if ln.startswith("@@"):
                import json
                return name, json.loads(ln[2:])
        return name, [-1, (p.stderr or "no output")[-300:]]
    t0 = __import__("time").time()
    keep, compiled, reused, failed = set(), 0, 0, []
    with concurrent.futures.ThreadPoolExecutor(jobs or min(8, os.cpu_count() or 1)) as ex:
        for name, (n, msg) in ex.map(one, names):
            if n < 0:
                failed.append((name, msg))
            else:
                keep.add(os.path.basename(msg))
                compiled += 1 if n > 0 else 0
                reused += 1 if n == 0 else 0
    if not failed:
        for f in os.listdir(store):
            if f.endswith(".co") and f not in keep:
                os.remove(os.path.join(store, f))
    say("tinympc_amd.build: run-time instantiated kernels prebuilt into tinympc_amd/jit_prebuilt/: %d compiled now, %d reused, %d failed, %.1f s"
        % (compiled, reused, len(failed), __import__("time").time() - t0))
    for name, msg in failed:
        say("  failed: %s: %s" % (name, msg))
    return {"compiled": compiled, "reused": reused, "failed": [n for n, _ in failed]}


_lib = None


def lib():
    """The loaded C ABI.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or `make -C tinympc_amd/csrc`). tinympc_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.tiny_batch_setup.argtypes = [C.POINTER(C.c_void_p), _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int]
        L.tiny_batch_setup_hetero.argtypes = [C.POINTER(C.c_void_p), _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int]
        L.tiny_batch_get_cache_instance.argtypes = [C.c_void_p, C.c_int, C.c_char_p, _dp, C.c_int]
        L.tiny_batch_destroy.argtypes = [C.c_void_p]
        L.tiny_batch_set_bound_constraints.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        L.tiny_batch_set_instance_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_instance_bounds.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        L.tiny_batch_set_cone_constraints.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _dp, C.c_int, _ip, _ip, _dp]
        L.tiny_batch_set_linear_constraints.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp]
        L.tiny_batch_set_tv_linear_constraints.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp]
        L.tiny_batch_set_instance_linear_constraints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_set_instance_tv_linear_constraints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_instance_linear_constraints.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
        L.tiny_batch_set_instance_cone_coefficients.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_instance_cone_coefficients.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.tiny_batch_set_disturbance.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.tiny_batch_get_disturbance.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.tiny_batch_set_measurement_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.tiny_batch_get_measurement_noise.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.tiny_batch_generate_disturbance.argtypes = [C.c_void_p, C.POINTER(NoiseSpec)]
        L.tiny_batch_generate_measurement_noise.argtypes = [C.c_void_p, C.POINTER(NoiseSpec)]
        L.tiny_noise_generate.argtypes = [C.POINTER(NoiseSpec), C.c_int, C.c_int, C.c_int, _dp]
        L.tiny_batch_set_estimator.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_estimator.argtypes = [C.c_void_p, C.c_int, _dp]
        L.tiny_batch_set_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_estimate.argtypes = [C.c_void_p, _dp]
        L.tiny_batch_get_estimate_log.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_batch_set_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_score_setup.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        L.tiny_batch_get_score.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.tiny_batch_reset_score.argtypes = [C.c_void_p]
        L.tiny_batch_set_actuator.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_actuator.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]
        L.tiny_batch_set_actuator_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_actuator_state.argtypes = [C.c_void_p, _dp]
        L.tiny_batch_set_actuation_noise.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.tiny_batch_get_actuation_noise.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
        L.tiny_batch_generate_actuation_noise.argtypes = [C.c_void_p, C.POINTER(NoiseSpec)]
        L.tiny_actuation_noise_generate.argtypes = [C.POINTER(NoiseSpec), C.c_int, C.c_int, _dp]
        L.tiny_batch_get_actuation_log.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_batch_set_actuator_delay.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.tiny_batch_get_actuator_delay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.tiny_batch_set_actuator_queue.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_actuator_queue.argtypes = [C.c_void_p, _dp]
        L.tiny_batch_update_settings.argtypes = [C.c_void_p, C.c_double, C.c_double] + [C.c_int] * 10
        L.tiny_batch_get_cache.argtypes = [C.c_void_p, C.c_char_p, _dp, C.c_int]
        L.tiny_batch_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.tiny_batch_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.tiny_batch_reset.argtypes = [C.c_void_p]
        L.tiny_batch_solve.argtypes = [C.c_void_p]
        L.tiny_batch_solve_async.argtypes = [C.c_void_p]
        L.tiny_batch_synchronize.argtypes = [C.c_void_p]
        L.tiny_batch_get_status.argtypes = [C.c_void_p, _ip, _ip, _ip, _dp]
        L.tiny_batch_reduce_stats.argtypes = [C.c_void_p, _dp, C.c_void_p]
        L.tiny_batch_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.tiny_batch_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.tiny_batch_get_timing.argtypes = [C.c_void_p, _fp, C.c_int]
        L.tiny_batch_set_reference_trajectory.argtypes = [C.c_void_p, _dp, C.c_int, _ip, C.c_int]
        L.tiny_batch_get_step_log.argtypes = [C.c_void_p, _ip, _dp, C.c_int]
        L.tiny_batch_set_plant.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.tiny_batch_get_plant.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
        L.tiny_batch_get_state_log.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_batch_last_error.argtypes = [C.c_void_p]
        L.tiny_batch_last_error.restype = C.c_char_p
        L.tiny_batch_supported_dims.argtypes = [_ip, C.c_int]
        L.tiny_batch_kernel_path.argtypes = [C.c_void_p]
        L.tiny_batch_algorithmic_bytes.argtypes = [C.c_void_p, C.c_int]
        L.tiny_batch_algorithmic_bytes.restype = C.c_long
        L.tiny_jit_compile.argtypes = [C.c_char_p, _ip, C.c_char_p, C.c_int]
        L.tiny_jit_compile.restype = C.c_long
        L.tiny_jit_prebuild.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.tiny_jit_prebuild.restype = C.c_long
        L.tiny_jit_used.argtypes = [C.c_char_p, C.c_int]
        L.tiny_batch_stats_message.argtypes = [C.c_void_p, C.c_void_p]
        L.tiny_batch_set_cache.argtypes = [C.c_void_p, C.c_char_p, _dp]
        L.tiny_predict_split.argtypes = [C.POINTER(C.c_uint), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp]
        L.tiny_step_regroup_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int]
        L.tiny_batch_get_plan.argtypes = [C.c_void_p, C.c_void_p]
        L.tiny_batch_set_plan.argtypes = [C.c_void_p, C.c_void_p]
        L.tiny_batch_get_option.argtypes = [C.c_void_p, C.c_char_p]
        L.tiny_batch_get_option.restype = C.c_long
        L.tiny_batch_set_adaptive_rho.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int]
        L.tiny_batch_set_sensitivity.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        L.tiny_batch_compute_sensitivity.argtypes = [C.c_void_p]
        L.tiny_batch_get_sensitivity.argtypes = [C.c_void_p, C.c_char_p, _dp, C.c_int]
        L.tiny_batch_get_sensitivity_instance.argtypes = [C.c_void_p, C.c_int, C.c_char_p, _dp, C.c_int]
        L.tiny_batch_set_cache_state.argtypes = [C.c_void_p, C.c_char_p, _dp]
        L.tiny_batch_get_cache_state.argtypes = [C.c_void_p, C.c_char_p, _dp]
        L.tiny_rccl_unique_id.argtypes = [C.c_void_p]
        L.tiny_rccl_comm_init_rank.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.tiny_rccl_comm_destroy.argtypes = [C.c_void_p]
        L.tiny_rccl_comm_count.argtypes = [C.c_void_p]
        L.tiny_reduce_stats_messages.argtypes = [_dp, C.c_int, C.c_long, _dp]
        L.tiny_batch_allreduce_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_long, _dp]
        L.tiny_group_setup.argtypes = [C.POINTER(C.c_void_p), _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_int,
                                       C.c_int, _ip, C.c_int, C.c_int, C.c_int]
        for name in ("tiny_group_destroy", "tiny_group_shards", "tiny_group_uses_rccl", "tiny_group_reset", "tiny_group_solve",
                     "tiny_group_solve_async", "tiny_group_synchronize"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.tiny_group_shard.argtypes = [C.c_void_p, C.c_int]
        L.tiny_group_shard.restype = C.c_void_p
        L.tiny_group_shard_indices.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int]
        L.tiny_group_last_error.argtypes = [C.c_void_p]
        L.tiny_group_last_error.restype = C.c_char_p
        L.tiny_group_set_bound_constraints.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        L.tiny_group_set_instance_bounds.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        L.tiny_group_set_cone_constraints.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _dp, C.c_int, _ip, _ip, _dp]
        L.tiny_group_set_linear_constraints.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp]
        L.tiny_group_set_tv_linear_constraints.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp]
        L.tiny_group_set_instance_linear_constraints.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp]
        L.tiny_group_set_instance_tv_linear_constraints.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp]
        L.tiny_group_set_instance_cone_coefficients.argtypes = [C.c_void_p, _dp, _dp, C.c_int]
        L.tiny_group_set_disturbance.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int]
        L.tiny_group_set_measurement_noise.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int]
        L.tiny_group_generate_disturbance.argtypes = [C.c_void_p, C.POINTER(NoiseSpec)]
        L.tiny_group_generate_measurement_noise.argtypes = [C.c_void_p, C.POINTER(NoiseSpec)]
        L.tiny_group_set_estimator.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_group_set_estimate.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_group_set_score.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.c_int]
        L.tiny_group_set_actuator.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, C.c_int]
        L.tiny_group_set_actuator_state.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_group_set_actuation_noise.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int]
        L.tiny_group_generate_actuation_noise.argtypes = [C.c_void_p, C.POINTER(NoiseSpec)]
        L.tiny_group_set_actuator_delay.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int]
        L.tiny_group_set_actuator_queue.argtypes = [C.c_void_p, _dp, C.c_int]
        L.tiny_group_set_plant.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int]
        L.tiny_group_update_settings.argtypes = [C.c_void_p, C.c_double, C.c_double] + [C.c_int] * 10
        L.tiny_group_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.tiny_group_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.tiny_group_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tiny_group_get_status.argtypes = [C.c_void_p, _ip, _ip, _ip, _dp]
        L.tiny_group_allreduce_stats.argtypes = [C.c_void_p, _dp]
        _lib = L
    return _lib


def device_count() -> int:
    return int(lib().tiny_batch_device_count())


def supported_dims():
    buf = (C.c_int * (3 * 256))()
    n = lib().tiny_batch_supported_dims(buf, 256)
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]


def jit_compile(instantiation: str):
    """Compile one run-time instantiated kernel by its C++ name without loading it (needs no GPU); with the environment
    variable TINYMPC_AMD_JIT_CACHE=<directory> the code object is looked up / kept there.  Returns (bytes, from_disk)."""
    msg = C.create_string_buffer(2048)
    hit = C.c_int(0)
    n = lib().tiny_jit_compile(instantiation.encode(), C.byref(hit), msg, len(msg))
    if n <= 0:
        raise RuntimeError(msg.value.decode(errors="replace") or f"tiny_jit_compile failed ({n})")
    return int(n), bool(hit.value)


def jit_prebuild(instantiation: str, directory=None):
    """Build time: compile one run-time instantiated kernel with THIS process's hipRTC and keep it in the prebuilt store (default: next
    to the library, tinympc_amd/jit_prebuilt/).  Returns (code-object size -- 0 if it was already there --, its file)."""
    msg = C.create_string_buffer(2048)
    n = lib().tiny_jit_prebuild(instantiation.encode(), directory.encode() if directory else None, msg, len(msg))
    if n < 0:
        raise RuntimeError(msg.value.decode(errors="replace") or f"tiny_jit_prebuild failed ({n})")
    return int(n), msg.value.decode(errors="replace")          # (size -- 0: it was there already --, file)


def jit_used():
    """C++ names of the kernels this process instantiated at run time so far (what to feed jit_compile elsewhere)."""
    n = lib().tiny_jit_used(None, 0)
    buf = C.create_string_buffer(512 * max(n, 1))
    lib().tiny_jit_used(buf, len(buf))
    return [l for l in buf.value.decode().split("\n") if l]


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _colmajor(a, shape):
    """numpy (rows, cols) -> flat column-major doubles."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    a = np.broadcast_to(a, shape)
    return np.ascontiguousarray(a.T).ravel()


def noise_spec(batch, nx, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
    """TinyNoiseSpec from numpy arrays.  scale: (nx,) or (batch, nx) -- with factor=True the MATRIX S (nx, nx) or (batch, nx, nx), passed
    on column-major --; mean: None, (nx,) or (batch, nx); a 1-D scale (2-D factor) is one for all, and then the mean is (nx,) too.
    Returns (spec, the arrays it points into: keep them alive across the call)"""
    S = np.asarray(scale, dtype=np.float64)
    one = S.ndim == (2 if factor else 1)
    n = 1 if one else batch
    want = (n, nx, nx) if factor else (n, nx)
    if one:
        S = S[None]
    if S.shape != want:
        raise ValueError(f"noise scale: {want[1:]} or {(batch,) + want[1:]}, got {np.shape(scale)}")
    flat = np.ascontiguousarray(S.transpose(0, 2, 1) if factor else S).ravel()
    mu = None
    if mean is not None:
        mu = _f64(mean)
        if mu.shape != ((nx,) if one else (batch, nx)):
            raise ValueError(f"noise mean: {(nx,) if one else (batch, nx)} with this scale, got {mu.shape}")
        mu = mu.ravel()
    spec = NoiseSpec(int(seed) & (2**64 - 1), int(id_base), int(id_stride), int(n_steps), HOST | (BROADCAST if one else 0) | (NOISE_FACTOR if factor else 0),
                     flat.ctypes.data_as(_dp), None if mu is None else mu.ctypes.data_as(_dp))
    return spec, (flat, mu)


def noise_generate(seed, stream, n_steps, batch, nx, scale, mean=None, factor=False, id_base=0, id_stride=1):
    """the rows tiny_batch_generate_disturbance (stream 0) / ..._measurement_noise (stream 1) fill, on the host (no GPU touched):
    (n_steps, batch, nx), bit for bit what the device writes.  scale / mean: see noise_spec"""
    spec, keep = noise_spec(batch, nx, seed, n_steps, scale, mean, factor, id_base, id_stride)
    out = np.zeros((max(int(n_steps), 0), batch, nx))
    rc = lib().tiny_noise_generate(C.byref(spec), int(stream), int(batch), int(nx), out.ctypes.data_as(_dp))
    if rc != OK:
        raise TinyMPCError(f"noise_generate failed ({rc}): a refused argument")
    return out


def actuation_noise_generate(seed, n_steps, batch, nu, scale, mean=None, factor=False, id_base=0, id_stride=1):
    """the rows tiny_batch_generate_actuation_noise fills (stream 2, rows of nu entries), on the host (no GPU touched): (n_steps, batch, nu),
    bit for bit what the device writes.  scale / mean: see noise_spec, with nu for nx"""
    spec, keep = noise_spec(batch, nu, seed, n_steps, scale, mean, factor, id_base, id_stride)
    out = np.zeros((max(int(n_steps), 0), batch, nu))
    rc = lib().tiny_actuation_noise_generate(C.byref(spec), int(batch), int(nu), out.ctypes.data_as(_dp))
    if rc != OK:
        raise TinyMPCError(f"actuation_noise_generate failed ({rc}): a refused argument")
    return out


class TinyBatchSolver:
    """``batch`` independent MPC QPs sharing one (A, B, f, Q, R, rho): device-resident state, one
    HIP launch per ``solve()``.  Method names / argument meaning follow ``tiny_api.hpp``."""

    def __init__(self, A, B, f, Q, R, rho, nx, nu, N, batch, device=0, verbose=0):
        self._h = C.c_void_p()
        self.nx, self.nu, self.N, self.batch = int(nx), int(nu), int(N), int(batch)
        A = _colmajor(A, (nx, nx))
        Bm = _colmajor(B, (nx, nu))
        fv = _f64(np.zeros(nx) if f is None else f).ravel()
        Q = _f64(Q)
        R = _f64(R)
        Qd = (np.diag(Q) if Q.ndim == 2 else Q).copy()      # callers pass Q.asDiagonal() (dense) or the diagonal
        Rd = (np.diag(R) if R.ndim == 2 else R).copy()
        rc = lib().tiny_batch_setup(C.byref(self._h), A.ctypes.data_as(_dp), Bm.ctypes.data_as(_dp),
                                    fv.ctypes.data_as(_dp), Qd.ctypes.data_as(_dp), Rd.ctypes.data_as(_dp),
                                    float(rho), nx, nu, N, batch, device, verbose)
        if rc != OK:
            self._h = C.c_void_p()
            msg = {ERR_NO_DEVICE: "no MI355X / HIP device available (there is no CPU fallback)",
                   ERR_UNSUPPORTED: f"(nx,nu,N)=({nx},{nu},{N}) has no compiled kernel; have {supported_dims()}",
                   ERR_DIM: "bad dimensions"}.get(rc, f"error {rc}")
            raise TinyMPCError(f"tiny_batch_setup failed: {msg}")

    @classmethod
    def hetero(cls, A, B, f, Q, R, rho, N, device=0):
        """Heterogeneous batch: A [batch, nx, nx], B [batch, nx, nu], f [batch, nx] or None, Q [batch, nx], R [batch, nu]
        (user diagonals), rho [batch].  The Riccati recursion runs on the GPU for every instance."""
        A = np.asarray(A, dtype=np.float64)
        Bm = np.asarray(B, dtype=np.float64)
        batch, nx, nu = A.shape[0], A.shape[1], Bm.shape[2]
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.nx, self.nu, self.N, self.batch = nx, nu, int(N), batch
        Af = np.ascontiguousarray(A.transpose(0, 2, 1)).ravel()          # column-major per instance
        Bf = np.ascontiguousarray(Bm.transpose(0, 2, 1)).ravel()
        ff = None if f is None else _f64(f).ravel()
        Qf, Rf, rf = _f64(Q).ravel(), _f64(R).ravel(), _f64(np.broadcast_to(rho, (batch,))).ravel()
        rc = lib().tiny_batch_setup_hetero(C.byref(self._h), Af.ctypes.data_as(_dp), Bf.ctypes.data_as(_dp),
                                           None if ff is None else ff.ctypes.data_as(_dp), Qf.ctypes.data_as(_dp),
                                           Rf.ctypes.data_as(_dp), rf.ctypes.data_as(_dp), nx, nu, int(N), batch, device, 0)
        if rc != OK:
            self._h = C.c_void_p()
            raise TinyMPCError(f"tiny_batch_setup_hetero failed ({rc})")
        return self

    def cache_instance(self, instance, name):
        shapes = {"Kinf": (self.nu, self.nx), "Pinf": (self.nx, self.nx), "Quu_inv": (self.nu, self.nu),
                  "AmBKt": (self.nx, self.nx), "APf": (self.nx, 1), "BPf": (self.nu, 1), "Q": (self.nx, 1),
                  "R": (self.nu, 1), "riccati_iters": (1, 1)}
        r, c = shapes[name]
        out = np.zeros(r * c)
        n = lib().tiny_batch_get_cache_instance(self._h, int(instance), name.encode(), out.ctypes.data_as(_dp), r * c)
        assert n == r * c, (n, name)
        return out.reshape((r, c), order="F")

    @classmethod
    def from_problem(cls, prob, batch, device=0):
        return cls(prob["A"], prob["B"], prob.get("f"), prob["Q"], prob["R"], prob["rho"], prob["nx"], prob["nu"],
                   prob["N"], batch, device)

    # ---- lifetime
    def close(self):
        if getattr(self, "_h", None):
            lib().tiny_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc not in (OK,):
            raise TinyMPCError(f"{what} failed ({rc}): {lib().tiny_batch_last_error(self._h).decode()}")

    # ---- problem family (tiny_api.hpp:13-18, 36-43)
    def set_bound_constraints(self, x_min, x_max, u_min, u_max):
        nx, nu, N = self.nx, self.nu, self.N
        a = [_colmajor(x_min, (nx, N)), _colmajor(x_max, (nx, N)), _colmajor(u_min, (nu, N - 1)),
             _colmajor(u_max, (nu, N - 1))]
        self._check(lib().tiny_batch_set_bound_constraints(self._h, *[v.ctypes.data_as(_dp) for v in a]),
                    "set_bound_constraints")

    def _instance_boxes(self, x_min, x_max, u_min, u_max):
        """[batch, nx, N] x 2, [batch, nu, N-1] x 2 -> flat [batch][knot][row] doubles (per instance column-major)"""
        shapes = [(self.batch, self.nx, self.N)] * 2 + [(self.batch, self.nu, self.N - 1)] * 2
        return [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), s).transpose(0, 2, 1)).ravel()
                for v, s in zip((x_min, x_max, u_min, u_max), shapes)]

    def set_instance_bounds(self, x_min, x_max, u_min, u_max):
        """every instance its own box: x_min / x_max [batch, nx, N], u_min / u_max [batch, nu, N-1]"""
        a = self._instance_boxes(x_min, x_max, u_min, u_max)
        self._check(lib().tiny_batch_set_instance_bounds(self._h, *[v.ctypes.data_as(C.c_void_p) for v in a], HOST), "set_instance_bounds")

    def set_instance_bounds_device(self, x_min, x_max, u_min, u_max):
        """the same from device pointers (ints) to [batch][N][nx] | [batch][N-1][nu] doubles resident in HBM (copied)"""
        self._check(lib().tiny_batch_set_instance_bounds(self._h, *[C.c_void_p(int(p)) for p in (x_min, x_max, u_min, u_max)], DEVICE),
                    "set_instance_bounds_device")

    def instance_bounds(self, i):
        """(x_min, x_max [nx, N], u_min, u_max [nu, N-1]) instance i is bound by, as set; on a shared box: the shared one"""
        out = [np.zeros((self.N, self.nx)), np.zeros((self.N, self.nx)), np.zeros((self.N - 1, self.nu)), np.zeros((self.N - 1, self.nu))]
        self._check(lib().tiny_batch_get_instance_bounds(self._h, int(i), *[v.ctypes.data_as(_dp) for v in out]), "instance_bounds")
        return tuple(v.T.copy() for v in out)

    def set_cone_constraints(self, Acx, qcx, cx, Acu, qcu, cu):
        """STATE triple first (the positional order of the reference's definition, tiny_api.cpp:176-178)."""
        ia = [np.ascontiguousarray(np.asarray(v, dtype=np.int32).ravel()) for v in (Acx, qcx, Acu, qcu)]
        da = [_f64(v).ravel() for v in (cx, cu)]
        self._check(lib().tiny_batch_set_cone_constraints(
            self._h, len(ia[0]), ia[0].ctypes.data_as(_ip), ia[1].ctypes.data_as(_ip), da[0].ctypes.data_as(_dp),
            len(ia[2]), ia[2].ctypes.data_as(_ip), ia[3].ctypes.data_as(_ip), da[1].ctypes.data_as(_dp)),
            "set_cone_constraints")

    def _instance_cones(self, cx, cu):
        """[batch, n_state_cones], [batch, n_input_cones] (None: that family keeps the shared coefficients) -> flat arrays; None stays None"""
        return [None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(self.batch, -1)).ravel() for v in (cx, cu)]

    def set_instance_cone_coefficients(self, cx, cu):
        """every instance its own cone coefficients on the cones set_cone_constraints installed: cx [batch, n_state_cones], cu
        [batch, n_input_cones]; None: that family keeps the shared coefficients for every instance"""
        a = self._instance_cones(cx, cu)
        p = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in a]
        self._check(lib().tiny_batch_set_instance_cone_coefficients(self._h, p[0], p[1], HOST), "set_instance_cone_coefficients")

    def set_instance_cone_coefficients_device(self, cx, cu):
        """the same from device pointers (ints; 0: none) to [batch][count] doubles resident in HBM (copied)"""
        p = [C.c_void_p(int(v)) if v else None for v in (cx, cu)]
        self._check(lib().tiny_batch_set_instance_cone_coefficients(self._h, p[0], p[1], DEVICE), "set_instance_cone_coefficients_device")

    def get_instance_cone_coefficients(self, i):
        """(cx [n_state_cones], cu [n_input_cones]) instance i is held to, as set; on a shared set: the shared values"""
        out = [np.zeros(self.get_option("n_state_cones")), np.zeros(self.get_option("n_input_cones"))]
        self._check(lib().tiny_batch_get_instance_cone_coefficients(self._h, int(i), *[v.ctypes.data_as(_dp) for v in out]),
                    "get_instance_cone_coefficients")
        return tuple(out)

    def _disturbance(self, w):
        """(n_steps, batch, nx), or (n_steps, nx) for one sequence for all -> (flat array, n_steps, broadcast flag)"""
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim == 2 and w.shape[1] == self.nx and w.shape[0] > 0:
            return w.ravel(), w.shape[0], BROADCAST
        if w.ndim != 3 or w.shape[0] == 0 or w.shape[1:] != (self.batch, self.nx):
            raise ValueError(f"disturbance: (n_steps, {self.batch}, {self.nx}) or (n_steps, {self.nx}), got {w.shape}")
        return w.ravel(), w.shape[0], 0

    def set_disturbance(self, w):
        """every instance its own additive disturbance at the plant step of a closed loop (advance_x0, steps_per_launch > 1): the x0
        MPC step k hands on is x1 + w[k, i].  w: (n_steps, batch, nx), or (n_steps, nx) for one sequence for all; None removes it.
        The step counter (option "disturbance_step") starts at 0 and advances with every plant step; steps outside w add nothing"""
        if w is None:
            return self._check(lib().tiny_batch_set_disturbance(self._h, None, 0, HOST), "set_disturbance")
        flat, n, bc = self._disturbance(w)
        self._check(lib().tiny_batch_set_disturbance(self._h, flat.ctypes.data_as(C.c_void_p), n, HOST | bc), "set_disturbance")

    def set_disturbance_device(self, w, n_steps, broadcast=False):
        """the same from a device pointer (int) to [n_steps][batch][nx] doubles ([n_steps][nx] with broadcast) resident in HBM (copied)"""
        self._check(lib().tiny_batch_set_disturbance(self._h, C.c_void_p(int(w)), int(n_steps), DEVICE | (BROADCAST if broadcast else 0)),
                    "set_disturbance_device")

    def get_disturbance(self, step, i):
        """w[step, i] (nx,) as installed"""
        out = np.zeros(self.nx)
        self._check(lib().tiny_batch_get_disturbance(self._h, int(step), int(i), out.ctypes.data_as(_dp)), "get_disturbance")
        return out

    def set_measurement_noise(self, v):
        """measurement noise in a closed loop (advance_x0, steps_per_launch > 1): x0 is the plant's true state, MPC step k solves from
        x0 + v[k, i] and the plant step starts from x0.  v: (n_steps, batch, nx), or (n_steps, nx) for one sequence for all; None
        removes it.  The step counter (option "measurement_step") starts at 0 and advances with every MPC step of such a launch; steps
        outside v measure x0 itself"""
        if v is None:
            return self._check(lib().tiny_batch_set_measurement_noise(self._h, None, 0, HOST), "set_measurement_noise")
        flat, n, bc = self._disturbance(v)
        self._check(lib().tiny_batch_set_measurement_noise(self._h, flat.ctypes.data_as(C.c_void_p), n, HOST | bc), "set_measurement_noise")

    def set_measurement_noise_device(self, v, n_steps, broadcast=False):
        """the same from a device pointer (int) to [n_steps][batch][nx] doubles ([n_steps][nx] with broadcast) resident in HBM (copied)"""
        self._check(lib().tiny_batch_set_measurement_noise(self._h, C.c_void_p(int(v)), int(n_steps), DEVICE | (BROADCAST if broadcast else 0)),
                    "set_measurement_noise_device")

    def get_measurement_noise(self, step, i):
        """v[step, i] (nx,) as installed"""
        out = np.zeros(self.nx)
        self._check(lib().tiny_batch_get_measurement_noise(self._h, int(step), int(i), out.ctypes.data_as(_dp)), "get_measurement_noise")
        return out

    def generate_disturbance(self, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
        """a disturbance sequence of n_steps rows GENERATED on the device: row k of instance i is mean + scale * g, g the standard normals
        of (seed, stream 0, id_base + i * id_stride, k) -- a pure function of those, so the noise of an instance does not depend on the
        batch it sits in.  scale (nx,) | (batch, nx); factor=True: a matrix S (nx, nx) | (batch, nx, nx), row = mean + S g (correlated
        noise from a Cholesky factor).  Installed like set_disturbance's; set_disturbance(None) removes it"""
        spec, keep = noise_spec(self.batch, self.nx, seed, n_steps, scale, mean, factor, id_base, id_stride)
        self._check(lib().tiny_batch_generate_disturbance(self._h, C.byref(spec)), "generate_disturbance")

    def generate_measurement_noise(self, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
        """the same for the measurement noise (stream 1: other deviates than the disturbance's under the same seed)"""
        spec, keep = noise_spec(self.batch, self.nx, seed, n_steps, scale, mean, factor, id_base, id_stride)
        self._check(lib().tiny_batch_generate_measurement_noise(self._h, C.byref(spec)), "generate_measurement_noise")

    def _plant(self, A_p, B_p, f_p):
        """A_p (batch, nx, nx) | (nx, nx), B_p (batch, nx, nu) | (nx, nu), f_p (batch, nx) | (nx,) | None -> (flat column-major arrays,
        broadcast flag)"""
        A, Bm = np.asarray(A_p, dtype=np.float64), np.asarray(B_p, dtype=np.float64)
        one = A.ndim == 2
        if one:
            A, Bm = A[None], Bm[None]
        n = 1 if one else self.batch
        if A.shape != (n, self.nx, self.nx) or Bm.shape != (n, self.nx, self.nu):
            raise ValueError(f"plant: A_p ({n}, {self.nx}, {self.nx}), B_p ({n}, {self.nx}, {self.nu}), got {A.shape}, {Bm.shape}")
        f = None if f_p is None else _f64(f_p).reshape(n, self.nx).ravel()
        return np.ascontiguousarray(A.transpose(0, 2, 1)).ravel(), np.ascontiguousarray(Bm.transpose(0, 2, 1)).ravel(), f, (BROADCAST if one else 0)

    def set_plant(self, A_p, B_p=None, f_p=None):
        """a plant model of its own at the plant step of a closed loop (advance_x0, steps_per_launch > 1): the state handed on is
        f_p + A_p x0 + B_p u0, one fused multiply-add chain in that order, while the controller keeps its own model.  A_p (batch, nx, nx),
        B_p (batch, nx, nu), f_p (batch, nx) or None; 2-D A_p, B_p: one plant for all (stored once).  A_p None removes it"""
        if A_p is None:
            return self._check(lib().tiny_batch_set_plant(self._h, None, None, None, HOST), "set_plant")
        if B_p is None:
            raise ValueError("plant: A_p without B_p")
        A, Bm, f, bc = self._plant(A_p, B_p, f_p)
        self._check(lib().tiny_batch_set_plant(self._h, A.ctypes.data_as(C.c_void_p), Bm.ctypes.data_as(C.c_void_p),
                                               None if f is None else f.ctypes.data_as(C.c_void_p), HOST | bc), "set_plant")

    def set_plant_device(self, A_p, B_p, f_p=None, broadcast=False):
        """the same from device pointers (ints) to column-major [batch][nx*nx], [batch][nx*nu], [batch][nx] doubles (one of each with
        broadcast) resident in HBM (copied)"""
        self._check(lib().tiny_batch_set_plant(self._h, C.c_void_p(int(A_p)), C.c_void_p(int(B_p)), None if f_p is None else C.c_void_p(int(f_p)),
                                               DEVICE | (BROADCAST if broadcast else 0)), "set_plant_device")

    def get_plant(self, i):
        """(A_p (nx, nx), B_p (nx, nu), f_p (nx,)) instance i is stepped by, as installed"""
        A, Bm, f = np.zeros(self.nx * self.nx), np.zeros(self.nx * self.nu), np.zeros(self.nx)
        self._check(lib().tiny_batch_get_plant(self._h, int(i), A.ctypes.data_as(_dp), Bm.ctypes.data_as(_dp), f.ctypes.data_as(_dp)), "get_plant")
        return A.reshape(self.nx, self.nx).T.copy(), Bm.reshape(self.nu, self.nx).T.copy(), f

    def state_log(self, steps):
        """x0_next[steps, batch, nx]: the state every MPC step of the last solve call handed on (option "state_log" = 1)"""
        out = np.zeros((steps, self.batch, self.nx))
        self._check(lib().tiny_batch_get_state_log(self._h, out.ctypes.data_as(_dp), int(steps)), "get_state_log")
        return out

    def _gain(self, M):
        """M (batch, nx, nx) | (nx, nx) -> (flat column-major array, broadcast flag)"""
        G = np.asarray(M, dtype=np.float64)
        one = G.ndim == 2
        if one:
            G = G[None]
        n = 1 if one else self.batch
        if G.shape != (n, self.nx, self.nx):
            raise ValueError(f"estimator: M ({n}, {self.nx}, {self.nx}), got {G.shape}")
        return np.ascontiguousarray(G.transpose(0, 2, 1)).ravel(), (BROADCAST if one else 0)

    def _estimate(self, xp):
        """xp (batch, nx) | (nx,) -> (flat array, broadcast flag)"""
        x = _f64(xp)
        if x.shape not in ((self.batch, self.nx), (self.nx,)):
            raise ValueError(f"estimate: ({self.batch}, {self.nx}) or ({self.nx},), got {x.shape}")
        return x.ravel(), (BROADCAST if x.ndim == 1 else 0)

    def set_estimator(self, M):
        """a fixed-gain state estimator in a closed loop (advance_x0, steps_per_launch > 1): x0 is the plant's true state, MPC step k
        solves from xhat = xp + M (xm - xp), xm the (noisy) measurement, and the model predicts the next xp from xhat and u0.  M (batch,
        nx, nx), or (nx, nx) for one gain for all (M = L C: a Luenberger observer, a steady-state Kalman filter); None removes it.
        Installing one where none is installed starts the estimate at x0; replacing the gain keeps it"""
        if M is None:
            return self._check(lib().tiny_batch_set_estimator(self._h, None, HOST), "set_estimator")
        flat, bc = self._gain(M)
        self._check(lib().tiny_batch_set_estimator(self._h, flat.ctypes.data_as(C.c_void_p), HOST | bc), "set_estimator")

    def set_estimator_device(self, M, broadcast=False):
        """the same from a device pointer (int) to column-major [batch][nx*nx] doubles (one with broadcast) resident in HBM (copied)"""
        self._check(lib().tiny_batch_set_estimator(self._h, C.c_void_p(int(M)), DEVICE | (BROADCAST if broadcast else 0)), "set_estimator_device")

    def get_estimator(self, i):
        """M (nx, nx) instance i is corrected by, as installed"""
        out = np.zeros(self.nx * self.nx)
        self._check(lib().tiny_batch_get_estimator(self._h, int(i), out.ctypes.data_as(_dp)), "get_estimator")
        return out.reshape(self.nx, self.nx).T.copy()

    def set_estimate(self, xp):
        """the predicted estimate: xp (batch, nx), or (nx,) for all"""
        flat, bc = self._estimate(xp)
        self._check(lib().tiny_batch_set_estimate(self._h, flat.ctypes.data_as(C.c_void_p), HOST | bc), "set_estimate")

    def get_estimate(self):
        """xp (batch, nx): the predicted estimate the next MPC step corrects"""
        out = np.zeros((self.batch, self.nx))
        self._check(lib().tiny_batch_get_estimate(self._h, out.ctypes.data_as(_dp)), "get_estimate")
        return out

    def estimate_log(self, steps):
        """xhat[steps, batch, nx]: the estimate every MPC step of the last solve call solved from (option "estimate_log" = 1)"""
        out = np.zeros((steps, self.batch, self.nx))
        self._check(lib().tiny_batch_get_estimate_log(self._h, out.ctypes.data_as(_dp), int(steps)), "get_estimate_log")
        return out

    def _score(self, weight, target, lo, hi):
        """four arrays over z = [x | u], (batch, nx+nu) | (nx+nu,) each (target, lo, hi may be None) -> (flat arrays or None, broadcast flag)"""
        nz = self.nx + self.nu
        w = _f64(weight)
        if w.shape not in ((self.batch, nz), (nz,)):
            raise ValueError(f"score: weight ({self.batch}, {nz}) or ({nz},), got {w.shape}")
        out = [w.ravel()]
        for name, a in (("target", target), ("lo", lo), ("hi", hi)):
            if a is None:
                out.append(None)
                continue
            v = _f64(a)
            if v.shape != w.shape:
                raise ValueError(f"score: {name} {w.shape} like weight, got {v.shape}")
            out.append(v.ravel())
        return out, (BROADCAST if w.ndim == 1 else 0)

    def set_score(self, weight, target=None, lo=None, hi=None):
        """a per-instance score of a closed loop (advance_x0, steps_per_launch > 1), accumulated on the device at every plant step: over
        z = [xn | u0] (the state handed on, what state_log records, and the applied control) cost += (weight * (z - target)) * (z - target)
        term by term in ascending order, and the largest violation of lo <= z <= hi with the steps that violated and the first of them.
        Each array (batch, nx+nu), or (nx+nu,) for one setup for all; target None: zeros, lo / hi None: no limit; weight None removes
        it.  Installing or replacing zeroes the record and rewinds the counter (option "score_step")"""
        if weight is None:
            return self._check(lib().tiny_batch_set_score(self._h, None, None, None, None, HOST), "set_score")
        a, bc = self._score(weight, target, lo, hi)
        p = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in a]
        self._check(lib().tiny_batch_set_score(self._h, p[0], p[1], p[2], p[3], HOST | bc), "set_score")

    def set_score_device(self, weight, target=None, lo=None, hi=None, broadcast=False):
        """the same from device pointers (int; None where an array is left out) to [batch][nx+nu] doubles (one row with broadcast) resident in HBM (copied)"""
        p = [None if v is None else C.c_void_p(int(v)) for v in (weight, target, lo, hi)]
        self._check(lib().tiny_batch_set_score(self._h, p[0], p[1], p[2], p[3], DEVICE | (BROADCAST if broadcast else 0)), "set_score_device")

    def get_score_setup(self, i):
        """(weight, target, lo, hi), (nx+nu,) each: what instance i is scored by, as installed"""
        out = [np.zeros(self.nx + self.nu) for _ in range(4)]
        self._check(lib().tiny_batch_get_score_setup(self._h, int(i), *[v.ctypes.data_as(_dp) for v in out]), "get_score_setup")
        return tuple(out)

    def get_score(self):
        """(cost, worst, violated_steps, first_violation), (batch,) each: the record as it stands"""
        cost, worst = np.zeros(self.batch), np.zeros(self.batch)
        steps, first = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
        self._check(lib().tiny_batch_get_score(self._h, cost.ctypes.data_as(_dp), worst.ctypes.data_as(_dp), steps.ctypes.data_as(C.POINTER(C.c_int)),
                                               first.ctypes.data_as(C.POINTER(C.c_int))), "get_score")
        return cost, worst, steps, first

    def reset_score(self):
        """zeroes the record and rewinds the counter; the setup stays"""
        self._check(lib().tiny_batch_reset_score(self._h), "reset_score")

    def _actuator(self, lo, hi, alpha, gain, offset):
        """five arrays over the inputs, (batch, nu) | (nu,) each or None -> (flat arrays or None, broadcast flag)"""
        shape, out = None, []
        for name, a in (("lo", lo), ("hi", hi), ("alpha", alpha), ("gain", gain), ("offset", offset)):
            if a is None:
                out.append(None)
                continue
            v = _f64(a)
            if v.shape not in ((self.batch, self.nu), (self.nu,)) or (shape is not None and v.shape != shape):
                raise ValueError(f"actuator: {name} ({self.batch}, {self.nu}) or ({self.nu},), all alike, got {v.shape}")
            shape = v.shape
            out.append(v.ravel())
        return out, (BROADCAST if shape is not None and len(shape) == 1 else 0)

    def set_actuator(self, lo=None, hi=None, alpha=None, gain=None, offset=None):
        """an actuator model between the command and the plant step of a closed loop (advance_x0, steps_per_launch > 1): per input the
        applied control is the command limited to [lo, hi], lagged (a += alpha * (s - a), one fma; a: actuator_state), scaled and offset
        (fma(m, gain, offset)) and, with set_actuation_noise, disturbed.  It replaces u0 at the plant step and in the score, nowhere
        else.  Each array (batch, nu), or (nu,) for one setup for all, or None (the stage is absent); all None removes it"""
        a, bc = self._actuator(lo, hi, alpha, gain, offset)
        p = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in a]
        self._check(lib().tiny_batch_set_actuator(self._h, p[0], p[1], p[2], p[3], p[4], HOST | bc), "set_actuator")

    def set_actuator_device(self, lo=None, hi=None, alpha=None, gain=None, offset=None, broadcast=False):
        """the same from device pointers (int; None where an array is left out) to [batch][nu] doubles (one row with broadcast) resident in HBM (copied)"""
        p = [None if v is None else C.c_void_p(int(v)) for v in (lo, hi, alpha, gain, offset)]
        self._check(lib().tiny_batch_set_actuator(self._h, p[0], p[1], p[2], p[3], p[4], DEVICE | (BROADCAST if broadcast else 0)), "set_actuator_device")

    def get_actuator(self, i):
        """(lo, hi, alpha, gain, offset), (nu,) each: what instance i is actuated by, as installed, defaults filled in"""
        out = [np.zeros(self.nu) for _ in range(5)]
        self._check(lib().tiny_batch_get_actuator(self._h, int(i), *[v.ctypes.data_as(_dp) for v in out]), "get_actuator")
        return tuple(out)

    def set_actuator_state(self, a):
        """the lag's record a: (batch, nu), or (nu,) for all"""
        v = _f64(a)
        if v.shape not in ((self.batch, self.nu), (self.nu,)):
            raise ValueError(f"actuator state: ({self.batch}, {self.nu}) or ({self.nu},), got {v.shape}")
        self._check(lib().tiny_batch_set_actuator_state(self._h, v.ctypes.data_as(C.c_void_p), HOST | (BROADCAST if v.ndim == 1 else 0)), "set_actuator_state")

    def set_actuator_state_device(self, a, broadcast=False):
        self._check(lib().tiny_batch_set_actuator_state(self._h, C.c_void_p(int(a)), DEVICE | (BROADCAST if broadcast else 0)), "set_actuator_state_device")

    def get_actuator_state(self):
        """a (batch, nu) as it stands"""
        out = np.zeros((self.batch, self.nu))
        self._check(lib().tiny_batch_get_actuator_state(self._h, out.ctypes.data_as(_dp)), "get_actuator_state")
        return out

    def _actuator_delay(self, d, d_max):
        """d: (batch,) ints or one int for all; d_max: None -> the largest d -> (int32 array, d_max, broadcast flag)"""
        v = np.asarray(d, dtype=np.int32)
        if v.shape not in ((self.batch,), ()):
            raise ValueError(f"actuator delay: ({self.batch},) or one int, got {v.shape}")
        bc = BROADCAST if v.ndim == 0 else 0
        v = np.ascontiguousarray(v.reshape(-1))
        return v, (int(v.max()) if d_max is None else int(d_max)), bc

    def set_actuator_delay(self, d=None, d_max=None):
        """stage 0 of the actuator, a transport delay: the command of MPC step k reaches the limits d[i] steps later (a FIFO of the
        instance's last d[i] commands, zeroed here).  d: (batch,) ints or one int for all, 0 <= d <= d_max <= MAX_DELAY; d_max None: the
        largest d; d None removes the delay.  Option "delay_compensation" = 1 lets every step solve from the model's prediction over the
        queue"""
        if d is None:
            return self._check(lib().tiny_batch_set_actuator_delay(self._h, None, 0, HOST), "set_actuator_delay")
        v, dm, bc = self._actuator_delay(d, d_max)
        self._check(lib().tiny_batch_set_actuator_delay(self._h, v.ctypes.data_as(C.c_void_p), dm, HOST | bc), "set_actuator_delay")

    def set_actuator_delay_device(self, d, d_max, broadcast=False):
        """set_actuator_delay from a device pointer to (batch,) ints (one with broadcast)"""
        self._check(lib().tiny_batch_set_actuator_delay(self._h, C.c_void_p(int(d)), int(d_max), DEVICE | (BROADCAST if broadcast else 0)), "set_actuator_delay_device")

    def get_actuator_delay(self, i):
        """d of instance i, as installed"""
        out = C.c_int(0)
        self._check(lib().tiny_batch_get_actuator_delay(self._h, int(i), C.byref(out)), "get_actuator_delay")
        return int(out.value)

    def _delay_max(self):
        return int(self.get_option("actuator_delay"))

    def _actuator_queue(self, q):
        d_max = self._delay_max()
        v = _f64(q)
        if v.shape not in ((self.batch, d_max, self.nu), (d_max, self.nu)):
            raise ValueError(f"actuator queue: ({self.batch}, {d_max}, {self.nu}) or ({d_max}, {self.nu}), got {v.shape}")
        return v, (BROADCAST if v.ndim == 2 else 0)

    def set_actuator_queue(self, q):
        """the delay's queue, oldest first: (batch, d_max, nu), or (d_max, nu) for all; only the first d[i] rows of an instance count"""
        v, bc = self._actuator_queue(q)
        self._check(lib().tiny_batch_set_actuator_queue(self._h, v.ctypes.data_as(C.c_void_p), HOST | bc), "set_actuator_queue")

    def set_actuator_queue_device(self, q, broadcast=False):
        self._check(lib().tiny_batch_set_actuator_queue(self._h, C.c_void_p(int(q)), DEVICE | (BROADCAST if broadcast else 0)), "set_actuator_queue_device")

    def get_actuator_queue(self):
        """(batch, d_max, nu) as it stands, oldest first, +0.0 behind an instance's first d[i] rows"""
        out = np.zeros((self.batch, max(self._delay_max(), 1), self.nu))
        self._check(lib().tiny_batch_get_actuator_queue(self._h, out.ctypes.data_as(_dp)), "get_actuator_queue")
        return out

    def _actuation_noise(self, n):
        """(n_steps, batch, nu), or (n_steps, nu) for one sequence for all -> (flat array, n_steps, broadcast flag)"""
        n = np.ascontiguousarray(n, dtype=np.float64)
        if n.ndim == 2 and n.shape[1] == self.nu and n.shape[0] > 0:
            return n.ravel(), n.shape[0], BROADCAST
        if n.ndim != 3 or n.shape[0] == 0 or n.shape[1:] != (self.batch, self.nu):
            raise ValueError(f"actuation noise: (n_steps, {self.batch}, {self.nu}) or (n_steps, {self.nu}), got {n.shape}")
        return n.ravel(), n.shape[0], 0

    def set_actuation_noise(self, n):
        """the noise of the actuator's last stage: the applied control of MPC step k takes + n[k, i].  n: (n_steps, batch, nu), or
        (n_steps, nu) for one sequence for all; None removes it.  The counter (option "actuation_step") starts at 0; steps outside n add
        nothing.  Allowed with no actuator installed"""
        if n is None:
            return self._check(lib().tiny_batch_set_actuation_noise(self._h, None, 0, HOST), "set_actuation_noise")
        flat, k, bc = self._actuation_noise(n)
        self._check(lib().tiny_batch_set_actuation_noise(self._h, flat.ctypes.data_as(C.c_void_p), k, HOST | bc), "set_actuation_noise")

    def set_actuation_noise_device(self, n, n_steps, broadcast=False):
        """the same from a device pointer (int) to [n_steps][batch][nu] doubles ([n_steps][nu] with broadcast) resident in HBM (copied)"""
        self._check(lib().tiny_batch_set_actuation_noise(self._h, C.c_void_p(int(n)), int(n_steps), DEVICE | (BROADCAST if broadcast else 0)),
                    "set_actuation_noise_device")

    def get_actuation_noise(self, step, i):
        """n[step, i] (nu,) as installed"""
        out = np.zeros(self.nu)
        self._check(lib().tiny_batch_get_actuation_noise(self._h, int(step), int(i), out.ctypes.data_as(_dp)), "get_actuation_noise")
        return out

    def generate_actuation_noise(self, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
        """generate_disturbance's twin for the actuation noise (stream 2, rows of nu entries: scale (nu,) | (batch, nu), ...)"""
        spec, keep = noise_spec(self.batch, self.nu, seed, n_steps, scale, mean, factor, id_base, id_stride)
        self._check(lib().tiny_batch_generate_actuation_noise(self._h, C.byref(spec)), "generate_actuation_noise")

    def actuation_log(self, steps):
        """ua[steps, batch, nu]: the control every plant step of the last solve call received (option "actuation_log" = 1)"""
        out = np.zeros((steps, self.batch, self.nu))
        self._check(lib().tiny_batch_get_actuation_log(self._h, out.ctypes.data_as(_dp), int(steps)), "get_actuation_log")
        return out

    def set_linear_constraints(self, Alin_x, blin_x, Alin_u, blin_u):
        """Half-spaces a_k' z <= b_k (tiny_set_linear_constraints): Alin_x (n_s, nx), blin_x (n_s,), Alin_u (n_i, nu)."""
        Ax = np.asarray(Alin_x, dtype=np.float64).reshape(-1, self.nx)
        Au = np.asarray(Alin_u, dtype=np.float64).reshape(-1, self.nu)
        a = [np.ascontiguousarray(Ax.T).ravel(), _f64(blin_x).ravel(), np.ascontiguousarray(Au.T).ravel(), _f64(blin_u).ravel()]
        self._check(lib().tiny_batch_set_linear_constraints(self._h, Ax.shape[0], a[0].ctypes.data_as(_dp), a[1].ctypes.data_as(_dp),
                                                            Au.shape[0], a[2].ctypes.data_as(_dp), a[3].ctypes.data_as(_dp)),
                    "set_linear_constraints")

    def set_tv_linear_constraints(self, tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u):
        """tiny_set_tv_linear_constraints: tv_Alin_x (n_s*N, nx) [row n_s*i+k = constraint k at knot i], tv_blin_x (n_s, N),
        tv_Alin_u (n_i*(N-1), nu), tv_blin_u (n_i, N-1)."""
        Ax = np.asarray(tv_Alin_x, dtype=np.float64).reshape(-1, self.nx)
        Au = np.asarray(tv_Alin_u, dtype=np.float64).reshape(-1, self.nu)
        bx = np.asarray(tv_blin_x, dtype=np.float64).reshape(-1, self.N)
        bu = np.asarray(tv_blin_u, dtype=np.float64).reshape(-1, self.N - 1)
        a = [np.ascontiguousarray(Ax.T).ravel(), np.ascontiguousarray(bx.T).ravel(), np.ascontiguousarray(Au.T).ravel(),
             np.ascontiguousarray(bu.T).ravel()]
        self._check(lib().tiny_batch_set_tv_linear_constraints(self._h, bx.shape[0], a[0].ctypes.data_as(_dp), a[1].ctypes.data_as(_dp),
                                                               bu.shape[0], a[2].ctypes.data_as(_dp), a[3].ctypes.data_as(_dp)),
                    "set_tv_linear_constraints")

    def _instance_halfspaces(self, tv, A_x, b_x, A_u, b_u):
        """[batch, rows, n] coefficients (None: keep them, the offsets-only update), [batch, n_s(, knots)] offsets -> (n_s, n_i, the four
        flat arrays with a leading batch axis, per instance column-major as the shared setter takes them; None stays None)"""
        ks, ki = (self.N, self.N - 1) if tv else (1, 1)
        bx = np.asarray(b_x, dtype=np.float64).reshape(self.batch, -1, ks)
        bu = np.asarray(b_u, dtype=np.float64).reshape(self.batch, -1, ki)
        ns, ni = bx.shape[1], bu.shape[1]
        col = lambda v, rows, n: None if v is None else np.ascontiguousarray(
            np.asarray(v, dtype=np.float64).reshape(self.batch, rows, n).transpose(0, 2, 1)).ravel()
        return ns, ni, [col(A_x, ns * ks, self.nx), np.ascontiguousarray(bx.transpose(0, 2, 1)).ravel(),
                        col(A_u, ni * ki, self.nu), np.ascontiguousarray(bu.transpose(0, 2, 1)).ravel()]

    def _set_instance_halfspaces(self, tv, A_x, b_x, A_u, b_u, what):
        ns, ni, a = self._instance_halfspaces(tv, A_x, b_x, A_u, b_u)
        p = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in a]
        f = lib().tiny_batch_set_instance_tv_linear_constraints if tv else lib().tiny_batch_set_instance_linear_constraints
        self._check(f(self._h, ns, p[0], p[1], ni, p[2], p[3], HOST), what)

    def set_instance_linear_constraints(self, Alin_x, blin_x, Alin_u, blin_u):
        """every instance its own static half-spaces: Alin_x [batch, n_s, nx], blin_x [batch, n_s], Alin_u [batch, n_i, nu], blin_u
        [batch, n_i].  Alin_x / Alin_u = None: keep the installed coefficients, rewrite the offsets only."""
        self._set_instance_halfspaces(0, Alin_x, blin_x, Alin_u, blin_u, "set_instance_linear_constraints")

    def set_instance_tv_linear_constraints(self, tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u):
        """every instance its own time-varying half-spaces: tv_Alin_x [batch, n_s*N, nx] (row n_s*i+k = constraint k at knot i), tv_blin_x
        [batch, n_s, N], tv_Alin_u [batch, n_i*(N-1), nu], tv_blin_u [batch, n_i, N-1].  None coefficients: the offsets-only update."""
        self._set_instance_halfspaces(1, tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u, "set_instance_tv_linear_constraints")

    def set_instance_linear_constraints_device(self, n_state, Alin_x, blin_x, n_input, Alin_u, blin_u):
        """the same from device pointers (ints; 0: none) to the arrays in the C layout, resident in HBM (copied)"""
        p = [C.c_void_p(int(v)) if v else None for v in (Alin_x, blin_x, Alin_u, blin_u)]
        self._check(lib().tiny_batch_set_instance_linear_constraints(self._h, int(n_state), p[0], p[1], int(n_input), p[2], p[3], DEVICE),
                    "set_instance_linear_constraints_device")

    def set_instance_tv_linear_constraints_device(self, n_state, tv_Alin_x, tv_blin_x, n_input, tv_Alin_u, tv_blin_u):
        p = [C.c_void_p(int(v)) if v else None for v in (tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u)]
        self._check(lib().tiny_batch_set_instance_tv_linear_constraints(self._h, int(n_state), p[0], p[1], int(n_input), p[2], p[3], DEVICE),
                    "set_instance_tv_linear_constraints_device")

    def instance_linear_constraints(self, i, tv=0):
        """(A_x, b_x, A_u, b_u) instance i is held to by the static (tv = 0) or time-varying (tv = 1) set, as set, in the shapes the
        shared setters take; on a shared set: the shared one"""
        ns = self.get_option("n_tv_state_linear" if tv else "n_state_linear")
        ni = self.get_option("n_tv_input_linear" if tv else "n_input_linear")
        ks, ki = (self.N, self.N - 1) if tv else (1, 1)
        out = [np.zeros((self.nx, ns * ks)), np.zeros((ks, ns)), np.zeros((self.nu, ni * ki)), np.zeros((ki, ni))]
        self._check(lib().tiny_batch_get_instance_linear_constraints(self._h, int(i), int(tv), *[v.ctypes.data_as(_dp) for v in out]),
                    "instance_linear_constraints")
        Ax, bx, Au, bu = (v.T.copy() for v in out)
        return (Ax, bx, Au, bu) if tv else (Ax, bx.ravel(), Au, bu.ravel())

    def update_settings(self, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=1000, check_termination=1,
                        en_state_bound=1, en_input_bound=1, en_state_soc=0, en_input_soc=0, en_state_linear=0,
                        en_input_linear=0, en_tv_state_linear=0, en_tv_input_linear=0):
        self._check(lib().tiny_batch_update_settings(
            self._h, abs_pri_tol, abs_dua_tol, int(max_iter), int(check_termination), int(en_state_bound),
            int(en_input_bound), int(en_state_soc), int(en_input_soc), int(en_state_linear), int(en_input_linear),
            int(en_tv_state_linear), int(en_tv_input_linear)), "update_settings")

    def cache(self, name):
        shapes = {"Kinf": (self.nu, self.nx), "Pinf": (self.nx, self.nx), "Quu_inv": (self.nu, self.nu),
                  "AmBKt": (self.nx, self.nx), "APf": (self.nx, 1), "BPf": (self.nu, 1), "Q": (self.nx, 1),
                  "R": (self.nu, 1)}
        r, c = shapes[name]
        out = np.zeros(r * c)
        n = lib().tiny_batch_get_cache(self._h, name.encode(), out.ctypes.data_as(_dp), r * c)
        assert n == r * c
        return out.reshape((r, c), order="F")

    # ---- per-instance data
    def _shape(self, name):
        if name == "x0":
            return (self.nx, 1)
        return (self.nx, self.N) if name in STATE_FIELDS else (self.nu, self.N - 1)

    def set(self, name, value, broadcast=False):
        """value: [batch, rows, cols] (or [rows, cols] with broadcast=True); x0: [batch, nx]."""
        r, c = self._shape(name)
        a = np.asarray(value, dtype=np.float64)
        if broadcast:
            flat = np.ascontiguousarray(a.reshape(r, c).T).ravel()
        else:
            flat = np.ascontiguousarray(a.reshape(self.batch, r, c).transpose(0, 2, 1)).ravel()
        self._check(lib().tiny_batch_set(self._h, FIELD_ID[name], flat.ctypes.data_as(C.c_void_p),
                                         HOST | (BROADCAST if broadcast else 0)), f"set({name})")

    def get(self, name):
        r, c = self._shape(name)
        out = np.zeros((self.batch, c, r))
        self._check(lib().tiny_batch_get(self._h, FIELD_ID[name], out.ctypes.data_as(C.c_void_p), HOST), f"get({name})")
        out = out.transpose(0, 2, 1)
        return out[:, :, 0] if name == "x0" else out

    def set_device(self, name, ptr, broadcast=False):
        """ptr: device pointer (int) to [batch][cols][rows] doubles already resident in HBM."""
        self._check(lib().tiny_batch_set(self._h, FIELD_ID[name], C.c_void_p(ptr),
                                         DEVICE | (BROADCAST if broadcast else 0)), f"set_device({name})")

    def set_x0(self, x0, broadcast=False):          # tiny_set_x0
        self.set("x0", x0, broadcast)

    def set_x_ref(self, x_ref, broadcast=False):    # tiny_set_x_ref
        self.set("Xref", x_ref, broadcast)

    def set_u_ref(self, u_ref, broadcast=False):    # tiny_set_u_ref
        self.set("Uref", u_ref, broadcast)

    def reset(self):
        self._check(lib().tiny_batch_reset(self._h), "reset")

    # ---- hot path
    def solve(self) -> int:
        rc = lib().tiny_batch_solve(self._h)
        if rc not in (0, 1):
            self._check(rc, "solve")
        return rc

    def solve_async(self):
        self._check(lib().tiny_batch_solve_async(self._h), "solve_async")

    def phase(self, name):
        """ONE phase of the iteration over the batch (the reference's exported phase functions, admm.hpp:12-17), on
        the device records as they are.  'termination_condition' returns the per-instance booleans."""
        self._check(lib().tiny_batch_phase(self._h, PHASES[name]), name)
        if name == "termination_condition":
            return self.status()["solved"].astype(bool)

    def synchronize(self):
        self._check(lib().tiny_batch_synchronize(self._h), "synchronize")

    def status(self):
        B = self.batch
        it, so, st = (np.zeros(B, dtype=np.int32) for _ in range(3))
        res = np.zeros((B, 4))
        self._check(lib().tiny_batch_get_status(self._h, it.ctypes.data_as(_ip), so.ctypes.data_as(_ip),
                                                st.ctypes.data_as(_ip), res.ctypes.data_as(_dp)), "get_status")
        return dict(iter=it, solved=so, status=st, primal_residual_state=res[:, 0], primal_residual_input=res[:, 1],
                    dual_residual_state=res[:, 2], dual_residual_input=res[:, 3])

    def reduce_stats(self, device_out=None):
        """[sum_iter, sum_solved, batch, max residual x4, accumulated iters, accumulated solved, 0];
        device_out: optional device pointer (int) receiving the same 10 doubles (e.g. the buffer of an
        RCCL all-reduce)."""
        out = np.zeros(10)
        self._check(lib().tiny_batch_reduce_stats(self._h, out.ctypes.data_as(_dp),
                                                  C.c_void_p(device_out) if device_out else None), "reduce_stats")
        return out

    def reduce_stats_async(self, device_out):
        self._check(lib().tiny_batch_reduce_stats(self._h, None, C.c_void_p(device_out)), "reduce_stats")

    # ---- adaptive rho (types.hpp:75-79; admm.cpp:397-423; rho_benchmark.cpp)
    def set_adaptive_rho(self, enable=1, rho_min=1.0, rho_max=100.0, clip=1):
        self._check(lib().tiny_batch_set_adaptive_rho(self._h, int(enable), float(rho_min), float(rho_max), int(clip)), "set_adaptive_rho")

    def set_sensitivity(self, dKinf, dPinf, dC1=None, dC2=None):
        """(rows, cols) arrays: dKinf_drho (nu, nx), dPinf_drho (nx, nx), dC1_drho (nu, nu), dC2_drho (nx, nx)"""
        nx, nu = self.nx, self.nu
        a = [_colmajor(dKinf, (nu, nx)), _colmajor(dPinf, (nx, nx)), None if dC1 is None else _colmajor(dC1, (nu, nu)),
             None if dC2 is None else _colmajor(dC2, (nx, nx))]
        self._check(lib().tiny_batch_set_sensitivity(self._h, *[None if v is None else v.ctypes.data_as(_dp) for v in a]), "set_sensitivity")

    _SENS_SHAPES = {"dKinf_drho": lambda s: (s.nu, s.nx), "dPinf_drho": lambda s: (s.nx, s.nx), "dC1_drho": lambda s: (s.nu, s.nu),
                    "dC2_drho": lambda s: (s.nx, s.nx), "steps": lambda s: (1, 1)}

    def compute_sensitivity(self):
        """the four d(.)/d(rho) tables of this batch's own system(s), computed on the GPU (csrc/sensitivity_kernel.hip.h): the
        derivative of tiny_setup's cache at the cache as it stands; a per-instance batch gets every instance's own"""
        self._check(lib().tiny_batch_compute_sensitivity(self._h), "compute_sensitivity")

    def sensitivity(self, name):
        """what is installed, computed or set: 'dKinf_drho' (nu, nx), 'dPinf_drho' (nx, nx), 'dC1_drho' (nu, nu), 'dC2_drho' (nx, nx)"""
        r, c = self._SENS_SHAPES[name](self)
        out = np.zeros(r * c)
        n = lib().tiny_batch_get_sensitivity(self._h, name.encode(), out.ctypes.data_as(_dp), r * c)
        if n != r * c:
            self._check(n if n < 0 else ERR_ARG, f"sensitivity({name})")
        return out.reshape((r, c), order="F")

    def sensitivity_instance(self, instance, name):
        """... of one instance of a per-instance batch; also 'steps': the squarings its Lyapunov solve took"""
        r, c = self._SENS_SHAPES[name](self)
        out = np.zeros(r * c)
        n = lib().tiny_batch_get_sensitivity_instance(self._h, int(instance), name.encode(), out.ctypes.data_as(_dp), r * c)
        if n != r * c:
            self._check(n if n < 0 else ERR_ARG, f"sensitivity_instance({name})")
        return int(out[0]) if name == "steps" else out.reshape((r, c), order="F")

    _CACHE_SHAPES = {"rho": lambda s: (1, 1), "Kinf": lambda s: (s.nu, s.nx), "Pinf": lambda s: (s.nx, s.nx),
                     "C1": lambda s: (s.nu, s.nu), "C2": lambda s: (s.nx, s.nx)}

    def set_cache_state(self, which, value):
        """per-instance cache state of an adaptive batch: value [batch] for 'rho', [batch, rows, cols] otherwise"""
        r, c = self._CACHE_SHAPES[which](self)
        a = np.asarray(value, dtype=np.float64).reshape(self.batch, r, c)
        flat = np.ascontiguousarray(a.transpose(0, 2, 1)).ravel()
        self._check(lib().tiny_batch_set_cache_state(self._h, which.encode(), flat.ctypes.data_as(_dp)), f"set_cache_state({which})")

    def get_cache_state(self, which):
        r, c = self._CACHE_SHAPES[which](self)
        out = np.zeros((self.batch, c, r))
        self._check(lib().tiny_batch_get_cache_state(self._h, which.encode(), out.ctypes.data_as(_dp)), f"get_cache_state({which})")
        out = out.transpose(0, 2, 1)
        return out[:, 0, 0] if which == "rho" else out

    def allreduce_stats(self, comm, n_ranks, rank, total_batch):
        """the path's one exchange on an RCCL communicator the caller owns (tiny_batch_allreduce_stats); returns the
        job-wide 10-entry statistics vector (the same on every rank)"""
        out = np.zeros(10)
        self._check(lib().tiny_batch_allreduce_stats(self._h, C.c_void_p(comm), int(n_ranks), int(rank), int(total_batch),
                                                     out.ctypes.data_as(_dp)), "allreduce_stats")
        return out

    def get_option(self, name) -> int:
        return int(lib().tiny_batch_get_option(self._h, name.encode()))

    def get_plan(self) -> bytes:
        """the settled launch form of this batch (TinyBatchPlan, include/tinympc_amd.h) as bytes: write them to a file, hand them
        to set_plan of another handle of the same (nx, nu, N) -- it takes the settled form on its first solve"""
        buf = C.create_string_buffer(PLAN_BYTES)
        self._check(lib().tiny_batch_get_plan(self._h, buf), "get_plan")
        return buf.raw

    def set_plan(self, plan: bytes):
        if len(plan) != PLAN_BYTES:
            raise TinyMPCError("set_plan: %d bytes, a TinyBatchPlan has %d" % (len(plan), PLAN_BYTES))
        self._check(lib().tiny_batch_set_plan(self._h, C.create_string_buffer(bytes(plan), PLAN_BYTES)), "set_plan")

    @staticmethod
    def plan_fields(plan: bytes) -> dict:
        """the scalar fields of a TinyBatchPlan (diagnostics, tests)"""
        import struct
        names = ("magic version bytes nx nu N batch max_iter check_termination open_questions auto_verdict auto_cap auto_cap_max_iter "
                 "auto_growth growth_verdict auto_probes tile_verdict regroup_verdict hist_valid").split()
        ints = struct.unpack_from("<%di" % len(names), plan, 0)
        off = (4 * len(names) + 7) // 8 * 8
        dbl = struct.unpack_from("<5d", plan, off)
        d = dict(zip(names, ints))
        d.update(zip(("auto_plain_rate", "auto_split_rate", "auto_gain", "tile_rate", "lockstep_ratio"), dbl))
        return d

    def stats_message_async(self, device_out):
        """the batch's 64-byte statistics message (8 doubles) -> device memory, on the batch's stream behind the solve"""
        self._check(lib().tiny_batch_stats_message(self._h, C.c_void_p(device_out)), "stats_message")

    def set_option(self, name, value):
        self._check(lib().tiny_batch_set_option(self._h, name.encode(), int(value)), f"set_option({name})")

    def set_stream(self, stream_ptr):
        self._check(lib().tiny_batch_set_stream(self._h, C.c_void_p(stream_ptr)), "set_stream")

    def timing_ms(self, capacity=4096):
        buf = np.zeros(capacity, dtype=np.float32)
        n = lib().tiny_batch_get_timing(self._h, buf.ctypes.data_as(_fp), capacity)
        return buf[:max(n, 0)].astype(np.float64)

    def set_reference_trajectory(self, xref_points, offsets=None):
        """xref_points: [n_points, nx] shared state-reference trajectory; the solve at MPC step k tracks the window
        k + offsets[b] ... + N - 1 (examples/quadrotor_tracking.cpp).  None removes it."""
        if xref_points is None:
            self._check(lib().tiny_batch_set_reference_trajectory(self._h, None, 0, None, HOST), "set_reference_trajectory")
            return
        t = _f64(xref_points).reshape(-1, self.nx)
        off = None if offsets is None else np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).ravel())
        self._check(lib().tiny_batch_set_reference_trajectory(
            self._h, t.ctypes.data_as(_dp), t.shape[0], None if off is None else off.ctypes.data_as(_ip), HOST),
            "set_reference_trajectory")

    def step_log(self, steps):
        """(iters[steps, batch] (negative: hit max_iter), u0[steps, batch, nu]) of the last fused launch."""
        it = np.zeros((steps, self.batch), dtype=np.int32)
        u0 = np.zeros((steps, self.batch, self.nu))
        self._check(lib().tiny_batch_get_step_log(self._h, it.ctypes.data_as(_ip), u0.ctypes.data_as(_dp), steps),
                    "get_step_log")
        return it, u0

    def kernel_path(self) -> str:
        return {0: "regs", 1: "tile", 2: "cover", 3: "jit", 4: "tile-jit"}[lib().tiny_batch_kernel_path(self._h)]

    def algorithmic_bytes(self, cold=False) -> int:
        """cold: False / 0 bytes_warm, True / 1 bytes_cold (one_shot = 2), 2 the traffic of one_shot = 1."""
        return int(lib().tiny_batch_algorithmic_bytes(self._h, int(cold)))


class TinyGroupSolver:
    """ctypes mirror of TinyGroup (include/tinympc_amd.h section C): ONE host process, the batch sharded over several
    GPUs (contiguous blocks or round-robin), one RCCL all-gather of 64-byte statistics messages as the only exchange.
    Per-instance arrays carry the FULL batch axis in the caller's order."""

    def __init__(self, A, B, f, Q, R, rho, nx, nu, N, batch, devices=None, n_shards=0, interleaved=False, verbose=0):
        self._h = C.c_void_p()
        self.nx, self.nu, self.N, self.batch = int(nx), int(nu), int(N), int(batch)
        A = _colmajor(A, (nx, nx))
        Bm = _colmajor(B, (nx, nu))
        fv = _f64(np.zeros(nx) if f is None else f).ravel()
        Q, R = _f64(Q), _f64(R)
        Qd = (np.diag(Q) if Q.ndim == 2 else Q).copy()
        Rd = (np.diag(R) if R.ndim == 2 else R).copy()
        dev = None
        if devices is not None:
            dev = np.ascontiguousarray(devices, dtype=np.int32)
            n_shards = len(dev)
        rc = lib().tiny_group_setup(C.byref(self._h), A.ctypes.data_as(_dp), Bm.ctypes.data_as(_dp), fv.ctypes.data_as(_dp),
                                    Qd.ctypes.data_as(_dp), Rd.ctypes.data_as(_dp), float(rho), nx, nu, N, batch,
                                    None if dev is None else dev.ctypes.data_as(_ip), int(n_shards), int(bool(interleaved)), verbose)
        if rc != OK:
            self._h = C.c_void_p()
            raise TinyMPCError(f"tiny_group_setup failed ({rc}): {lib().tiny_group_last_error(None).decode()}")

    @classmethod
    def from_problem(cls, prob, batch, **kw):
        return cls(prob["A"], prob["B"], prob.get("f"), prob["Q"], prob["R"], prob["rho"], prob["nx"], prob["nu"], prob["N"], batch, **kw)

    def close(self):
        if getattr(self, "_h", None):
            lib().tiny_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != OK:
            raise TinyMPCError(f"{what} failed ({rc}): {lib().tiny_group_last_error(self._h).decode()}")

    @property
    def shards(self):
        return int(lib().tiny_group_shards(self._h))

    def uses_rccl(self):
        return bool(lib().tiny_group_uses_rccl(self._h))

    def shard_indices(self, k):
        n = lib().tiny_group_shard_indices(self._h, k, None, 0)
        idx = np.zeros(n, dtype=np.int32)
        lib().tiny_group_shard_indices(self._h, k, idx.ctypes.data_as(_ip), n)
        return idx

    def set_bound_constraints(self, x_min, x_max, u_min, u_max):
        nx, nu, N = self.nx, self.nu, self.N
        xm, xM = _colmajor(x_min, (nx, N)), _colmajor(x_max, (nx, N))
        um, uM = _colmajor(u_min, (nu, N - 1)), _colmajor(u_max, (nu, N - 1))
        self._check(lib().tiny_group_set_bound_constraints(self._h, xm.ctypes.data_as(_dp), xM.ctypes.data_as(_dp),
                                                           um.ctypes.data_as(_dp), uM.ctypes.data_as(_dp)), "set_bound_constraints")

    def set_instance_bounds(self, x_min, x_max, u_min, u_max):
        """every instance its own box, the full batch axis in the caller's order: [batch, nx, N] x 2, [batch, nu, N-1] x 2"""
        a = TinyBatchSolver._instance_boxes(self, x_min, x_max, u_min, u_max)
        self._check(lib().tiny_group_set_instance_bounds(self._h, *[v.ctypes.data_as(_dp) for v in a]), "set_instance_bounds")

    def _set_instance_halfspaces(self, tv, A_x, b_x, A_u, b_u, what):
        ns, ni, a = TinyBatchSolver._instance_halfspaces(self, tv, A_x, b_x, A_u, b_u)
        p = [None if v is None else v.ctypes.data_as(_dp) for v in a]
        f = lib().tiny_group_set_instance_tv_linear_constraints if tv else lib().tiny_group_set_instance_linear_constraints
        self._check(f(self._h, ns, p[0], p[1], ni, p[2], p[3]), what)

    def set_instance_linear_constraints(self, Alin_x, blin_x, Alin_u, blin_u):
        """every instance its own static half-spaces, the full batch axis in the caller's order (TinyBatchSolver's shapes)"""
        self._set_instance_halfspaces(0, Alin_x, blin_x, Alin_u, blin_u, "set_instance_linear_constraints")

    def set_instance_tv_linear_constraints(self, tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u):
        self._set_instance_halfspaces(1, tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u, "set_instance_tv_linear_constraints")

    def set_instance_cone_coefficients(self, cx, cu):
        """every instance its own cone coefficients, the full batch axis in the caller's order (TinyBatchSolver's shapes)"""
        a = TinyBatchSolver._instance_cones(self, cx, cu)
        p = [None if v is None else v.ctypes.data_as(_dp) for v in a]
        self._check(lib().tiny_group_set_instance_cone_coefficients(self._h, p[0], p[1], HOST), "set_instance_cone_coefficients")

    def get_instance_cone_coefficients(self, i):
        """(cx, cu) instance i (the caller's order) is held to: asked of the shard that holds it"""
        for k in range(self.shards):
            at = np.flatnonzero(self.shard_indices(k) == int(i))
            if len(at):
                h = lib().tiny_group_shard(self._h, k)
                out = [np.zeros(int(lib().tiny_batch_get_option(h, n))) for n in (b"n_state_cones", b"n_input_cones")]
                rc = lib().tiny_batch_get_instance_cone_coefficients(h, int(at[0]), *[v.ctypes.data_as(_dp) for v in out])
                if rc != OK:
                    raise TinyMPCError(f"get_instance_cone_coefficients failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
                return tuple(out)
        raise TinyMPCError(f"get_instance_cone_coefficients: instance {i} of {self.batch}")

    def set_disturbance(self, w):
        """every instance its own disturbance sequence, the full batch axis in the caller's order (TinyBatchSolver's shapes); None removes"""
        if w is None:
            return self._check(lib().tiny_group_set_disturbance(self._h, None, 0, HOST), "set_disturbance")
        flat, n, bc = TinyBatchSolver._disturbance(self, w)
        self._check(lib().tiny_group_set_disturbance(self._h, flat.ctypes.data_as(_dp), n, HOST | bc), "set_disturbance")

    def set_measurement_noise(self, v):
        """measurement noise for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); None removes"""
        if v is None:
            return self._check(lib().tiny_group_set_measurement_noise(self._h, None, 0, HOST), "set_measurement_noise")
        flat, n, bc = TinyBatchSolver._disturbance(self, v)
        self._check(lib().tiny_group_set_measurement_noise(self._h, flat.ctypes.data_as(_dp), n, HOST | bc), "set_measurement_noise")

    def generate_disturbance(self, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
        """TinyBatchSolver.generate_disturbance over the full batch axis: id_base / id_stride name the caller-order instance, so every
        instance gets the noise it gets on a single batch, whatever the sharding"""
        spec, keep = noise_spec(self.batch, self.nx, seed, n_steps, scale, mean, factor, id_base, id_stride)
        self._check(lib().tiny_group_generate_disturbance(self._h, C.byref(spec)), "generate_disturbance")

    def generate_measurement_noise(self, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
        """TinyBatchSolver.generate_measurement_noise over the full batch axis (see generate_disturbance)"""
        spec, keep = noise_spec(self.batch, self.nx, seed, n_steps, scale, mean, factor, id_base, id_stride)
        self._check(lib().tiny_group_generate_measurement_noise(self._h, C.byref(spec)), "generate_measurement_noise")

    def get_disturbance(self, step, i):
        """w[step, i] of instance i (the caller's order): asked of the shard that holds it"""
        for k in range(self.shards):
            at = np.flatnonzero(self.shard_indices(k) == int(i))
            if len(at):
                h = lib().tiny_group_shard(self._h, k)
                out = np.zeros(self.nx)
                rc = lib().tiny_batch_get_disturbance(h, int(step), int(at[0]), out.ctypes.data_as(_dp))
                if rc != OK:
                    raise TinyMPCError(f"get_disturbance failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
                return out
        raise TinyMPCError(f"get_disturbance: instance {i} of {self.batch}")

    def set_plant(self, A_p, B_p=None, f_p=None):
        """a plant of its own for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); A_p None removes"""
        if A_p is None:
            return self._check(lib().tiny_group_set_plant(self._h, None, None, None, HOST), "set_plant")
        if B_p is None:
            raise ValueError("plant: A_p without B_p")
        A, Bm, f, bc = TinyBatchSolver._plant(self, A_p, B_p, f_p)
        self._check(lib().tiny_group_set_plant(self._h, A.ctypes.data_as(_dp), Bm.ctypes.data_as(_dp), None if f is None else f.ctypes.data_as(_dp),
                                               HOST | bc), "set_plant")

    def set_estimator(self, M):
        """a state estimator for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); None removes"""
        if M is None:
            return self._check(lib().tiny_group_set_estimator(self._h, None, HOST), "set_estimator")
        flat, bc = TinyBatchSolver._gain(self, M)
        self._check(lib().tiny_group_set_estimator(self._h, flat.ctypes.data_as(_dp), HOST | bc), "set_estimator")

    def set_estimator_device(self, M, broadcast=False):
        raise TinyMPCError("estimator of a group: host arrays (a device pointer belongs to one shard)")

    def set_estimate(self, xp):
        """the predicted estimate of every instance (the caller's order), or (nx,) for all"""
        flat, bc = TinyBatchSolver._estimate(self, xp)
        self._check(lib().tiny_group_set_estimate(self._h, flat.ctypes.data_as(_dp), HOST | bc), "set_estimate")

    def get_estimator(self, i):
        """the gain of instance i (the caller's order): asked of the shard that holds it"""
        h, at = self._of_shard(i)
        out = np.zeros(self.nx * self.nx)
        rc = lib().tiny_batch_get_estimator(h, at, out.ctypes.data_as(_dp))
        if rc != OK:
            raise TinyMPCError(f"get_estimator failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
        return out.reshape(self.nx, self.nx).T.copy()

    def set_score(self, weight, target=None, lo=None, hi=None):
        """a closed-loop score for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); None removes"""
        if weight is None:
            return self._check(lib().tiny_group_set_score(self._h, None, None, None, None, HOST), "set_score")
        a, bc = TinyBatchSolver._score(self, weight, target, lo, hi)
        p = [None if v is None else v.ctypes.data_as(_dp) for v in a]
        self._check(lib().tiny_group_set_score(self._h, p[0], p[1], p[2], p[3], HOST | bc), "set_score")

    def set_score_device(self, *args, **kwargs):
        raise TinyMPCError("score of a group: host arrays (a device pointer belongs to one shard)")

    def get_score(self):
        """(cost, worst, violated_steps, first_violation), (batch,) each, gathered from the shards into the caller's order"""
        cost, worst = np.zeros(self.batch), np.zeros(self.batch)
        steps, first = np.zeros(self.batch, dtype=np.int32), np.zeros(self.batch, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        for k in range(self.shards):
            idx = self.shard_indices(k)
            c, w = np.zeros(len(idx)), np.zeros(len(idx))
            v, f = np.zeros(len(idx), dtype=np.int32), np.zeros(len(idx), dtype=np.int32)
            h = lib().tiny_group_shard(self._h, k)
            rc = lib().tiny_batch_get_score(h, c.ctypes.data_as(_dp), w.ctypes.data_as(_dp), v.ctypes.data_as(ip), f.ctypes.data_as(ip))
            if rc != OK:
                raise TinyMPCError(f"get_score failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
            cost[idx], worst[idx], steps[idx], first[idx] = c, w, v, f
        return cost, worst, steps, first

    def reset_score(self):
        for k in range(self.shards):
            h = lib().tiny_group_shard(self._h, k)
            rc = lib().tiny_batch_reset_score(h)
            if rc != OK:
                raise TinyMPCError(f"reset_score failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")

    def set_actuator(self, lo=None, hi=None, alpha=None, gain=None, offset=None):
        """an actuator model for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); all None removes"""
        a, bc = TinyBatchSolver._actuator(self, lo, hi, alpha, gain, offset)
        p = [None if v is None else v.ctypes.data_as(_dp) for v in a]
        self._check(lib().tiny_group_set_actuator(self._h, p[0], p[1], p[2], p[3], p[4], HOST | bc), "set_actuator")

    def set_actuator_device(self, *args, **kwargs):
        raise TinyMPCError("actuator of a group: host arrays (a device pointer belongs to one shard)")

    def set_actuator_state(self, a):
        """the lag's record of every instance (the caller's order), or (nu,) for all"""
        v = _f64(a)
        if v.shape not in ((self.batch, self.nu), (self.nu,)):
            raise ValueError(f"actuator state: ({self.batch}, {self.nu}) or ({self.nu},), got {v.shape}")
        self._check(lib().tiny_group_set_actuator_state(self._h, v.ctypes.data_as(_dp), HOST | (BROADCAST if v.ndim == 1 else 0)), "set_actuator_state")

    def set_actuation_noise(self, n):
        """actuation noise for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); None removes"""
        if n is None:
            return self._check(lib().tiny_group_set_actuation_noise(self._h, None, 0, HOST), "set_actuation_noise")
        flat, k, bc = TinyBatchSolver._actuation_noise(self, n)
        self._check(lib().tiny_group_set_actuation_noise(self._h, flat.ctypes.data_as(_dp), k, HOST | bc), "set_actuation_noise")

    def generate_actuation_noise(self, seed, n_steps, scale, mean=None, factor=False, id_base=0, id_stride=1):
        """TinyBatchSolver.generate_actuation_noise over the full batch axis (see generate_disturbance)"""
        spec, keep = noise_spec(self.batch, self.nu, seed, n_steps, scale, mean, factor, id_base, id_stride)
        self._check(lib().tiny_group_generate_actuation_noise(self._h, C.byref(spec)), "generate_actuation_noise")

    def set_actuator_delay(self, d=None, d_max=None):
        """a transport delay for every instance, the full batch axis in the caller's order (TinyBatchSolver's shapes); None removes"""
        if d is None:
            return self._check(lib().tiny_group_set_actuator_delay(self._h, None, 0, HOST), "set_actuator_delay")
        v, dm, bc = TinyBatchSolver._actuator_delay(self, d, d_max)
        self._check(lib().tiny_group_set_actuator_delay(self._h, v.ctypes.data_as(C.POINTER(C.c_int)), dm, HOST | bc), "set_actuator_delay")

    def _delay_max(self):
        return int(lib().tiny_batch_get_option(lib().tiny_group_shard(self._h, 0), b"actuator_delay"))

    def set_actuator_queue(self, q):
        """the delay's queue of every instance (the caller's order), oldest first: (batch, d_max, nu), or (d_max, nu) for all"""
        v, bc = TinyBatchSolver._actuator_queue(self, q)
        self._check(lib().tiny_group_set_actuator_queue(self._h, v.ctypes.data_as(_dp), HOST | bc), "set_actuator_queue")

    def get_actuator_queue(self):
        """(batch, d_max, nu), gathered from the shards into the caller's order"""
        d_max = self._delay_max()
        flat = self._from_shards(1, lambda h, part: lib().tiny_batch_get_actuator_queue(h, part.ctypes.data_as(_dp)), "get_actuator_queue", d_max * self.nu)[0]
        return flat.reshape(self.batch, d_max, self.nu)

    def get_actuator_state(self):
        """a (batch, nu), gathered from the shards into the caller's order"""
        return self._from_shards(1, lambda h, part: lib().tiny_batch_get_actuator_state(h, part.ctypes.data_as(_dp)), "get_actuator_state", self.nu)[0]

    def actuation_log(self, steps):
        """ua[steps, batch, nu] of the last solve call (option "actuation_log" = 1), gathered from the shards into the caller's order"""
        return self._from_shards(steps, lambda h, part: lib().tiny_batch_get_actuation_log(h, part.ctypes.data_as(_dp), int(steps)), "get_actuation_log", self.nu)

    def _from_shards(self, steps, read, what, width=None):
        width = self.nx if width is None else width
        out = np.zeros((steps, self.batch, width))
        for k in range(self.shards):
            idx = self.shard_indices(k)
            part = np.zeros((steps, len(idx), width))
            h = lib().tiny_group_shard(self._h, k)
            rc = read(h, part)
            if rc != OK:
                raise TinyMPCError(f"{what} failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
            out[:, idx] = part
        return out

    def get_estimate(self):
        """xp (batch, nx), gathered from the shards into the caller's order"""
        return self._from_shards(1, lambda h, part: lib().tiny_batch_get_estimate(h, part.ctypes.data_as(_dp)), "get_estimate")[0]

    def estimate_log(self, steps):
        """xhat[steps, batch, nx] of the last solve call (option "estimate_log" = 1), gathered from the shards into the caller's order"""
        return self._from_shards(steps, lambda h, part: lib().tiny_batch_get_estimate_log(h, part.ctypes.data_as(_dp), int(steps)), "get_estimate_log")

    def _of_shard(self, i):
        for k in range(self.shards):
            at = np.flatnonzero(self.shard_indices(k) == int(i))
            if len(at):
                return lib().tiny_group_shard(self._h, k), int(at[0])
        raise TinyMPCError(f"instance {i} of {self.batch}")

    def get_plant(self, i):
        """the plant of instance i (the caller's order): asked of the shard that holds it"""
        h, at = self._of_shard(i)
        A, Bm, f = np.zeros(self.nx * self.nx), np.zeros(self.nx * self.nu), np.zeros(self.nx)
        rc = lib().tiny_batch_get_plant(h, at, A.ctypes.data_as(_dp), Bm.ctypes.data_as(_dp), f.ctypes.data_as(_dp))
        if rc != OK:
            raise TinyMPCError(f"get_plant failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
        return A.reshape(self.nx, self.nx).T.copy(), Bm.reshape(self.nu, self.nx).T.copy(), f

    def state_log(self, steps):
        """x0_next[steps, batch, nx] of the last solve call (option "state_log" = 1), gathered from the shards into the caller's order"""
        out = np.zeros((steps, self.batch, self.nx))
        for k in range(self.shards):
            idx = self.shard_indices(k)
            part = np.zeros((steps, len(idx), self.nx))
            h = lib().tiny_group_shard(self._h, k)
            rc = lib().tiny_batch_get_state_log(h, part.ctypes.data_as(_dp), int(steps))
            if rc != OK:
                raise TinyMPCError(f"get_state_log failed ({rc}): {lib().tiny_batch_last_error(h).decode()}")
            out[:, idx] = part
        return out

    def set_cone_constraints(self, Acx, qcx, cx, Acu, qcu, cu):
        ai = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        Acx, qcx, Acu, qcu = ai(Acx), ai(qcx), ai(Acu), ai(qcu)
        cx, cu = _f64(cx).ravel(), _f64(cu).ravel()
        self._check(lib().tiny_group_set_cone_constraints(self._h, len(Acx), Acx.ctypes.data_as(_ip), qcx.ctypes.data_as(_ip),
                                                          cx.ctypes.data_as(_dp), len(Acu), Acu.ctypes.data_as(_ip),
                                                          qcu.ctypes.data_as(_ip), cu.ctypes.data_as(_dp)), "set_cone_constraints")

    def update_settings(self, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=1000, check_termination=1, en_state_bound=1,
                        en_input_bound=1, en_state_soc=0, en_input_soc=0, en_state_linear=0, en_input_linear=0,
                        en_tv_state_linear=0, en_tv_input_linear=0):
        self._check(lib().tiny_group_update_settings(self._h, abs_pri_tol, abs_dua_tol, max_iter, check_termination, en_state_bound,
                                                     en_input_bound, en_state_soc, en_input_soc, en_state_linear, en_input_linear,
                                                     en_tv_state_linear, en_tv_input_linear), "update_settings")

    def set_option(self, name, value):
        self._check(lib().tiny_group_set_option(self._h, name.encode(), int(value)), f"set_option({name})")

    def _shape(self, name):
        if name == "x0":
            return self.nx, 1
        return (self.nx, self.N) if name in STATE_FIELDS else (self.nu, self.N - 1)

    def set(self, name, value, broadcast=False):
        r, c = self._shape(name)
        a = np.asarray(value, dtype=np.float64)
        flat = (np.ascontiguousarray(a.reshape(r, c).T) if broadcast else
                np.ascontiguousarray(a.reshape(self.batch, r, c).transpose(0, 2, 1))).ravel()
        self._check(lib().tiny_group_set(self._h, FIELD_ID[name], flat.ctypes.data_as(C.c_void_p), HOST | (BROADCAST if broadcast else 0)), f"set({name})")

    def get(self, name):
        r, c = self._shape(name)
        out = np.zeros((self.batch, c, r))
        self._check(lib().tiny_group_get(self._h, FIELD_ID[name], out.ctypes.data_as(C.c_void_p)), f"get({name})")
        out = out.transpose(0, 2, 1)
        return out[:, :, 0] if name == "x0" else out

    def set_x0(self, x0, broadcast=False):
        self.set("x0", x0, broadcast)

    def set_x_ref(self, x_ref, broadcast=False):
        self.set("Xref", x_ref, broadcast)

    def set_u_ref(self, u_ref, broadcast=False):
        self.set("Uref", u_ref, broadcast)

    def reset(self):
        self._check(lib().tiny_group_reset(self._h), "reset")

    def solve(self) -> int:
        rc = lib().tiny_group_solve(self._h)
        if rc not in (0, 1):
            self._check(rc, "solve")
        return rc

    def solve_async(self):
        self._check(lib().tiny_group_solve_async(self._h), "solve_async")

    def synchronize(self):
        self._check(lib().tiny_group_synchronize(self._h), "synchronize")

    def allreduce_stats(self):
        out = np.zeros(10)
        self._check(lib().tiny_group_allreduce_stats(self._h, out.ctypes.data_as(_dp)), "allreduce_stats")
        return out

    def status(self):
        B = self.batch
        it, so, st = (np.zeros(B, dtype=np.int32) for _ in range(3))
        res = np.zeros((B, 4))
        self._check(lib().tiny_group_get_status(self._h, it.ctypes.data_as(_ip), so.ctypes.data_as(_ip), st.ctypes.data_as(_ip),
                                                res.ctypes.data_as(_dp)), "get_status")
        return dict(iter=it, solved=so, status=st, residuals=res)


def step_regroup_plan(steps, k=-1, known=False, half=0):
    """the stretches option "step_regroup" cuts a fused launch of `steps` MPC steps into (k <= 0: the automatic length).  Host
    arithmetic, no GPU."""
    out = np.zeros(max(int(steps), 1) + 1, dtype=np.int32)
    n = lib().tiny_step_regroup_plan(int(steps), int(k), int(bool(known)), int(half), out.ctypes.data_as(_ip), len(out))
    return [int(v) for v in out[:n]]


def predict_split(hist, nx, nu, N, max_iter, check_termination=1, num_cus=256):
    """(K, predicted time ratio) of the automatic split solve's cost model for an iteration-count histogram (hist[i] =
    instances needing i iterations); K = 0: a plain launch is predicted to be within 5 %.  Host arithmetic, no GPU."""
    h = np.zeros(1024, dtype=np.uint32)
    hist = np.asarray(hist)
    h[:min(len(hist), 1024)] = hist[:1024]
    r = C.c_double(1.0)
    k = lib().tiny_predict_split(h.ctypes.data_as(C.POINTER(C.c_uint)), nx, nu, N, max_iter, check_termination, num_cus, C.byref(r))
    return int(k), float(r.value)


def rccl_unique_id() -> bytes:
    """rank 0: a fresh 128-byte ncclUniqueId (tiny_rccl_unique_id)"""
    buf = C.create_string_buffer(128)
    rc = lib().tiny_rccl_unique_id(buf)
    if rc != OK:
        raise TinyMPCError(f"tiny_rccl_unique_id failed ({rc})")
    return buf.raw


def rccl_comm_init_rank(n_ranks, unique_id: bytes, rank, device) -> int:
    """join the communicator of `unique_id` as `rank` on GPU `device`; returns the ncclComm_t as an integer"""
    comm = C.c_void_p()
    rc = lib().tiny_rccl_comm_init_rank(C.byref(comm), int(n_ranks), C.c_char_p(unique_id), int(rank), int(device))
    if rc != OK:
        raise TinyMPCError(f"tiny_rccl_comm_init_rank failed ({rc})")
    return comm.value


def rccl_comm_destroy(comm):
    lib().tiny_rccl_comm_destroy(C.c_void_p(comm))


def rccl_comm_count(comm) -> int:
    """ranks of the communicator, asked of RCCL itself (ncclCommCount)"""
    n = lib().tiny_rccl_comm_count(C.c_void_p(comm))
    if n < 0:
        raise TinyMPCError(f"tiny_rccl_comm_count failed ({n})")
    return int(n)


def reduce_stats_messages(table, total_batch):
    """native host reduction of gathered 64-byte messages ([n_shards, 8]) -> the 10-entry statistics vector (no GPU needed)"""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1, 8))
    out = np.zeros(10)
    rc = lib().tiny_reduce_stats_messages(t.ctypes.data_as(_dp), t.shape[0], int(total_batch), out.ctypes.data_as(_dp))
    if rc != OK:
        raise TinyMPCError(f"tiny_reduce_stats_messages failed ({rc})")
    return out


def rccl_available() -> bool:
    """librccl loads next to this library's HIP runtime (nothing collective happens)"""
    return bool(lib().tiny_rccl_available())


def load_problem(name):
    """Problem families of the reference examples (numbers extracted by oracle/extract_problem_data.py)."""
    import json
    p = json.load(open(os.path.join(_HERE, "data", "problems.json")))[name]
    prob = dict(nx=p["nx"], nu=p["nu"], N=p["N"], rho=float(p["rho"]), A=np.array(p["A"], dtype=np.float64),
                B=np.array(p["B"], dtype=np.float64), f=np.array(p["f"], dtype=np.float64),
                Q=np.array(p["Q"], dtype=np.float64), R=np.array(p["R"], dtype=np.float64))
    extra = {k: v for k, v in p.items() if k not in prob and k != "source"}
    return prob, extra


def random_problem(nx, nu, N):
    """The synthetic problem family of BASELINE configs[4]: one shared (A, B, Q, R)
    per (nx, nu, N) cell, seeded; A is scaled to spectral radius 0.95."""
    rng = np.random.default_rng(1000 * nx + 10 * nu + N)
    M = rng.standard_normal((nx, nx))
    A = M * 0.95 / np.max(np.abs(np.linalg.eigvals(M)))
    B = rng.standard_normal((nx, nu)) / np.sqrt(nx)
    Q = rng.uniform(1, 10, nx)
    R = rng.uniform(0.1, 1, nu)
    return dict(nx=nx, nu=nu, N=N, rho=1.0, A=A, B=B, f=np.zeros(nx), Q=Q, R=R), rng


def flops_per_iter(nx, nu, N):
    """FLOPs of one ADMM iteration with box constraints (footnote 1)."""
    S = nx * N + nu * (N - 1)
    return (4 * S + 2 * nx * nx + 3 * nx + (N - 1) * (2 * nx * nx + 4 * nx * nu + 2 * nu * nu + 2 * nu + 3 * nx)
            + (N - 1) * (2 * nx * nx + 4 * nx * nu + 2 * nx + 2 * nu) + 11 * S)
