// closed_loop.hpp -- the state of the stages at the fused closed-loop plant step (batch_closed_loop.hip sets, builds, reads and drops
// it; TinyBatch of batch_impl.hpp holds one member per stage): a disturbance, a plant of its own with the state log, measurement
// noise, a state estimator, a score, an actuator model with actuation noise and a transport delay in front of it.  One shape per kind of state: StepSequence (a step-major
// sequence and its counter), StepLog (what every MPC step of the last solve call left), ModelBlock (the batch's own model as a plant
// block), and per stage the caller's arrays `src` next to the lane block `built` the one-row kernel reads.  Plain C++, no HIP call.
// Every struct names the device buffers it owns in each_buffer: the drop paths and tiny_batch_destroy free through it, nothing else
#pragma once
#include <algorithm>
#include <cstdint>

// a step-major sequence seq [steps][batch][width] -- a launch reads one contiguous [batch][width] block per MPC step; a broadcast
// sequence is expanded to that layout on the device.  step: the row the next MPC step takes (the setter rewinds it, an option moves it,
// every MPC step of a launch that takes a plant step under it advances it, tiny_batch_reset leaves it alone); rows outside
// [0, steps) add nothing.  generated: the sequence came from tiny_batch_generate_* (options "*_generated")
struct StepSequence {
    double* seq = nullptr;
    int steps = 0;
    long step = 0;
    bool generated = false;
    template <class F> void each_buffer(F f) { f(seq); }
};
// what every MPC step of the LAST solve call left behind: buf [capacity][batch][width], of which that call wrote `rows`
struct StepLog {
    bool on = false;                               // the option that asks for it ("state_log", "estimate_log", "actuation_log")
    double* buf = nullptr;
    int capacity = 0, rows = 0;
};
// the batch's own model as a plant: src: A | B | f of a shared family as the coverage path's helper kernels read them (a per-instance
// family: the arrays tiny_batch_setup_hetero keeps, src stays null), built: the block(s) the one-row kernel reads (plant_entry of
// lane_tables.hpp).  What measurement noise and an actuator step the true state by with no plant installed, and what a state
// estimator predicts by whatever plant is installed.  Made once, on demand: A, B and f are fixed at setup (no setter moves them;
// adaptive rho moves the cache only); freed at destroy
struct ModelBlock {
    double *src[3] = {nullptr, nullptr, nullptr}, *built = nullptr;
    template <class F> void each_buffer(F f) { for (double*& p : src) f(p); f(built); }
};

// every instance its own additive disturbance at the plant step (tiny_batch_set_disturbance), rows of nx entries
struct Disturbance : StepSequence {
    bool last = false;                             // the last solve's launches applied the sequence: installed and a plant step taken
};
// a plant model of its own at the plant step (tiny_batch_set_plant) and the log of the x0 every MPC step handed on (option "state_log").
// src: the caller's A_p | B_p | f_p, kept on the device as given ([batch][...] column-major, or ONE set with kind 1; f_p may be null:
// zero) -- what the getter and the coverage path's helper kernel read; built: the blocks the one-row kernel's PP forms read
// (plant_entry: [batch or 1][nx + nu + 1][16]), made in front of the next launch; next: [batch][nx], where the coverage path's helper
// kernel puts the new states before they replace x0
struct PlantStep {
    int kind = 0;                                  // 0 none, 1 one plant for all, 2 every instance its own
    bool dirty = false, last = false;              // (... took their plant step through it: installed and a plant step taken)
    double *src[3] = {nullptr, nullptr, nullptr}, *built = nullptr, *next = nullptr;
    StepLog log;                                   // rows of nx entries
    template <class F> void each_buffer(F f) { for (double*& p : src) f(p); f(built); f(next); f(log.buf); }
};
// measurement noise at the plant step (tiny_batch_set_measurement_noise), rows of nx entries.  While it applies the x0 record is the
// TRUE state and the plant step goes through a plant block: the installed plant's, or the model's (TinyBatch::model).  xm [batch][nx]:
// where the coverage path forms the measurements its launch takes as x0
struct MeasurementNoise : StepSequence {
    bool last = false;                             // (... applied the sequence: installed and a plant step taken)
    double* xm = nullptr;
    template <class F> void each_buffer(F f) { f(seq); f(xm); }
};
// a fixed-gain state estimator between the measurement and the solve (tiny_batch_set_estimator) and the log of what every MPC step
// solved from (option "estimate_log").  src: the caller's M, kept on the device as given ([batch][nx*nx] column-major, or ONE with kind
// 1) -- what the getter and the coverage path's helper kernel read; built: the blocks the one-row kernel's PE forms read (gain_entry:
// [batch or 1][nx][16]), made in front of the next launch; xp [batch][nx]: the predicted estimate, STATE of the batch like x0 (it lives
// as long as an estimator is installed); xhat [batch][nx]: where the coverage path forms the corrected estimates its launch takes as x0
struct Estimator {
    int kind = 0;                                  // 0 none, 1 one gain for all, 2 every instance its own
    bool dirty = false, last = false;              // (... went through it: installed and a plant step taken)
    double *src = nullptr, *built = nullptr, *xp = nullptr, *xhat = nullptr;
    StepLog log;                                   // rows of nx entries
    template <class F> void each_buffer(F f) { f(src); f(built); f(xp); f(xhat); f(log.buf); }
};
// a closed-loop score at the plant step (tiny_batch_set_score).  src: the caller's weight | target | lo | hi, kept on the device as given
// ([batch][nx+nu] each, or ONE with kind 1; target, lo and hi may be null) -- what the getter and the coverage path's helper kernel read;
// built: the blocks the one-row kernel's PS forms read (score_entry: [batch or 1][4][16]), made in front of the next launch; rec
// [batch]: the record (ScoreRecord of admm_kernel.hip.h), STATE of the batch: it accumulates over launches until the setter or
// tiny_batch_reset_score zeroes it.  step: the score step counter (the setter and the reset rewind it, option "score_step" moves it,
// every MPC step of a launch that takes a plant step advances it)
struct Score {
    int kind = 0;                                  // 0 none, 1 one setup for all, 2 every instance its own
    bool dirty = false, last = false;              // (... scored: installed and a plant step taken)
    double *src[4] = {nullptr, nullptr, nullptr, nullptr}, *built = nullptr;
    void* rec = nullptr;
    long step = 0;
    template <class F> void each_buffer(F f) { for (double*& p : src) f(p); f(built); f(rec); }
};
// an actuator model between the command and the plant step (tiny_batch_set_actuator).  src: the caller's lo | hi | alpha | gain | offset,
// kept on the device as given ([batch][nu] each, or ONE with kind 1; any may be null) -- what the getter and the coverage path's helper
// kernel read; built: the blocks the one-row kernel's PA forms read (actuator_entry: [batch or 1][5][16]), made in front of the next
// launch; state [batch][nu]: the lag's record a, STATE of the batch, there while a lag (alpha) is installed; ua [batch][nu]: where the
// coverage path's helper kernel puts the applied control for the plant and score helpers behind it; log: the applied control of every
// MPC step (option "actuation_log"); desc: the record the PA forms read (ActuatorLaunch of admm_kernel.hip.h), written on the stream in
// front of a solve call's first launch.  last: the last solve's launches went through the actuator -- this setup or the actuation
// noise (TinyBatch::anoise, a StepSequence with rows of nu entries: the applied control's last stage)
struct Actuator {
    int kind = 0;                                  // 0 none, 1 one setup for all, 2 every instance its own
    bool lag = false;                              // alpha is installed
    bool dirty = false, last = false;
    double *src[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *built = nullptr, *state = nullptr, *ua = nullptr;
    StepLog log;                                   // rows of nu entries
    void* desc = nullptr;
    template <class F> void each_buffer(F f) { for (double*& p : src) f(p); f(built); f(state); f(ua); f(log.buf); f(desc); }
};
// a transport delay in front of the actuator's stages (tiny_batch_set_actuator_delay) and the predictor that compensates it (option
// "delay_compensation").  d [batch] ints: every instance's delay in MPC steps, 0 .. d_max; queue [batch][d_max][nu]: the instance's last
// d commands, STATE of the batch like the lag's record -- a ring over the instance's first d rows; head [batch] ints: the row of the
// oldest entry (the getter unrolls it: how the device stores the queue is not observable).  s0 [batch][nu]: where the coverage path's
// actuator helper puts what left the queue, for the estimator's prediction helper under compensation; xs [batch][nx]: where the coverage
// path forms the predicted states its launch takes as x0.  On the one-row kernel the PQ / PX forms read all of it through the actuator's
// launch record (Actuator::desc)
struct ActuatorDelay {
    int d_max = 0;                                 // 0: none installed
    bool compensate = false;                       // option "delay_compensation" (inert with no delay installed)
    int *d = nullptr, *head = nullptr;
    double *queue = nullptr, *s0 = nullptr, *xs = nullptr;
    template <class F> void each_buffer(F f) { f(d); f(head); f(queue); f(s0); f(xs); }
};

namespace tinympc_amd {
// the pointer a form reads for a lane block: bit 0 says "one block for all", bit 1 (the actuator's) "a lag is installed"
inline const double* tagged_block(const double* ptr, bool shared, bool lag = false) {
    return reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(ptr) | (shared ? (uintptr_t)1 : (uintptr_t)0) | (lag ? (uintptr_t)2 : (uintptr_t)0));
}
// a step counter as the kernels take it (they count steps in an int; a counter moved beyond +-2^30 is outside every sequence either way)
inline int kernel_step(long step) { return (int)std::clamp<long>(step, -(1L << 30), 1L << 30); }
}  // namespace tinympc_amd
