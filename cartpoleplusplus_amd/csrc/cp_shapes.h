// cp_shapes.h — which CP_SHAPE_* a handle's step and autoreset kernels run on, in plain host C++ (no HIP):
// the resolver behind cp_create / cp_set_lqr / cp_set_kernel_shape, the checks of cp_set_kernel_shape's
// requests, and the two facts the launchers (cp_env.h) share with it.  tests/shape_table.cpp pins it on the CPU.
#pragma once
#include "../../include/cartpole_amd.h"

namespace cps {

// fp64, CP_MODEL_PERSISTENT and CP_MODEL_SLEEPING handles have the two-lane latency layout only
inline bool latency_only(bool f64, unsigned model_flags) {
    return f64 || (model_flags & (CP_MODEL_PERSISTENT | CP_MODEL_SLEEPING)) != 0;
}

// lanes per env of a shape's layout (CP_SHAPE_LIST launches several: launch_reset)
inline int lanes_per_env(int shape) {
    return shape == CP_SHAPE_WIDE ? 16 : shape == CP_SHAPE_WIDE8 ? 8 : shape == CP_SHAPE_WIDE64 ? 64 : 2;
}

// CP_STEP_LATENCY / CP_RESET_LATENCY: -1 unset (or neither "0" nor "1"), else 0 / 1
inline int knob_value(const char* v) { return (v && (v[0] == '0' || v[0] == '1')) ? v[0] - '0' : -1; }

struct ShapeInputs {
    int num_envs;
    bool f64;
    unsigned model_flags;
    int autoreset;            // CP_AUTORESET_*
    bool done_on_bounds;
    bool lqr_done;            // the LQR policy is on with a done threshold > 0
    int step_knob, reset_knob;  // knob_value of CP_STEP_LATENCY / CP_RESET_LATENCY
    int step_req, reset_req;  // cp_set_kernel_shape requests (CP_SHAPE_AUTO: the resolver decides)
};
struct Shapes {
    int step, reset;
};

// cp_set_kernel_shape's checks: null, or why the requests are refused
inline const char* check_requests(bool f64, unsigned model_flags, int step_req, int reset_req) {
    auto ok = [](int v) { return v >= CP_SHAPE_AUTO && v <= CP_SHAPE_LIST; };
    if (!ok(step_req) || !ok(reset_req))
        return "shapes must be CP_SHAPE_AUTO, CP_SHAPE_THROUGHPUT, CP_SHAPE_LATENCY, CP_SHAPE_WIDE, CP_SHAPE_WIDE8, "
               "CP_SHAPE_WIDE64 or CP_SHAPE_LIST";
    if (step_req == CP_SHAPE_WIDE64 || step_req == CP_SHAPE_LIST)
        return "CP_SHAPE_WIDE64 and CP_SHAPE_LIST are reset-kernel layouts";
    auto free = [](int v) { return v == CP_SHAPE_AUTO || v == CP_SHAPE_LATENCY; };
    if (latency_only(f64, model_flags) && !(free(step_req) && free(reset_req)))
        return "fp64, persistent-manifold and sleeping-model handles have the latency shape only";
    return nullptr;
}

// CP_SHAPE_AUTO picks, for the latency-shaped kernels, the widest layout whose waves still fit the chip once
// (1,024 SIMDs x 64 lanes): for the step kernel 16 lanes per env up to 4,096 envs (C2), 8 up to 8,192, else
// the two-lane layout; for the reset kernel also one env per wave (64 lanes) up to 1,024 envs.  The reset lists
// of desynchronised episodes (bounds / LQR termination) have a length only the device knows: tens to hundreds
// of envs per step, thousands where many episodes reach max_episode_len together, the whole batch at the first
// cp_reset; CP_SHAPE_LIST launches one kernel per layout and the list's length picks the one that runs
// (one env per wave for short lists).  Measured in profiles/rd7d_wide, rd7e_wide, rd7m_reset, rd7z_bench,
// rd8f_list.
inline int step_layout_for(int envs) {
    return envs <= 4096 ? CP_SHAPE_WIDE : (envs <= 8192 ? CP_SHAPE_WIDE8 : CP_SHAPE_LATENCY);
}
inline int reset_layout_for(int envs) { return envs <= 1024 ? CP_SHAPE_WIDE64 : step_layout_for(envs); }

// The shapes of a handle whose requests passed check_requests.  Register budget first: the latency budget (every
// wave a SIMD of its own) up to 32,768 envs, where even a full burst fits the chip's 1,024 SIMDs once, and for the
// reset kernel also whenever episodes can end early (bounds termination, LQR done thresholds): they end at
// different steps, so every step resets a short list and its latency is the step's, while fixed-length episodes
// end together in bursts (throughput).  A knob of 0 / 1 overrides the budget only: under the latency budget the
// layout is then chosen as without the knob.  A request overrides budget and layout.
inline Shapes resolve_shapes(const ShapeInputs& in) {
    if (latency_only(in.f64, in.model_flags)) return {CP_SHAPE_LATENCY, CP_SHAPE_LATENCY};
    const bool small = in.num_envs <= 32768;
    const bool early = in.done_on_bounds || in.lqr_done;
    const bool step_lat = in.step_knob >= 0 ? in.step_knob != 0 : small;
    const bool reset_lat = in.reset_knob >= 0 ? in.reset_knob != 0 : (early || small);
    Shapes s;
    s.step = step_lat ? step_layout_for(in.num_envs) : CP_SHAPE_THROUGHPUT;
    // Lists of desynchronised episodes: CP_SHAPE_LIST under either autoreset mode (bounds regime, steps 61-260:
    // SAME_STEP 10.9 M with one env per wave whatever the list's length, 11.1 M two-lane, 13.2 M by the length;
    // NEXT_STEP 17.6 / 21.5 / 24.9 M; profiles/rd8f_list).  Fixed-length episodes under NEXT_STEP keep the
    // two-lane reset beside the next call's step kernel.
    s.reset = !reset_lat ? CP_SHAPE_THROUGHPUT
              : early ? CP_SHAPE_LIST
              : in.autoreset != CP_AUTORESET_NEXT_STEP ? reset_layout_for(in.num_envs) : CP_SHAPE_LATENCY;
    if (in.step_req != CP_SHAPE_AUTO) s.step = in.step_req;
    if (in.reset_req != CP_SHAPE_AUTO) s.reset = in.reset_req;
    return s;
}

}  // namespace cps
