// cp_shapes.h — which CP_SHAPE_* a handle's step and autoreset kernels run on, in plain host C++ (no HIP):
// the resolver behind cp_create / cp_set_lqr / cp_set_kernel_shape, the checks of cp_set_kernel_shape's
// requests, and the two facts the launchers (cp_env.h) share with it.  tests/shape_table.cpp pins it on the CPU.
// Also cp_policy_act's kernel choice for a policy population and the member path's work split, which the kernel
// (cp_policy.h) and the launcher share; tests/policy_runs.cpp pins those.
#pragma once
#include <stddef.h>

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

// ---- cp_policy_act's kernel for a policy population (cp_policy.h)
#ifdef __HIPCC__
#define CPS_HD __host__ __device__ inline
#else
#define CPS_HD inline
#endif

enum PolicyPath {
    POLICY_SHARED,  // population <= 1: the lane-per-env kernel, one weight set
    POLICY_WAVE,    // every wave of the lane-per-env kernel serves one member (scalar weight loads stay)
    POLICY_MEMBER,  // a wave's lanes would belong to several members: one member run per wave
};
inline PolicyPath policy_path(int population, int group, int64_t env_id_offset) {
    if (population <= 1) return POLICY_SHARED;
    return (group % 64 == 0 && env_id_offset % 64 == 0) ? POLICY_WAVE : POLICY_MEMBER;
}

// The member path's work split.  A member run is a maximal stretch of consecutive local envs with one member:
// run r holds the global ids [(k0 + r) G, (k0 + r + 1) G) cut to the handle's [off, off + B), k0 = off / G, and
// is served in chunks of at most 64 envs, one chunk per wave (block): block = r * chunks_per_run + c.  The first
// and last run can be short, so their trailing chunks can be empty.
struct PolicyRuns {
    int64_t k0;          // the first run's global group index
    int runs;            // member runs that meet [off, off + B)
    int chunks_per_run;  // ceil(min(G, B) / 64)
};
CPS_HD PolicyRuns policy_runs(int64_t off, int group, int B) {
    PolicyRuns r;
    r.k0 = off / group;
    r.runs = (int)((off + B - 1) / group - r.k0) + 1;
    r.chunks_per_run = ((group < B ? group : B) + 63) / 64;
    return r;
}
struct PolicyChunk {
    int lo, n;       // local envs [lo, lo + n), n <= 64; n <= 0: an empty chunk
    int64_t member;  // ((off + lo) / G) % P
};
CPS_HD PolicyChunk policy_chunk(int64_t off, int group, int population, int B, const PolicyRuns& r, int block) {
    const int run = block / r.chunks_per_run, c = block - run * r.chunks_per_run;
    const int64_t k = r.k0 + run;
    const int64_t g0 = k * group > off ? k * group : off;                          // the run, in global ids
    const int64_t g1 = (k + 1) * group < off + B ? (k + 1) * group : off + B;
    PolicyChunk ch;
    ch.lo = (int)(g0 - off) + c * 64;
    const int end = (int)(g1 - off);
    ch.n = (end - ch.lo < 64 ? end - ch.lo : 64);
    ch.member = k % population;
    return ch;
}

// The member path's LDS (floats), per block: two activation tiles [width][env stride] and one layer's weights
// with odd row strides (policy_env_stride / policy_weight_floats are what the kernel indexes with).
CPS_HD int policy_env_stride(int group, int B) {
    const int n = group < B ? (group < 64 ? group : 64) : (B < 64 ? B : 64);  // the longest chunk
    const int es = n <= 4 ? 4 : (n + 15) / 16 * 16;  // env blocks of 4, or of 16 (cp_policy.h)
    return es % 8 == 0 ? es + 4 : es;                // 16-byte rows whose 8-lane store groups cover 32 banks
}
CPS_HD int policy_weight_floats(int nin, int nout) {  // W rows at stride nin | 1, then b continuing that grid
    return (nout + (nout + nin - 1) / nin) * (nin | 1);
}
inline size_t policy_member_lds_bytes(const int32_t* width, int num_layers, int group, int B) {
    int amax = 0, wmax = 0;
    for (int l = 0; l <= num_layers; ++l) amax = width[l] > amax ? width[l] : amax;
    for (int l = 0; l < num_layers; ++l) {
        const int w = policy_weight_floats(width[l], width[l + 1]);
        wmax = w > wmax ? w : wmax;
    }
    return sizeof(float) * ((size_t)2 * amax * policy_env_stride(group, B) + (size_t)((wmax + 3) & ~3));
}

}  // namespace cps
