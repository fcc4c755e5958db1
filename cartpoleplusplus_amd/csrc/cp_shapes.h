// cp_shapes.h — which CP_SHAPE_* a handle's step and autoreset kernels run on, in plain host C++ (no HIP):
// the resolver behind cp_create / cp_set_lqr / cp_set_kernel_shape, the checks of cp_set_kernel_shape's
// requests, and the two facts the launchers (cp_env.h) share with it.  tests/shape_table.cpp pins it on the CPU.
// Also cp_policy_act's kernel choice for a policy population and the member path's work split, which the kernel
// (cp_policy.h) and the launcher share; tests/policy_runs.cpp pins those.  And cp_policy_gradient's plan (tile size,
// tiles per member, partial sums), shared by cp_policy_grad.h and the C-ABI; tests/policy_grad_plan.cpp pins it.
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

// ---- cp_policy_gradient's work split (cp_policy_grad.h; DESIGN.md §9.5 "Policy gradient")
// The window's samples (k, i) of one member run (policy_runs' runs: consecutive local envs with one member) are
// numbered s = k * len + (i - lo), and a tile is `tile` consecutive s of one run.  A member's tiles are those of its
// runs r0, r0 + P, ... in run order; `slices` blocks per member take contiguous shares of them and each writes one
// partial [F], so the scratch is slices * P * F floats.  With one member (population <= 1) the handle is one run.
constexpr int kPolicyGradThreads = 256;
constexpr size_t kPolicyGradLdsMax = 160 * 1024;  // a CU's LDS
constexpr int kPolicyGradMeta = 64 * 24;          // the kernel's static LDS: per tile column index, coeff, 2 actions

struct PolicyGrad {
    int64_t off, k0;      // env_id_offset (0 with one member); the first run's global group index
    int32_t P, G, K, B;   // P >= 1; one member: G = B
    int32_t runs;         // member runs that meet [off, off + B)
    int32_t first_len, last_len;  // envs of run 0 and of run runs - 1 (the others hold G)
    int32_t tile, es;     // samples per tile (64, 32 or 16) and the LDS row stride of a tile (floats)
    int32_t rows;         // LDS rows: every layer's inputs and a row of ones, then the 10 logits
    int32_t wfloats;      // LDS floats of the widest layer's [W | b] image
    int32_t slices;       // partial sums per member
    int64_t tiles_full;   // tiles of a run of G envs
};
struct PolicyGradTile {
    int lo, len;  // the run's local envs [lo, lo + len)
    int s0, n;    // the tile's samples s0 .. s0 + n - 1 of the run's len * K
};
CPS_HD int64_t policy_grad_run_tiles(const PolicyGrad& p, int len) { return ((int64_t)len * p.K + p.tile - 1) / p.tile; }
CPS_HD int policy_grad_run_len(const PolicyGrad& p, int r) { return r == 0 ? p.first_len : r == p.runs - 1 ? p.last_len : p.G; }
// member m's first run, or >= runs if it has none
CPS_HD int64_t policy_grad_first_run(const PolicyGrad& p, int m) { return ((int64_t)m - p.k0 % p.P + p.P) % p.P; }
CPS_HD int64_t policy_grad_member_tiles(const PolicyGrad& p, int m) {
    const int64_t r0 = policy_grad_first_run(p, m);
    if (r0 >= p.runs) return 0;
    int64_t J = (p.runs - 1 - r0) / p.P + 1, t = 0;  // the member's runs
    if (r0 == 0) {
        t += policy_grad_run_tiles(p, p.first_len);
        --J;
    }
    if (p.runs > 1 && (p.runs - 1 - r0) % p.P == 0) {
        t += policy_grad_run_tiles(p, p.last_len);
        --J;
    }
    return t + J * p.tiles_full;
}
// tile t < policy_grad_member_tiles(p, m) of member m
CPS_HD PolicyGradTile policy_grad_tile(const PolicyGrad& p, int m, int64_t t) {
    const int64_t r0 = policy_grad_first_run(p, m);
    int64_t r, within;
    const int64_t tf = r0 == 0 ? policy_grad_run_tiles(p, p.first_len) : 0;
    if (t < tf) {
        r = 0;
        within = t;
    } else {
        const int64_t j = (r0 == 0 ? 1 : 0) + (t - tf) / p.tiles_full;
        r = r0 + j * p.P;
        within = (t - tf) % p.tiles_full;
    }
    PolicyGradTile x;
    x.len = policy_grad_run_len(p, (int)r);
    x.lo = r == 0 ? 0 : (int)((p.k0 + r) * p.G - p.off);
    const int64_t total = (int64_t)x.len * p.K, s0 = within * p.tile;
    x.s0 = (int)s0;
    x.n = (int)(total - s0 < p.tile ? total - s0 : p.tile);
    return x;
}
inline int policy_grad_env_stride(int tile) { return tile % 8 == 0 ? tile + 4 : tile; }
inline size_t policy_grad_lds_bytes(const int32_t* width, int num_layers, int tile, int* rows_out, int* wfloats_out) {
    int rows = width[num_layers], wmax = 0;
    for (int l = 0; l < num_layers; ++l) {
        rows += width[l] + 1;
        const int w = policy_weight_floats(width[l], width[l + 1]);
        wmax = w > wmax ? w : wmax;
    }
    wmax = (wmax + 3) & ~3;
    if (rows_out) *rows_out = rows;
    if (wfloats_out) *wfloats_out = wmax;
    return sizeof(float) * ((size_t)rows * policy_grad_env_stride(tile) + (size_t)wmax) + kPolicyGradMeta;
}
// The plan of a call that passed cp_policy_gradient's checks (K * B < 2^31, env_id_offset >= 0 with a population).
// The tile is the largest of 64 / 32 / 16 samples whose LDS lets two blocks share a CU, else the largest that fits
// one (the widest legal policy, 4 layers of 128 units, fits at 32); slices: a block takes at least 4 tiles of the
// member with the most, and about 2,048 blocks fill the chip.
inline PolicyGrad policy_grad_plan(const int32_t* width, int num_layers, int population, int group, int64_t off, int K,
                                   int B) {
    PolicyGrad p{};
    const bool one = population <= 1;
    p.off = one ? 0 : off;
    p.P = one ? 1 : population;
    p.G = one ? B : group;
    p.K = K;
    p.B = B;
    p.k0 = p.off / p.G;
    p.runs = (int32_t)((p.off + B - 1) / p.G - p.k0) + 1;
    const int64_t end0 = (p.k0 + 1) * p.G < p.off + B ? (p.k0 + 1) * p.G : p.off + B;
    p.first_len = (int32_t)(end0 - p.off);
    p.last_len = p.runs == 1 ? p.first_len : (int32_t)(p.off + B - (p.k0 + p.runs - 1) * p.G);
    p.tile = 0;
    for (int pass = 0; pass < 2 && !p.tile; ++pass)
        for (int t = 64; t >= 16 && !p.tile; t >>= 1)
            if (policy_grad_lds_bytes(width, num_layers, t, nullptr, nullptr) <= kPolicyGradLdsMax / (pass ? 1 : 2)) p.tile = t;
    if (!p.tile) p.tile = 16;  // not reached by a policy cp_set_policy accepts
    p.es = policy_grad_env_stride(p.tile);
    int rows, wf;
    policy_grad_lds_bytes(width, num_layers, p.tile, &rows, &wf);
    p.rows = rows;
    p.wfloats = wf;
    p.tiles_full = policy_grad_run_tiles(p, p.G);
    // an upper bound of a member's tiles
    const int64_t most = ((int64_t)p.runs + p.P - 1) / p.P * policy_grad_run_tiles(p, p.G < B ? p.G : B);
    const int64_t want = (most + 3) / 4, cap = p.P >= 2048 ? 1 : 2048 / p.P;
    p.slices = (int32_t)(want < 1 ? 1 : want < cap ? want : cap);
    return p;
}
inline int64_t policy_grad_scratch_bytes(const PolicyGrad& p, int64_t F) {
    return ((int64_t)p.slices * p.P * F * (int64_t)sizeof(float) + 15) & ~(int64_t)15;
}

}  // namespace cps
