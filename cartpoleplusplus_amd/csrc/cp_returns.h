// Episode returns, GAE and standardised advantages of a rollout window (C-ABI and the arithmetic contract:
// include/cartpole_amd.h, cp_returns).
//
// One lane per env, consecutive lanes on consecutive envs: every [k][.] row access of a wave is one coalesced
// 4-byte (reward, values, adv) or 1-byte (done, valid) load or store.  The recurrences are serial in k but no load
// depends on them, so a lane holds BLK steps in registers and the next BLK are in flight while it computes
// (one wave per block, so that a small batch still spreads over the CUs: at B = 4,096 there are only 64 waves).
//
//   DISCOUNTED / GAE   one backward walk (scan_kernel); STICKY needs the env's first done sample first, a forward
//                      walk over the done column alone
//   EPISODE_TOTAL      the totals add up forwards (total_forward_kernel: the total goes to adv at the done sample
//                      that closes a segment, and valid gets a code 0 padding / 1 step / 2 closing step), and a
//                      backward walk (total_backward_kernel) spreads each total over its segment.  Every access
//                      stays a coalesced row access however ragged the episodes are.
//   STANDARDISE        per env (n, sum x) in fp64 from the walk above; per member a block reduction in a fixed
//                      order (member_reduce_kernel, S slices per member); a walk for sum (x - mean)^2
//                      (deviation_kernel); the same reduction; a walk that normalises (normalise_kernel).  A lane
//                      adds its member's S slices itself, in slice order, so every lane of a member gets the same
//                      bits.  No floating-point atomics anywhere.
#pragma once

#include <hip/hip_runtime.h>

namespace cpret {

constexpr int BLK = 8;            // steps a lane holds in registers
constexpr int THREADS = 64;       // walk kernels: one wave per block
constexpr int RED_THREADS = 256;  // member_reduce_kernel
constexpr int RED_WAVES = RED_THREADS / 64;
constexpr int MAX_SLICES = 32;    // S <= this: what a lane adds up per member
constexpr int64_t SLICE_ENVS = 8192;

struct Args {
    int K, B;
    uint32_t flags;
    float gamma, c;  // c = fl(gamma * lambda)
    int64_t off;     // env_id_offset
    int32_t P, G;    // P >= 1, G >= 1
    int S;           // slices per member
    int64_t chunk;   // envs (of a member's list) per slice
    const float* reward;
    const uint8_t* done;
    const float* values;
    const float* head;
    const uint8_t* done_in;
    const float* tail;
    float* adv;
    uint8_t* valid;
    float* carry;
    float* ret;
    double* stats;
    // scratch
    int32_t* cnt;    // [B] valid samples per env
    double* sum;     // [B] their sum
    double* sum2;    // [B] their squared deviations from the member's mean
    double2* part1;  // [P][S] (n, sum x)
    double2* part2;  // [P][S] (n, sum (x - mean)^2)
};

__device__ inline size_t at(const Args& a, int k, int i) { return (size_t)k * (size_t)a.B + (size_t)i; }

// ---------------------------------------------------------------------------------------------------------
// EPISODE_TOTAL, forwards
struct FwdBlk {
    float r[BLK];
    uint8_t d[BLK];
};

__device__ inline FwdBlk load_fwd(const Args& a, int k0, int i) {
    FwdBlk b;
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
        const int k = k0 + j;
        b.r[j] = k < a.K ? a.reward[at(a, k, i)] : 0.0f;
        b.d[j] = k < a.K ? a.done[at(a, k, i)] : (uint8_t)0;
    }
    return b;
}

template <int BOUNDARY>
__global__ void __launch_bounds__(THREADS) total_forward_kernel(Args a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.B) return;
    // pad: whether the sample about to be read is padding
    bool pad = BOUNDARY != CP_RET_BOUNDARY_SAME_STEP && a.done_in && a.done_in[i];
    float T = (a.head && !pad) ? a.head[i] : 0.0f;
    bool open = false;
    FwdBlk cur = load_fwd(a, 0, i);
    for (int k0 = 0; k0 < a.K; k0 += BLK) {
        FwdBlk nxt = cur;
        if (k0 + BLK < a.K) nxt = load_fwd(a, k0 + BLK, i);
#pragma unroll
        for (int j = 0; j < BLK; ++j) {
            const int k = k0 + j;
            if (k >= a.K) break;
            const bool dn = cur.d[j] != 0;
            uint8_t code = 0;
            if (pad) {
                open = false;
                if (BOUNDARY == CP_RET_BOUNDARY_NEXT_STEP) pad = dn;
            } else {
                T = T + cur.r[j];
                if (dn) {
                    a.adv[at(a, k, i)] = T;
                    T = 0.0f;
                    code = 2;
                    open = false;
                    pad = BOUNDARY != CP_RET_BOUNDARY_SAME_STEP;
                } else {
                    code = 1;
                    open = true;
                }
            }
            a.valid[at(a, k, i)] = code;
        }
        cur = nxt;
    }
    if (a.carry) a.carry[i] = open ? T : 0.0f;
}

// EPISODE_TOTAL, backwards: valid holds the forward walk's codes, adv the totals at the closing steps
struct CodeBlk {
    uint8_t c[BLK];
};

__device__ inline CodeBlk load_codes(const Args& a, int k0, int i) {
    CodeBlk b;
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
        const int k = k0 + j;
        b.c[j] = k < a.K ? a.valid[at(a, k, i)] : (uint8_t)0;
    }
    return b;
}

__global__ void __launch_bounds__(THREADS) total_backward_kernel(Args a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.B) return;
    float T = 0.0f;
    bool closed = false;
    int32_t n = 0;
    double sum = 0.0;
    const int top = ((a.K - 1) / BLK) * BLK;
    CodeBlk cur = load_codes(a, top, i);
    for (int k0 = top; k0 >= 0; k0 -= BLK) {
        CodeBlk nxt = cur;
        if (k0 > 0) nxt = load_codes(a, k0 - BLK, i);
        float t[BLK];
#pragma unroll
        for (int j = 0; j < BLK; ++j) {
            const int k = k0 + j;
            t[j] = (k < a.K && cur.c[j] == 2) ? a.adv[at(a, k, i)] : 0.0f;
        }
#pragma unroll
        for (int j = BLK - 1; j >= 0; --j) {
            const int k = k0 + j;
            if (k >= a.K) continue;
            if (cur.c[j] == 0) closed = false;
            if (cur.c[j] == 2) {
                T = t[j];
                closed = true;
            }
            const bool v = closed && cur.c[j] != 0;
            const float x = v ? T : 0.0f;
            a.adv[at(a, k, i)] = x;
            a.valid[at(a, k, i)] = v ? 1 : 0;
            if (v) {
                ++n;
                sum += (double)x;
            }
        }
        cur = nxt;
    }
    if (a.flags & CP_RET_STANDARDISE) {
        a.cnt[i] = n;
        a.sum[i] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------------
// DISCOUNTED and GAE, backwards
template <bool GAE>
struct ScanBlk {
    float r[BLK];
    float v[GAE ? BLK : 1];
    uint8_t d[BLK];
    uint8_t dprev;  // done of the sample below the block (done_in below k = 0): NEXT_STEP's padding of d[0]
};

template <bool GAE, int BOUNDARY>
__device__ inline ScanBlk<GAE> load_scan(const Args& a, int k0, int i, bool din) {
    ScanBlk<GAE> b;
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
        const int k = k0 + j;
        b.r[j] = k < a.K ? a.reward[at(a, k, i)] : 0.0f;
        b.d[j] = k < a.K ? a.done[at(a, k, i)] : (uint8_t)0;
        if (GAE) b.v[j] = k < a.K ? a.values[at(a, k, i)] : 0.0f;
    }
    b.dprev = 0;
    if (BOUNDARY == CP_RET_BOUNDARY_NEXT_STEP) b.dprev = k0 > 0 ? a.done[at(a, k0 - 1, i)] : (uint8_t)(din ? 1 : 0);
    return b;
}

template <bool GAE, int BOUNDARY>
__global__ void __launch_bounds__(THREADS) scan_kernel(Args a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.B) return;
    const bool din = a.done_in && a.done_in[i];
    // STICKY: the samples above the env's first done sample are padding (all of them after a done_in)
    int first = a.K;
    if (BOUNDARY == CP_RET_BOUNDARY_STICKY) {
        if (din) {
            first = -1;
        } else {
            for (int k0 = 0; k0 < a.K; k0 += BLK) {
                uint8_t d[BLK];
#pragma unroll
                for (int j = 0; j < BLK; ++j) d[j] = k0 + j < a.K ? a.done[at(a, k0 + j, i)] : (uint8_t)0;
#pragma unroll
                for (int j = BLK - 1; j >= 0; --j)
                    if (d[j] && k0 + j < first) first = k0 + j;
            }
        }
    }
    const bool mask_open = (a.flags & CP_RET_MASK_OPEN) != 0;
    float G = (!GAE && a.tail) ? a.tail[i] : 0.0f;  // G_{k+1}
    float A = 0.0f;                                  // A_{k+1}
    float vnext = GAE ? a.values[at(a, a.K, i)] : 0.0f;
    bool open = true;
    int32_t n = 0;
    double sum = 0.0;
    const int top = ((a.K - 1) / BLK) * BLK;
    ScanBlk<GAE> cur = load_scan<GAE, BOUNDARY>(a, top, i, din);
    for (int k0 = top; k0 >= 0; k0 -= BLK) {
        ScanBlk<GAE> nxt = cur;
        if (k0 > 0) nxt = load_scan<GAE, BOUNDARY>(a, k0 - BLK, i, din);
#pragma unroll
        for (int j = BLK - 1; j >= 0; --j) {
            const int k = k0 + j;
            if (k >= a.K) continue;
            const bool dn = cur.d[j] != 0;
            bool pad = false;
            if (BOUNDARY == CP_RET_BOUNDARY_STICKY) pad = k > first;
            if (BOUNDARY == CP_RET_BOUNDARY_NEXT_STEP) pad = (j > 0 ? cur.d[j - 1] : cur.dprev) != 0;
            const float r = cur.r[j];
            const float V = GAE ? cur.v[j] : 0.0f;
            float x = 0.0f, rt = 0.0f;
            bool v = false;
            if (pad) {
                open = false;
                G = 0.0f;
                A = 0.0f;
            } else {
                if (dn) {
                    open = false;
                    if (GAE) A = r - V;
                    else G = r;
                } else if (GAE) {
                    const float gv = a.gamma * vnext;
                    const float ca = a.c * A;
                    A = ((r + gv) - V) + ca;
                } else {
                    const float gg = a.gamma * G;
                    G = r + gg;
                }
                v = !(mask_open && open);
                if (v) {
                    x = GAE ? A : G;
                    if (GAE) rt = A + V;
                }
            }
            vnext = V;
            a.adv[at(a, k, i)] = x;
            a.valid[at(a, k, i)] = v ? 1 : 0;
            if (GAE && a.ret) a.ret[at(a, k, i)] = rt;
            if (v) {
                ++n;
                sum += (double)x;
            }
        }
        cur = nxt;
    }
    if (a.carry) a.carry[i] = 0.0f;
    if (a.flags & CP_RET_STANDARDISE) {
        a.cnt[i] = n;
        a.sum[i] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------------
// STANDARDISE
__device__ inline int32_t member_of(const Args& a, int i) { return (int32_t)(((a.off + i) / a.G) % a.P); }

// The envs of this call that map to member m, in ascending order: global ids (q P + m) G + r, r < G, cut to
// [off, off + B).  Only the first and the last period can hold a cut run, so the list is the first period's
// piece, then whole runs, then the last period's piece, and list index -> env needs no search.
struct MemberList {
    int64_t lo0, len0, q0, total;
    int32_t m;
};

__device__ inline MemberList member_list(const Args& a, int32_t m) {
    const int64_t period = (int64_t)a.P * a.G, end = a.off + a.B;
    MemberList l;
    l.m = m;
    l.q0 = a.off / period;
    const int64_t q1 = (end - 1) / period;
    const int64_t g0 = (l.q0 * a.P + m) * a.G;
    l.lo0 = g0 > a.off ? g0 : a.off;
    const int64_t hi0 = g0 + a.G < end ? g0 + a.G : end;
    l.len0 = hi0 > l.lo0 ? hi0 - l.lo0 : 0;
    l.total = l.len0;
    if (q1 > l.q0) {
        const int64_t g1 = (q1 * a.P + m) * a.G;  // >= off
        const int64_t hi1 = g1 + a.G < end ? g1 + a.G : end;
        l.total += (q1 - l.q0 - 1) * a.G + (hi1 > g1 ? hi1 - g1 : 0);
    }
    return l;
}

__device__ inline int member_env(const Args& a, const MemberList& l, int64_t idx) {
    if (idx < l.len0) return (int)(l.lo0 + idx - a.off);
    const uint32_t e = (uint32_t)(idx - l.len0), g = (uint32_t)a.G;  // e < B
    const int64_t q = l.q0 + 1 + e / g;
    return (int)((q * a.P + l.m) * a.G + e % g - a.off);
}

// part[m][s] = (sum cnt, sum val) over slice s of member m's list: a thread adds its envs in ascending order,
// then the wave's shuffle tree, then the block's waves in order
__global__ void __launch_bounds__(RED_THREADS) member_reduce_kernel(Args a, const double* val, double2* part) {
    __shared__ double lds[2 * RED_WAVES];
    const int32_t m = (int32_t)(blockIdx.x / (unsigned)a.S);
    const int s = (int)(blockIdx.x % (unsigned)a.S);
    const MemberList l = member_list(a, m);
    const int64_t lo = (int64_t)s * a.chunk;
    const int64_t hi = lo + a.chunk < l.total ? lo + a.chunk : l.total;
    double n = 0.0, acc = 0.0;
    for (int64_t idx = lo + threadIdx.x; idx < hi; idx += RED_THREADS) {
        const int i = member_env(a, l, idx);
        n += (double)a.cnt[i];
        acc += val[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_down(n, o, 64);
        acc += __shfl_down(acc, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds[2 * wave] = n;
        lds[2 * wave + 1] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tn = lds[0], ta = lds[1];
#pragma unroll
        for (int w = 1; w < RED_WAVES; ++w) {
            tn += lds[2 * w];
            ta += lds[2 * w + 1];
        }
        part[(size_t)m * a.S + s] = make_double2(tn, ta);
    }
}

struct MemberStats {
    double n, mean, std;
    bool degenerate;
};

// a member's slices added in slice order
__device__ inline double2 member_total(const Args& a, const double2* part, int32_t m) {
    double2 t = make_double2(0.0, 0.0);
    for (int s = 0; s < a.S; ++s) {
        const double2 p = part[(size_t)m * a.S + s];
        t.x += p.x;
        t.y += p.y;
    }
    return t;
}

__device__ inline double member_mean(const Args& a, int32_t m, double* n_out) {
    const double2 t = member_total(a, a.part1, m);
    *n_out = t.x;
    return t.x > 0.0 ? t.y / t.x : 0.0;
}

__device__ inline MemberStats member_stats(const Args& a, int32_t m) {
    MemberStats st;
    st.mean = member_mean(a, m, &st.n);
    const double2 t2 = member_total(a, a.part2, m);
    st.std = st.n > 0.0 ? sqrt(t2.y / st.n) : 0.0;
    st.degenerate = !(st.n > 0.0 && st.std > 0.0);
    return st;
}

struct OutBlk {
    float x[BLK];
    uint8_t v[BLK];
};

__device__ inline OutBlk load_out(const Args& a, int k0, int i) {
    OutBlk b;
#pragma unroll
    for (int j = 0; j < BLK; ++j) {
        const int k = k0 + j;
        b.x[j] = k < a.K ? a.adv[at(a, k, i)] : 0.0f;
        b.v[j] = k < a.K ? a.valid[at(a, k, i)] : (uint8_t)0;
    }
    return b;
}

// sum2[i] = the env's sum of (x - mean)^2 over its valid samples, ascending k
__global__ void __launch_bounds__(THREADS) deviation_kernel(Args a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.B) return;
    double n;
    const double mean = member_mean(a, member_of(a, i), &n);
    double acc = 0.0;
    if (a.cnt[i] > 0) {
        OutBlk cur = load_out(a, 0, i);
        for (int k0 = 0; k0 < a.K; k0 += BLK) {
            OutBlk nxt = cur;
            if (k0 + BLK < a.K) nxt = load_out(a, k0 + BLK, i);
#pragma unroll
            for (int j = 0; j < BLK; ++j) {
                if (k0 + j < a.K && cur.v[j]) {
                    const double dx = (double)cur.x[j] - mean;
                    acc += dx * dx;
                }
            }
            cur = nxt;
        }
    }
    a.sum2[i] = acc;
}

// adv = (float)((x - mean) / std) on the valid samples (0 for a degenerate member); stats_out
__global__ void __launch_bounds__(THREADS) normalise_kernel(Args a) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (a.stats) {
        const int64_t all = (int64_t)gridDim.x * THREADS;
        for (int64_t m = t; m < a.P; m += all) {
            const MemberStats st = member_stats(a, (int32_t)m);
            double* o = a.stats + 4 * m;
            o[0] = st.n;
            o[1] = st.mean;
            o[2] = st.std;
            o[3] = st.degenerate ? 1.0 : 0.0;
        }
    }
    const int i = (int)t;
    if (t >= a.B || a.cnt[i] == 0) return;  // an env without a valid sample: its adv are 0 already
    const MemberStats st = member_stats(a, member_of(a, i));
    OutBlk cur = load_out(a, 0, i);
    for (int k0 = 0; k0 < a.K; k0 += BLK) {
        OutBlk nxt = cur;
        if (k0 + BLK < a.K) nxt = load_out(a, k0 + BLK, i);
#pragma unroll
        for (int j = 0; j < BLK; ++j) {
            const int k = k0 + j;
            if (k < a.K && cur.v[j])
                a.adv[at(a, k, i)] = st.degenerate ? 0.0f : (float)(((double)cur.x[j] - st.mean) / st.std);
        }
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host
struct Layout {
    int S;
    int64_t chunk, cnt_off, sum_off, sum2_off, part1_off, part2_off, bytes;
};

inline Layout layout(const cp_returns& p) {
    Layout l{};
    const int64_t B = p.num_envs, P = p.population > 1 ? p.population : 1, G = p.population > 1 ? p.group : 1;
    const int64_t longest = std::min<int64_t>(B, B / P + 2 * G);  // bound on a member's list
    l.S = (int)std::min<int64_t>(MAX_SLICES, std::max<int64_t>(1, (longest + SLICE_ENVS - 1) / SLICE_ENVS));
    l.chunk = (longest + l.S - 1) / l.S;
    auto up = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
    if (!(p.flags & CP_RET_STANDARDISE)) {
        l.bytes = 256;
        return l;
    }
    l.cnt_off = 0;
    l.sum_off = up(B * 4);
    l.sum2_off = l.sum_off + B * 8;
    l.part1_off = up(l.sum2_off + B * 8);
    l.part2_off = l.part1_off + P * l.S * 16;
    l.bytes = l.part2_off + P * l.S * 16;
    return l;
}

template <bool GAE>
inline void launch_scan(int boundary, dim3 grid, hipStream_t st, const Args& a) {
    switch (boundary) {
        case CP_RET_BOUNDARY_SAME_STEP:
            hipLaunchKernelGGL((scan_kernel<GAE, CP_RET_BOUNDARY_SAME_STEP>), grid, dim3(THREADS), 0, st, a);
            break;
        case CP_RET_BOUNDARY_STICKY:
            hipLaunchKernelGGL((scan_kernel<GAE, CP_RET_BOUNDARY_STICKY>), grid, dim3(THREADS), 0, st, a);
            break;
        default:
            hipLaunchKernelGGL((scan_kernel<GAE, CP_RET_BOUNDARY_NEXT_STEP>), grid, dim3(THREADS), 0, st, a);
    }
}

// every launch of one cp_returns_compute (the arguments are checked by the caller)
inline void launch(const cp_returns& p, Args a, void* scratch, hipStream_t st) {
    const Layout l = layout(p);
    char* base = static_cast<char*>(scratch);
    a.S = l.S;
    a.chunk = l.chunk;
    a.cnt = reinterpret_cast<int32_t*>(base + l.cnt_off);
    a.sum = reinterpret_cast<double*>(base + l.sum_off);
    a.sum2 = reinterpret_cast<double*>(base + l.sum2_off);
    a.part1 = reinterpret_cast<double2*>(base + l.part1_off);
    a.part2 = reinterpret_cast<double2*>(base + l.part2_off);
    const dim3 grid((unsigned)((a.B + THREADS - 1) / THREADS)), block(THREADS);
    if (p.kind == CP_RET_EPISODE_TOTAL) {
        switch (p.boundary) {
            case CP_RET_BOUNDARY_SAME_STEP:
                hipLaunchKernelGGL(total_forward_kernel<CP_RET_BOUNDARY_SAME_STEP>, grid, block, 0, st, a);
                break;
            case CP_RET_BOUNDARY_STICKY:
                hipLaunchKernelGGL(total_forward_kernel<CP_RET_BOUNDARY_STICKY>, grid, block, 0, st, a);
                break;
            default:
                hipLaunchKernelGGL(total_forward_kernel<CP_RET_BOUNDARY_NEXT_STEP>, grid, block, 0, st, a);
        }
        hipLaunchKernelGGL(total_backward_kernel, grid, block, 0, st, a);
    } else if (p.kind == CP_RET_GAE) {
        launch_scan<true>(p.boundary, grid, st, a);
    } else {
        launch_scan<false>(p.boundary, grid, st, a);
    }
    if (p.flags & CP_RET_STANDARDISE) {
        const dim3 rgrid((unsigned)((int64_t)a.P * a.S)), rblock(RED_THREADS);
        hipLaunchKernelGGL(member_reduce_kernel, rgrid, rblock, 0, st, a, (const double*)a.sum, a.part1);
        hipLaunchKernelGGL(deviation_kernel, grid, block, 0, st, a);
        hipLaunchKernelGGL(member_reduce_kernel, rgrid, rblock, 0, st, a, (const double*)a.sum2, a.part2);
        hipLaunchKernelGGL(normalise_kernel, grid, block, 0, st, a);
    }
}

}  // namespace cpret
