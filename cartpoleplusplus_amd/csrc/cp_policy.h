// cp_policy.h — the in-kernel dense ReLU MLP policy (cp_set_policy): the agents'
// observation -> small MLP -> action (lrpg_cartpole.py:149-163, ddpg_cartpole.py:121-138), evaluated by
// one lane per env by cp_policy_act_kernel, or, for a policy population whose members change inside a wave, by
// one member run per wave (cp_policy_member_kernel, below).  With seeded ES perturbations on (cp_set_policy_es) the
// members are formed from one centre while they are staged (cp_policy_es_kernel, and the weights / gradient kernels
// at the end).  fp32 only; included by cp_env.h inside namespace CP_NS.
//
// The arithmetic order is part of the C-ABI's contract (include/cartpole_amd.h): per unit acc = b[j], then
// acc = fmaf(W[j][i], x[i], acc) for i ascending; hidden units max(acc, 0) as acc > 0 ? acc : 0.
//
// Weights are wave-uniform: they are read through the constant address space with indices built from
// kernel arguments and loop counters only (scalar loads), PB output units per activation load.
// Activations ping-pong between the two halves of a lane-private column of the policy scratch
// [2][CP_POLICY_MAX_WIDTH][B] in HBM (coalesced, each lane reads only its own writes, as the RC_* columns
// of cp_rollout): the throughput shape's LDS is full (8 waves x 20 KiB) and a lane's pool columns (80
// floats) cannot hold two consecutive 100-wide layers.

typedef const float __attribute__((address_space(4))) * PolW;
// the unit block: PB output units per activation load, PI inputs per trip of its inner loop
constexpr int PB = 16;
constexpr int PI = 4;
static_assert(PI > 0 && (PI & (PI - 1)) == 0, "PI: a power of two");

CP_DEV void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// In-kernel exploration noise of the continuous heads (cp_set_policy_noise; the arithmetic is spelled out in
// include/cartpole_amd.h and is part of the contract): one Philox block per evaluated env and step gives four
// Box-Muller normals g; GAUSSIAN x = sigma * g, OU x += theta * (-x), x += sigma * g on the env's state row
// (util.OrnsteinUhlenbeckNoise, one process per env and action component), then the clip.  The row [4] of
// noise_state is one 16-byte load (OU only) and one 16-byte store per lane, consecutive lanes on consecutive
// rows.  -ffp-contract=off: every product and sum below rounds on its own.
CP_DEV void policy_noise(const cpc::Pol& p, int steps, int episode, uint64_t gid, size_t row, float x[4]) {
    uint32_t w[4];
    philox4(0x80000000u + (uint32_t)steps, (uint32_t)episode, (uint32_t)gid, (uint32_t)(gid >> 32),
            (uint32_t)p.noise_seed, (uint32_t)(p.noise_seed >> 32), w);
    float g[4];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float u1 = (float)((w[2 * q] >> 8) + 1u) * 5.9604644775390625e-08f;  // (0, 1]
        const float u2 = (float)(w[2 * q + 1] >> 8) * 5.9604644775390625e-08f;     // [0, 1)
        const float r = sqrtf(-2.0f * logf(u1));
        const float t = 6.283185307179586f * u2;
        g[2 * q] = r * cosf(t);
        g[2 * q + 1] = r * sinf(t);
    }
    float4* const srow = reinterpret_cast<float4*>(p.noise_state) + row;
    if (p.noise_kind == CP_NOISE_OU) {
        const float4 s = *srow;
        x[0] = s.x; x[1] = s.y; x[2] = s.z; x[3] = s.w;
        const bool fresh = (p.noise_flags & CP_NOISE_RESET_ON_EPISODE) && steps == 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (fresh) x[c] = 0.0f;
            const float pull = p.noise_theta * (-x[c]);
            x[c] = x[c] + pull;
            const float push = p.noise_sigma * g[c];
            x[c] = x[c] + push;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = p.noise_sigma * g[c];
    }
    if (p.noise_max > 0.0f) {
        const float m = p.noise_max;
        const bool sym = (p.noise_flags & CP_NOISE_CLIP_SYMMETRIC) != 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (sym && x[c] < -m) x[c] = -m;
            if (x[c] > m) x[c] = m;  // the default bounds from above only (util.py:155's argument order)
        }
    }
    *srow = make_float4(x[0], x[1], x[2], x[3]);
}

// The layers of the MLP over the lane's scratch column (coff = env * 4 bytes), with the wave's weights woff
// floats into p.weights (wave-uniform: 0, or the wave's member of a population): the input x[0 .. width[0]) is
// in half 0; returns the half that holds the last layer's (linear) outputs.
CP_DEV int policy_layers(const cpc::Pol& p, uint64_t woff, const SoaF& scr, uint32_t coff) {
    PolW w = (PolW)(uintptr_t)(p.weights + woff);
    int half = 0;
    for (int l = 0; l < p.num_layers; ++l) {
        const int nin = p.width[l], nout = p.width[l + 1];
        const bool hidden = l + 1 < p.num_layers;
        PolW bias = w + nout * nin;
        const int src = half * CP_POLICY_MAX_WIDTH, dst = (half ^ 1) * CP_POLICY_MAX_WIDTH;
        for (int j0 = 0; j0 < nout; j0 += PB) {
            // rows past the layer's last unit repeat it (in-bounds, uniform); their sums are dropped
            int row[PB];
            float acc[PB];
#pragma unroll
            for (int u = 0; u < PB; ++u) {
                row[u] = (j0 + u < nout ? j0 + u : nout - 1);
                acc[u] = bias[row[u]];
                row[u] *= nin;
            }
            // PI inputs per trip, the next trip's loaded before this trip's FMAs (a lone load's latency per
            // input would be the whole cost); per unit the FMAs still run i ascending
            const int nfull = nin & ~(PI - 1);
            float xc[PI];
            if (nfull) {
#pragma unroll
                for (int k = 0; k < PI; ++k) xc[k] = scr.ld(src + k, coff);
            }
            for (int i = 0; i < nfull; i += PI) {
                const int inext = i + PI < nfull ? i + PI : i;  // the last trip reloads itself (in bounds, unused)
                float xn[PI];
#pragma unroll
                for (int k = 0; k < PI; ++k) xn[k] = scr.ld(src + inext + k, coff);
#pragma unroll
                for (int u = 0; u < PB; ++u) {
#pragma unroll
                    for (int k = 0; k < PI; ++k) acc[u] = __builtin_fmaf(w[row[u] + i + k], xc[k], acc[u]);
                }
#pragma unroll
                for (int k = 0; k < PI; ++k) xc[k] = xn[k];
            }
            for (int i = nfull; i < nin; ++i) {
                const float x = scr.ld(src + i, coff);
#pragma unroll
                for (int u = 0; u < PB; ++u) acc[u] = __builtin_fmaf(w[row[u] + i], x, acc[u]);
            }
#pragma unroll
            for (int u = 0; u < PB; ++u)
                if (j0 + u < nout) scr.st(dst + j0 + u, coff, hidden ? (acc[u] > 0.0f ? acc[u] : 0.0f) : acc[u]);
        }
        w = bias + nout;
        half ^= 1;
    }
    return half;
}

// The head on one env's last-layer outputs zv(0 .. 3) (continuous) or zv(0 .. 9) (discrete; zv reads the z vector
// where the kernel keeps it: the scratch column or the LDS tile), the caller's noise row (4 floats or null; with
// in-kernel noise on, policy_noise's draw on the env's state row instead) and the env's counters before the step:
// writes actions_out[row] (float4 or char2) and returns the unit action a00 a01 a10 a11 the step scales by
// action_force.  Shared by both kernels.
template <int KIND, typename Z>
CP_DEV void policy_head(const cpc::Pol& p, const Z& zv, const float* noise, int steps, int episode, uint64_t gid,
                        void* actions_out, size_t row, float a[4]) {
    if constexpr (KIND == CP_ACTION_CONTINUOUS) {
        float n[4];
        if (p.noise_kind != CP_NOISE_OFF) {
            policy_noise(p, steps, episode, gid, row, n);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) n[c] = noise ? noise[c] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float z = zv(c);
            if (p.head == CP_HEAD_TANH) z = tanhf(z);
            a[c] = fminf(fmaxf(z + n[c], -1.0f), 1.0f);
        }
        reinterpret_cast<float4*>(actions_out)[row] = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        int idx[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float z[CP_NUM_DISCRETE];
#pragma unroll
            for (int j = 0; j < CP_NUM_DISCRETE; ++j) z[j] = zv(c * CP_NUM_DISCRETE + j);
            int best = 0;
            float m = z[0];
#pragma unroll
            for (int j = 1; j < CP_NUM_DISCRETE; ++j)
                if (z[j] > m) {
                    m = z[j];
                    best = j;
                }
            if (p.head == CP_HEAD_SAMPLE) {  // lrpg's epsilon-greedy multinomial (lrpg_cartpole.py:132-146)
                uint32_t w[4];
                philox4(0x40000000u + 2u * (uint32_t)steps + (uint32_t)c, (uint32_t)episode, (uint32_t)gid,
                        (uint32_t)(gid >> 32), (uint32_t)p.seed, (uint32_t)(p.seed >> 32), w);
                const float u0 = (float)(w[0] >> 8) * 5.9604644775390625e-08f;
                if (u0 < p.epsilon) {
                    best = (int)(((w[1] >> 8) * 5u) >> 24);
                } else {
                    const float u2 = (float)(w[2] >> 8) * 5.9604644775390625e-08f;
                    float e[CP_NUM_DISCRETE], S = 0.0f;
#pragma unroll
                    for (int j = 0; j < CP_NUM_DISCRETE; ++j) {
                        e[j] = expf(z[j] - m);
                        S = j ? S + e[j] : e[j];
                    }
                    const float t = u2 * S;
                    float run = 0.0f;  // the smallest index whose running sum (S's partial sums) exceeds t
                    bool found = false;
                    best = CP_NUM_DISCRETE - 1;
#pragma unroll
                    for (int j = 0; j < CP_NUM_DISCRETE; ++j) {
                        run = j ? run + e[j] : e[j];
                        if (!found && run > t) {
                            best = j;
                            found = true;
                        }
                    }
                }
            }
            idx[c] = best;
        }
        reinterpret_cast<char2*>(actions_out)[row] = make_char2((signed char)idx[0], (signed char)idx[1]);
        a[0] = kDiscrete[idx[0]][0]; a[1] = kDiscrete[idx[0]][1];
        a[2] = kDiscrete[idx[1]][0]; a[3] = kDiscrete[idx[1]][1];
    }
}

// One env's action from its obs row x[14 R] (unscaled) by the lane-per-env layers and the head.
template <int KIND>
CP_DEV void policy_act(const cpc::Pol& p, uint64_t woff, const SoaF& scr, uint32_t coff, const float* x, const float* noise,
                       int steps, int episode, uint64_t gid, void* actions_out, size_t row, float a[4]) {
    for (int i = 0; i < p.width[0]; ++i) scr.st(i, coff, x[i]);
    const int zo = policy_layers(p, woff, scr, coff) * CP_POLICY_MAX_WIDTH;
    policy_head<KIND>(p, [&](int j) { return scr.ld(zo + j, coff); }, noise, steps, episode, gid, actions_out, row, a);
}

template <int KIND>
CP_DEV void policy_zero_action(void* actions_out, size_t row) {
    if constexpr (KIND == CP_ACTION_CONTINUOUS) reinterpret_cast<float4*>(actions_out)[row] = make_float4(0.f, 0.f, 0.f, 0.f);
    else reinterpret_cast<char2*>(actions_out)[row] = make_char2(0, 0);
}

// cp_policy_act, one lane per env: policy_act on the caller's obs and the state's counters; an env that is done
// is not evaluated and gets a zero action.  POP (cps::POLICY_WAVE): a population whose members change at wave
// boundaries only; the wave's member comes from the block index and kernel arguments, through readfirstlane, so
// the weight base is wave-uniform to the compiler and the weight loads stay scalar.
template <int KIND, bool POP>
__global__ void __launch_bounds__(WAVE) cp_policy_act_kernel(cp_config cfg, Bufs b, cpc::Pol pol) {
    const int B = cfg.num_envs;
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= B) return;
    const SoaT<float> st = SoaT<float>::make(b.state, B, CP_STATE_FIELDS);
    const uint32_t o = SoaT<float>::eoff(i);
    auto ldint = [&](int f) { return (int32_t)__float_as_uint(st.ld(f, o)); };
    if (ldint(CP_SF_DONE) != 0) {
        policy_zero_action<KIND>(pol.actions_out, (size_t)i);
        return;
    }
    uint64_t woff = 0;
    if constexpr (POP) {
        const uint64_t g0 = (uint64_t)cfg.env_id_offset + (uint64_t)blockIdx.x * WAVE;  // the wave's first global id
        const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)(uint32_t)((g0 / (uint32_t)pol.group) % (uint32_t)pol.population));
        woff = (uint64_t)m * (uint64_t)pol.floats;  // added to the 64-bit base: member * F * 4 bytes passes 4 GiB
    }
    const SoaF scr = SoaF::make(pol.scratch, B, 2 * CP_POLICY_MAX_WIDTH);
    float a[4];
    policy_act<KIND>(pol, woff, scr, SoaF::eoff(i), pol.obs_in + (size_t)i * cfg.action_repeats * 14,
                     pol.noise ? pol.noise + (size_t)i * 4 : nullptr, ldint(CP_SF_STEPS), ldint(CP_SF_EPISODE),
                     (uint64_t)(cfg.env_id_offset + i), pol.actions_out, (size_t)i, a);
}

// ---- the member path (cps::POLICY_MEMBER): one member run's chunk of n <= 64 envs per wave -------------------
// A wave's lanes would belong to several members, so the lane-per-env kernel would read 64 weight sets per load.
// Here the lanes are the layer's output units (two passes at widths above 64) and the chunk's envs are the loop:
//   * the chunk's activations are two LDS tiles [unit][env] with env stride ES (cps::policy_env_stride), so the
//     envs e0 .. e0+3 of one input unit are one 16-byte broadcast read;
//   * a layer's W and b come from HBM once per chunk, as 16-byte loads over the contiguous [W | b] range (dword
//     loads for the at most 6 floats before and after the 16-byte aligned part), into LDS at row stride nin | 1:
//     lane j's read of W[j][i] then meets 32 distinct banks;
//   * per (env, unit) acc = b[j] and the FMAs run i ascending, as in policy_layers: the same bits.
// Element f of the [W | b] range lands at (f / nin) * stride + f % nin, the bias rows continuing W's grid.
CP_DEV void member_stage_weights(const float* src, int nin, int nout, float* wl, int lane) {
    const int stride = nin | 1, total = nout * nin + nout;
    int head = (int)((0u - (uint32_t)((uintptr_t)src >> 2)) & 3u);  // floats up to the 16-byte boundary
    head = head < total ? head : total;
    const int nvec = (total - head) >> 2, tail0 = head + 4 * nvec;
    if (lane < head + total - tail0) {
        const int f = lane < head ? lane : tail0 + (lane - head);
        const int j = f / nin;
        wl[j * stride + (f - j * nin)] = src[f];
    }
    const float4* src4 = reinterpret_cast<const float4*>(src + head);
    const int q = (4 * WAVE) / nin, r = 4 * WAVE - q * nin;  // a wave-wide load advances a lane by 256 floats
    const int f0 = head + 4 * lane;
    int j = f0 / nin, i = f0 - j * nin;
    constexpr int U = 8;  // 16-byte loads in flight per lane before the LDS writes
    for (int v0 = lane; v0 - lane < nvec; v0 += U * WAVE) {
        float4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (v0 + u * WAVE < nvec) x[u] = src4[v0 + u * WAVE];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (v0 + u * WAVE < nvec) {
                const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
                int jj = j, ii = i;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    wl[jj * stride + ii] = e[k];
                    if (++ii >= nin) {
                        ii = 0;
                        ++jj;
                    }
                }
            }
            i += r;
            j += q;
            if (i >= nin) {
                i -= nin;
                ++j;
            }
        }
    }
}

// Unit j's outputs for the envs e0 .. e0+E-1 of the chunk (columns past the chunk's last env hold don't-cares
// inside the tile, computed and never read out)
template <int E>
CP_DEV void member_block(const float* wrow, float bias, const float* xs, float* out, int ES, int nin, bool hidden,
                         bool store) {
    float acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = bias;
#pragma unroll 4
    for (int i = 0; i < nin; ++i) {
        const float w = wrow[i];
#pragma unroll
        for (int k = 0; k < E; k += 4) {
            const float4 x = *reinterpret_cast<const float4*>(xs + i * ES + k);
            acc[k + 0] = __builtin_fmaf(w, x.x, acc[k + 0]);
            acc[k + 1] = __builtin_fmaf(w, x.y, acc[k + 1]);
            acc[k + 2] = __builtin_fmaf(w, x.z, acc[k + 2]);
            acc[k + 3] = __builtin_fmaf(w, x.w, acc[k + 3]);
        }
    }
    if (!store) return;
#pragma unroll
    for (int k = 0; k < E; ++k)
        if (hidden) acc[k] = acc[k] > 0.0f ? acc[k] : 0.0f;
#pragma unroll
    for (int k = 0; k < E; k += 4)
        *reinterpret_cast<float4*>(out + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
}

// ---- seeded ES perturbations (cp_set_policy_es; the arithmetic is spelled out in include/cartpole_amd.h and is
// part of the contract): member m's weights are theta + s sigma eps(e, f), eps from one Philox word per parameter.
constexpr float kEsK = 0x1.bb688cp-8f;  // the float32 nearest to 21845^(-1/2)
struct EsMember {
    uint64_t e;  // the draw: m >> 1 with ANTITHETIC, else m
    bool neg;    // s = -1: odd m with ANTITHETIC
};
CP_DEV EsMember es_member(const cpc::PolEs& es, uint64_t m) {
    const bool anti = (es.flags & CP_ES_ANTITHETIC) != 0;
    return {anti ? m >> 1 : m, anti && (m & 1u)};
}
// The four words of Philox block blk: the parameters 4 blk .. 4 blk + 3.  philox4's rounds with each 32 x 32
// product written as one 64-bit multiply (a single v_mad_u64_u32 instead of a lo / hi pair: the draw is most of
// what the ES kernels do, and those multiplies are most of the draw); the same words.
CP_DEV void es_words(const cpc::PolEs& es, uint64_t e, uint32_t blk, uint32_t w[4]) {
    uint32_t c0 = 0xC0000000u + blk, c1 = es.generation, c2 = (uint32_t)e, c3 = (uint32_t)(e >> 32);
    uint32_t k0 = (uint32_t)es.seed, k1 = (uint32_t)(es.seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
CP_DEV float es_epsilon(uint32_t w) {
    const uint32_t S = __builtin_amdgcn_sad_u8(w, 0u, 0u);  // the sum of the four bytes, one instruction
    return ((float)S - 510.0f) * kEsK;
}
CP_DEV float es_weight(float theta, float eps, float sigma, bool neg) {
    const float d = sigma * eps;
    return neg ? theta - d : theta + d;
}

// The ES form of member_stage_weights: the layer's [W | b] range is the parameters [fbase, fbase + total) of
// member m, formed from the centre (cache resident, read by dword loads: it may start at any multiple of
// 4 bytes) and written to the same LDS image.  A lane takes whole Philox blocks, so the first and last block of a
// layer are partial.  The next block's four centre floats are loaded before this block's draw, from addresses
// clamped into the layer (loaded and dropped outside it): a load waited for per element was most of the kernel's
// time.  The LDS position is carried from block to block (a wave-wide trip advances a lane by 256 floats), as in
// member_stage_weights.
CP_DEV void es_stage_weights(const cpc::PolEs& es, uint64_t m, const float* theta, int fbase, int nin, int nout,
                             float* wl, int lane) {
    const int pad = (nin | 1) - nin, total = nout * nin + nout;
    const EsMember mem = es_member(es, m);
    const float* th = theta + fbase;
    const int blk1 = (fbase + total - 1) >> 2;
    int blk = (fbase >> 2) + lane;
    if (blk > blk1) return;
    auto load = [&](int lf, float x[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = lf + k < 0 ? 0 : lf + k;
            x[k] = th[f < total ? f : total - 1];
        }
    };
    int lf = 4 * blk - fbase;  // the block's first parameter within the layer: -3 .. total - 1
    // column i and LDS index a = row * stride + i of parameter lf; a block that starts before the layer counts
    // up to (0, 0) from i = a = lf < 0
    int i = lf, a = lf;
    if (lf >= 0) {
        const int j = lf / nin;
        i = lf - j * nin;
        a = lf + j * pad;
    }
    const int q = (4 * WAVE) / nin, r = 4 * WAVE - q * nin, qa = 4 * WAVE + q * pad;
    float x[4];
    load(lf, x);
    for (; blk <= blk1; blk += WAVE) {
        float xn[4];
        load(lf + 4 * WAVE, xn);
        uint32_t w[4];
        es_words(es, mem.e, (uint32_t)blk, w);
        int ii = i, aa = a;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lf + k >= 0 && lf + k < total) wl[aa] = es_weight(x[k], es_epsilon(w[k]), es.sigma, mem.neg);
            ++aa;
            if (++ii >= nin) {
                ii = 0;
                aa += pad;
            }
        }
        lf += 4 * WAVE;
        i += r;
        a += qa;
        while (i < 0) {  // only after a block that started before the layer
            i += nin;
            a -= pad;
        }
        if (i >= nin) {
            i -= nin;
            a += pad;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = xn[k];
    }
}

template <int KIND>
__global__ void __launch_bounds__(WAVE) cp_policy_member_kernel(cp_config cfg, Bufs b, cpc::Pol pol, cps::PolicyRuns runs) {
    extern __shared__ float4 policy_lds[];
    float* const lds = reinterpret_cast<float*>(policy_lds);
    const int B = cfg.num_envs, lane = threadIdx.x;
    const cps::PolicyChunk ch = cps::policy_chunk(cfg.env_id_offset, pol.group, pol.population, B, runs, (int)blockIdx.x);
    const int n = ch.n, row = ch.lo + lane;
    if (n <= 0) return;  // a short first or last run's trailing chunk (the whole wave leaves)
    const bool mine = lane < n;
    const SoaT<float> st = SoaT<float>::make(b.state, B, CP_STATE_FIELDS);
    const uint32_t o = SoaT<float>::eoff(mine ? row : ch.lo);
    auto ldint = [&](int f) { return (int32_t)__float_as_uint(st.ld(f, o)); };
    const bool live = mine && ldint(CP_SF_DONE) == 0;
    if (mine && !live) policy_zero_action<KIND>(pol.actions_out, (size_t)row);
    if (__builtin_amdgcn_ballot_w64(live) == 0) return;  // every env of the chunk is done

    int amax = 0;
    for (int l = 0; l <= pol.num_layers; ++l) amax = pol.width[l] > amax ? pol.width[l] : amax;
    const int ES = cps::policy_env_stride(pol.group, B), tile = amax * ES;
    float* const wl = lds + 2 * tile;
    {   // the chunk's obs rows (contiguous in obs_in) into tile 0, transposed to [unit][env]
        const int nin = pol.width[0], total = n * nin;
        const float* obs = pol.obs_in + (size_t)ch.lo * nin;
        for (int f = lane; f < total; f += WAVE) {
            const int e = f / nin;
            lds[(f - e * nin) * ES + e] = obs[f];
        }
    }
    const float* wsrc = pol.weights + (uint64_t)ch.member * (uint64_t)pol.floats;  // 64-bit: passes 4 GiB
    int half = 0;
    for (int l = 0; l < pol.num_layers; ++l) {
        const int nin = pol.width[l], nout = pol.width[l + 1], stride = nin | 1;
        const bool hidden = l + 1 < pol.num_layers;
        member_stage_weights(wsrc, nin, nout, wl, lane);
        __syncthreads();
        const float* src = lds + half * tile;
        float* dst = lds + (half ^ 1) * tile;
        for (int jb = 0; jb < nout; jb += WAVE) {
            const bool store = jb + lane < nout;
            const int j = store ? jb + lane : nout - 1;  // lanes past the last unit repeat it, unstored
            const int fb = nout * nin + j, jbias = fb / nin;
            const float bias = wl[jbias * stride + (fb - jbias * nin)];
            const float* wrow = wl + j * stride;
            int e0 = 0;
            for (; e0 + 4 < n; e0 += 16) member_block<16>(wrow, bias, src + e0, dst + j * ES + e0, ES, nin, hidden, store);
            for (; e0 < n; e0 += 4) member_block<4>(wrow, bias, src + e0, dst + j * ES + e0, ES, nin, hidden, store);
        }
        __syncthreads();
        wsrc += nout * nin + nout;
        half ^= 1;
    }
    if (!live) return;
    const float* zt = lds + half * tile + lane;  // the last layer's tile: unit j of this lane's env
    float a[4];
    policy_head<KIND>(pol, [&](int j) { return zt[j * ES]; }, pol.noise ? pol.noise + (size_t)row * 4 : nullptr, ldint(CP_SF_STEPS), ldint(CP_SF_EPISODE),
                      (uint64_t)(cfg.env_id_offset + row), pol.actions_out, (size_t)row, a);
}

// cp_policy_act with ES on, for every G and offset (the lane-per-env kernels read weights by scalar loads and
// cannot perturb them): cp_policy_member_kernel with the ES struct's P and G and es_stage_weights where that one
// loads a member's weights.  A copy, not a shared body: the population kernel's device code stays what it was.
template <int KIND>
__global__ void __launch_bounds__(WAVE) cp_policy_es_kernel(cp_config cfg, Bufs b, cpc::Pol pol, cpc::PolEs es,
                                                            cps::PolicyRuns runs) {
    extern __shared__ float4 policy_lds[];
    float* const lds = reinterpret_cast<float*>(policy_lds);
    const int B = cfg.num_envs, lane = threadIdx.x;
    const cps::PolicyChunk ch = cps::policy_chunk(cfg.env_id_offset, es.group, es.population, B, runs, (int)blockIdx.x);
    const int n = ch.n, row = ch.lo + lane;
    if (n <= 0) return;  // a short first or last run's trailing chunk (the whole wave leaves)
    const bool mine = lane < n;
    const SoaT<float> st = SoaT<float>::make(b.state, B, CP_STATE_FIELDS);
    const uint32_t o = SoaT<float>::eoff(mine ? row : ch.lo);
    auto ldint = [&](int f) { return (int32_t)__float_as_uint(st.ld(f, o)); };
    const bool live = mine && ldint(CP_SF_DONE) == 0;
    if (mine && !live) policy_zero_action<KIND>(pol.actions_out, (size_t)row);
    if (__builtin_amdgcn_ballot_w64(live) == 0) return;  // every env of the chunk is done

    int amax = 0;
    for (int l = 0; l <= pol.num_layers; ++l) amax = pol.width[l] > amax ? pol.width[l] : amax;
    const int ES = cps::policy_env_stride(es.group, B), tile = amax * ES;
    float* const wl = lds + 2 * tile;
    {   // the chunk's obs rows (contiguous in obs_in) into tile 0, transposed to [unit][env]
        const int nin = pol.width[0], total = n * nin;
        const float* obs = pol.obs_in + (size_t)ch.lo * nin;
        for (int f = lane; f < total; f += WAVE) {
            const int e = f / nin;
            lds[(f - e * nin) * ES + e] = obs[f];
        }
    }
    int fbase = 0;  // the layer's first parameter index
    int half = 0;
    for (int l = 0; l < pol.num_layers; ++l) {
        const int nin = pol.width[l], nout = pol.width[l + 1], stride = nin | 1;
        const bool hidden = l + 1 < pol.num_layers;
        es_stage_weights(es, (uint64_t)ch.member, pol.weights, fbase, nin, nout, wl, lane);
        __syncthreads();
        const float* src = lds + half * tile;
        float* dst = lds + (half ^ 1) * tile;
        for (int jb = 0; jb < nout; jb += WAVE) {
            const bool store = jb + lane < nout;
            const int j = store ? jb + lane : nout - 1;  // lanes past the last unit repeat it, unstored
            const int fb = nout * nin + j, jbias = fb / nin;
            const float bias = wl[jbias * stride + (fb - jbias * nin)];
            const float* wrow = wl + j * stride;
            int e0 = 0;
            for (; e0 + 4 < n; e0 += 16) member_block<16>(wrow, bias, src + e0, dst + j * ES + e0, ES, nin, hidden, store);
            for (; e0 < n; e0 += 4) member_block<4>(wrow, bias, src + e0, dst + j * ES + e0, ES, nin, hidden, store);
        }
        __syncthreads();
        fbase += nout * nin + nout;
        half ^= 1;
    }
    if (!live) return;
    const float* zt = lds + half * tile + lane;  // the last layer's tile: unit j of this lane's env
    float a[4];
    policy_head<KIND>(pol, [&](int j) { return zt[j * ES]; }, pol.noise ? pol.noise + (size_t)row * 4 : nullptr, ldint(CP_SF_STEPS), ldint(CP_SF_EPISODE),
                      (uint64_t)(cfg.env_id_offset + row), pol.actions_out, (size_t)row, a);
}

#ifdef CP_POLICY  // not templates, so every includer would emit them: the fp32 translation unit only
// cp_policy_es_weights: one thread per (member, Philox block) of the members [lo, lo + count), out [count][F]
__global__ void __launch_bounds__(256) cp_policy_es_weights_kernel(cpc::PolEs es, const float* theta, int F, int64_t lo,
                                                                   int count, float* out) {
    const int nblk = (F + 3) >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)count * nblk) return;
    const int mi = (int)(t / nblk), blk = (int)(t - (int64_t)mi * nblk);
    const EsMember mem = es_member(es, (uint64_t)(lo + mi));
    uint32_t w[4];
    es_words(es, mem.e, (uint32_t)blk, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int f = 4 * blk + k;
        if (f < F) out[(size_t)mi * F + f] = es_weight(theta[f], es_epsilon(w[k]), es.sigma, mem.neg);
    }
}

// cp_policy_es_gradient, first stage: one thread per (Philox block, member slice) sums its slice's
// coeff * s * eps in registers, draws ascending, into partial[slice][F].  With ANTITHETIC a draw e serves the
// members 2e and 2e + 1 with c = c_2e - c_2e+1 (a member outside [lo, lo + count) counts 0).
__global__ void __launch_bounds__(256) cp_policy_es_gradient_kernel(cpc::PolEs es, int F, int64_t lo, int count,
                                                                    const float* coeff, float* partial) {
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (4 * blk >= F) return;
    const bool anti = (es.flags & CP_ES_ANTITHETIC) != 0;
    const int64_t hi = lo + count;
    const int64_t e_lo = anti ? lo >> 1 : lo, e_hi = anti ? (hi + 1) >> 1 : hi;  // the draws [e_lo, e_hi)
    const int64_t per = (e_hi - e_lo + gridDim.y - 1) / gridDim.y;
    const int64_t a = e_lo + (int64_t)blockIdx.y * per, z = a + per < e_hi ? a + per : e_hi;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t e = a; e < z; ++e) {
        float c;
        if (anti) {
            const float c0 = 2 * e >= lo ? coeff[2 * e - lo] : 0.0f, c1 = 2 * e + 1 < hi ? coeff[2 * e + 1 - lo] : 0.0f;
            c = c0 - c1;
        } else {
            c = coeff[e - lo];
        }
        uint32_t w[4];
        es_words(es, (uint64_t)e, (uint32_t)blk, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = c * es_epsilon(w[k]);
            acc[k] = acc[k] + t;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * blk + k < F) partial[(size_t)blockIdx.y * F + 4 * blk + k] = acc[k];
}

// second stage: the slices' partial sums in slice order (no atomics: equal calls give equal bits)
__global__ void __launch_bounds__(256) cp_policy_es_reduce_kernel(int F, int slices, const float* partial, float* grad) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float g = partial[f];
    for (int s = 1; s < slices; ++s) g = g + partial[(size_t)s * F + f];
    grad[f] = g;
}
#endif  // CP_POLICY
