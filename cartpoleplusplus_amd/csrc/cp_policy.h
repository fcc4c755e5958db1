// cp_policy.h — the in-kernel dense ReLU MLP policy (cp_set_policy): the agents'
// observation -> small MLP -> action (lrpg_cartpole.py:149-163, ddpg_cartpole.py:121-138), evaluated by
// one lane per env by cp_policy_act_kernel.  fp32 only; included by cp_env.h inside namespace CP_NS.
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

// The layers of the MLP over the lane's scratch column (coff = env * 4 bytes): the input x[0 .. width[0]) is
// in half 0; returns the half that holds the last layer's (linear) outputs.
CP_DEV int policy_layers(const cpc::Pol& p, const SoaF& scr, uint32_t coff) {
    PolW w = (PolW)(uintptr_t)p.weights;
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

// One env's action from its obs row x[14 R] (unscaled), the caller's noise row (4 floats or null) and the
// env's counters before the step: writes actions_out[row] (float4 or char2) and returns the unit action
// a00 a01 a10 a11 the step scales by action_force.
template <int KIND>
CP_DEV void policy_act(const cpc::Pol& p, const SoaF& scr, uint32_t coff, const float* x, const float* noise, int steps,
                       int episode, uint64_t gid, void* actions_out, size_t row, float a[4]) {
    for (int i = 0; i < p.width[0]; ++i) scr.st(i, coff, x[i]);
    const int zo = policy_layers(p, scr, coff) * CP_POLICY_MAX_WIDTH;
    if constexpr (KIND == CP_ACTION_CONTINUOUS) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float z = scr.ld(zo + c, coff);
            if (p.head == CP_HEAD_TANH) z = tanhf(z);
            a[c] = fminf(fmaxf(z + (noise ? noise[c] : 0.0f), -1.0f), 1.0f);
        }
        reinterpret_cast<float4*>(actions_out)[row] = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        int idx[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float z[CP_NUM_DISCRETE];
#pragma unroll
            for (int j = 0; j < CP_NUM_DISCRETE; ++j) z[j] = scr.ld(zo + c * CP_NUM_DISCRETE + j, coff);
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

// cp_policy_act: one lane per env, policy_act on the caller's obs and the state's
// counters; an env that is done is not evaluated and gets a zero action.
template <int KIND>
__global__ void __launch_bounds__(WAVE) cp_policy_act_kernel(cp_config cfg, Bufs b, cpc::Pol pol) {
    const int B = cfg.num_envs;
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= B) return;
    const SoaT<float> st = SoaT<float>::make(b.state, B, CP_STATE_FIELDS);
    const uint32_t o = SoaT<float>::eoff(i);
    auto ldint = [&](int f) { return (int32_t)__float_as_uint(st.ld(f, o)); };
    if (ldint(CP_SF_DONE) != 0) {
        if constexpr (KIND == CP_ACTION_CONTINUOUS) reinterpret_cast<float4*>(pol.actions_out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else reinterpret_cast<char2*>(pol.actions_out)[i] = make_char2(0, 0);
        return;
    }
    const SoaF scr = SoaF::make(pol.scratch, B, 2 * CP_POLICY_MAX_WIDTH);
    float a[4];
    policy_act<KIND>(pol, scr, SoaF::eoff(i), pol.obs_in + (size_t)i * cfg.action_repeats * 14,
                     pol.noise ? pol.noise + (size_t)i * 4 : nullptr, ldint(CP_SF_STEPS), ldint(CP_SF_EPISODE),
                     (uint64_t)(cfg.env_id_offset + i), pol.actions_out, (size_t)i, a);
}
