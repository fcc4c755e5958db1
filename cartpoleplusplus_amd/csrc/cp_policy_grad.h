// cp_policy_grad.h — cp_policy_gradient: the likelihood-ratio gradient of the discrete MLP policy over a window of
// samples, per population member (C-ABI and the arithmetic contract: include/cartpole_amd.h; DESIGN.md §9.5
// "Policy gradient").  fp32 only; included by cp_kernels.hip after cp_env.h, whose namespace cp holds member_block.
//
// A block of 256 threads takes tiles of up to 64 samples of one member (cps::policy_grad_tile) and keeps, per tile,
// every layer's inputs in LDS as [unit][sample] tiles with sample stride ES, each followed by a row of ones (the
// bias's input), then the logits' tile, then one layer's [W | b] image as cp_policy_member_kernel lays it out:
//   forward   member_block<16> per (unit, 16 samples): cp_policy_act's bits.  A skipped sample's column holds
//             zeros, so it stays finite and its deltas are zero: it adds +-0 everywhere.
//   head      one thread per sample: logits_out, logp_out, and dz over the logits in place
//   backward  per layer, last to first: dW = delta x^T over the tile as 4 x 4 register patches (the ones row gives
//             db), added to the block's own partial [F] in the scratch by the thread that owns the patch in every
//             tile; then delta_in = relu'(x) W^T delta over the layer's input tile in place.
// A second kernel adds a member's partials in partial order.  No floating-point atomics: the order of every sum is
// a function of the plan alone.
#pragma once

namespace cp {

constexpr int PG_THREADS = cps::kPolicyGradThreads;

struct PolGrad {
    const float* obs;       // [K][B][nin]
    const int8_t* actions;  // [K][B][2]
    const float* coeff;     // [K][B]
    float* logits;          // [K][B][10] or null
    float* logp;            // [K][B] or null
    float* partial;         // [slices][P][F]
};

CP_DEV void pg_stage_weights(const float* src, int nin, int nout, float* wl, int tid) {
    const int stride = nin | 1, total = nout * nin + nout;
    for (int f = tid; f < total; f += PG_THREADS) {
        const int j = f / nin;
        wl[j * stride + (f - j * nin)] = src[f];
    }
}

// delta_in of input unit i for the samples e0 .. e0+E-1, in place over the input tile's row (x > 0 is the forward
// pass's acc > 0): wcol = wl + i, d = the layer's output deltas + e0
template <int E>
CP_DEV void pg_back_block(const float* wcol, int stride, const float* d, float* x, int ES, int nout) {
    float acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = 0.0f;
#pragma unroll 4
    for (int j = 0; j < nout; ++j) {
        const float w = wcol[j * stride];
#pragma unroll
        for (int k = 0; k < E; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(d + j * ES + k);
            acc[k + 0] = __builtin_fmaf(w, v.x, acc[k + 0]);
            acc[k + 1] = __builtin_fmaf(w, v.y, acc[k + 1]);
            acc[k + 2] = __builtin_fmaf(w, v.z, acc[k + 2]);
            acc[k + 3] = __builtin_fmaf(w, v.w, acc[k + 3]);
        }
    }
#pragma unroll
    for (int k = 0; k < E; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(x + k);
        *reinterpret_cast<float4*>(x + k) = make_float4(v.x > 0.0f ? acc[k] : 0.0f, v.y > 0.0f ? acc[k + 1] : 0.0f,
                                                        v.z > 0.0f ? acc[k + 2] : 0.0f, v.w > 0.0f ? acc[k + 3] : 0.0f);
    }
}

// The 4 x 4 patch (units 4 jb .., inputs 4 ib .., input nin being the ones row: db) of delta x^T over the tile's T
// samples, added to the layer's packed [W | b] range g of the block's partial.  Rows past the last repeat it
// (in bounds) and are dropped.
CP_DEV void pg_dw_patch(const float* d, const float* x, int ES, int T, int nin, int nout, int jb, int ib, float* g) {
    int jr[4], ir[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        jr[a] = (4 * jb + a < nout ? 4 * jb + a : nout - 1) * ES;
        ir[a] = (4 * ib + a <= nin ? 4 * ib + a : nin) * ES;
    }
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0f;
    for (int e = 0; e < T; e += 4) {
        float4 dv[4], xv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            dv[a] = *reinterpret_cast<const float4*>(d + jr[a] + e);
            xv[a] = *reinterpret_cast<const float4*>(x + ir[a] + e);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float s = acc[a][c];
                s = __builtin_fmaf(dv[a].x, xv[c].x, s);
                s = __builtin_fmaf(dv[a].y, xv[c].y, s);
                s = __builtin_fmaf(dv[a].z, xv[c].z, s);
                s = __builtin_fmaf(dv[a].w, xv[c].w, s);
                acc[a][c] = s;
            }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int j = 4 * jb + a;
        if (j >= nout) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = 4 * ib + c;
            if (i > nin) continue;
            float* const p = g + (i < nin ? j * nin + i : nout * nin + j);
            *p = *p + acc[a][c];
        }
    }
}

__global__ void __launch_bounds__(PG_THREADS) cp_policy_grad_kernel(cpc::Pol pol, cps::PolicyGrad pg, PolGrad a) {
    extern __shared__ float4 policy_grad_lds[];
    __shared__ int64_t col_idx[64];  // the column's sample k * B + i, or -1: skipped, or past the tile's last
    __shared__ float col_coeff[64];
    __shared__ int col_act[64][2];
    float* const lds = reinterpret_cast<float*>(policy_grad_lds);
    const int tid = threadIdx.x, L = pol.num_layers, F = (int)pol.floats;
    const int T = pg.tile, ES = pg.es;
    const int m = (int)(blockIdx.x / (unsigned)pg.slices), slice = (int)(blockIdx.x - (unsigned)m * (unsigned)pg.slices);
    float* const part = a.partial + ((size_t)slice * (size_t)pg.P + (size_t)m) * (size_t)F;
    for (int f = tid; f < F; f += PG_THREADS) part[f] = 0.0f;

    float* const wl = lds + pg.rows * ES;
    int row0[CP_POLICY_MAX_LAYERS + 1];  // the first LDS row of layer l's input tile; [L]: the logits' tile
    {
        int r = 0;
        for (int l = 0; l <= CP_POLICY_MAX_LAYERS; ++l) {
            row0[l] = r;
            if (l < L) {
                r += pol.width[l] + 1;
                for (int e = tid; e < T; e += PG_THREADS) lds[(r - 1) * ES + e] = 1.0f;  // the ones row, written once
            }
        }
    }
    float* const zt = lds + row0[L] * ES;
    const float* const wmem = pol.weights + (uint64_t)m * (uint64_t)pol.floats;
    __syncthreads();  // the partial's zeros, before another thread adds to them

    const int64_t tiles = cps::policy_grad_member_tiles(pg, m);
    const int64_t per = (tiles + pg.slices - 1) / pg.slices;
    const int64_t t_lo = (int64_t)slice * per, t_hi = t_lo + per < tiles ? t_lo + per : tiles;
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const cps::PolicyGradTile tl = cps::policy_grad_tile(pg, m, t);
        bool valid = false;
        if (tid < T) {
            int64_t idx = -1;
            float c = 0.0f;
            int a0 = 0, a1 = 0;
            if (tid < tl.n) {
                const uint32_t s = (uint32_t)tl.s0 + (uint32_t)tid, k = s / (uint32_t)tl.len;
                const int64_t gi = (int64_t)k * pg.B + tl.lo + (int)(s - k * (uint32_t)tl.len);
                c = a.coeff[gi];
                a0 = a.actions[2 * gi];
                a1 = a.actions[2 * gi + 1];
                valid = c != 0.0f && a0 >= 0 && a0 < CP_NUM_DISCRETE && a1 >= 0 && a1 < CP_NUM_DISCRETE;
                if (valid) {
                    idx = gi;
                } else {
                    if (a.logp) a.logp[gi] = 0.0f;
                    if (a.logits)
                        for (int j = 0; j < 2 * CP_NUM_DISCRETE; ++j) a.logits[gi * (2 * CP_NUM_DISCRETE) + j] = 0.0f;
                }
            }
            col_idx[tid] = idx;
            col_coeff[tid] = valid ? c : 0.0f;
            col_act[tid][0] = a0;
            col_act[tid][1] = a1;
        }
        if (!__syncthreads_or(valid)) continue;  // every sample of the tile is skipped (the whole block moves on)

        {   // the samples' obs rows into the first tile, transposed to [unit][sample]; zeros in skipped columns
            const int nin = pol.width[0];
            for (int f = tid; f < T * nin; f += PG_THREADS) {
                const int e = f / nin, i = f - e * nin;
                const int64_t gi = col_idx[e];
                lds[i * ES + e] = gi >= 0 ? a.obs[gi * nin + i] : 0.0f;
            }
        }
        const float* wsrc = wmem;
        for (int l = 0; l < L; ++l) {
            const int nin = pol.width[l], nout = pol.width[l + 1], stride = nin | 1;
            const bool hidden = l + 1 < L;
            pg_stage_weights(wsrc, nin, nout, wl, tid);
            __syncthreads();
            const float* src = lds + row0[l] * ES;
            float* dst = lds + row0[l + 1] * ES;
            for (int w = tid; w < nout * (T / 16); w += PG_THREADS) {
                const int eb = w / nout, j = w - eb * nout;
                const int fb = nout * nin + j, jbias = fb / nin;
                member_block<16>(wl + j * stride, wl[jbias * stride + (fb - jbias * nin)], src + 16 * eb,
                                 dst + j * ES + 16 * eb, ES, nin, hidden, true);
            }
            __syncthreads();
            if (hidden) wsrc += nout * nin + nout;  // stays on the last layer: its image is still staged below
        }
        if (tid < T) {  // the head: z -> logits_out, logp_out, dz in place
            const int64_t gi = col_idx[tid];
            const float c = col_coeff[tid];
            float lp = 0.0f;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float z[CP_NUM_DISCRETE], ex[CP_NUM_DISCRETE];
#pragma unroll
                for (int j = 0; j < CP_NUM_DISCRETE; ++j) z[j] = zt[(q * CP_NUM_DISCRETE + j) * ES + tid];
                if (gi >= 0 && a.logits) {
#pragma unroll
                    for (int j = 0; j < CP_NUM_DISCRETE; ++j) a.logits[gi * (2 * CP_NUM_DISCRETE) + q * CP_NUM_DISCRETE + j] = z[j];
                }
                float mx = z[0];
#pragma unroll
                for (int j = 1; j < CP_NUM_DISCRETE; ++j)
                    if (z[j] > mx) mx = z[j];
                float S = 0.0f;
#pragma unroll
                for (int j = 0; j < CP_NUM_DISCRETE; ++j) {
                    ex[j] = expf(z[j] - mx);
                    S = j ? S + ex[j] : ex[j];
                }
                const int act = col_act[tid][q];
                float za = z[0];
#pragma unroll
                for (int j = 1; j < CP_NUM_DISCRETE; ++j)
                    if (j == act) za = z[j];
                const float lpc = (za - mx) - logf(S);
                lp = q ? lp + lpc : lpc;
#pragma unroll
                for (int j = 0; j < CP_NUM_DISCRETE; ++j) {
                    const float pj = ex[j] / S;
                    const float dz = c * ((j == act ? 1.0f : 0.0f) - pj);
                    zt[(q * CP_NUM_DISCRETE + j) * ES + tid] = gi >= 0 ? dz : 0.0f;
                }
            }
            if (gi >= 0 && a.logp) a.logp[gi] = lp;
        }
        __syncthreads();
        int fbase = F;  // the layer's first parameter
        for (int l = L - 1; l >= 0; --l) {
            const int nin = pol.width[l], nout = pol.width[l + 1], stride = nin | 1;
            fbase -= nout * nin + nout;
            float* const x = lds + row0[l] * ES;
            const float* const d = lds + row0[l + 1] * ES;
            const int nI = (nin + 1 + 3) / 4, nJ = (nout + 3) / 4;
            for (int p = tid; p < nI * nJ; p += PG_THREADS) {
                const int jb = p / nI;
                pg_dw_patch(d, x, ES, T, nin, nout, jb, p - jb * nI, part + fbase);
            }
            if (l == 0) break;
            if (l < L - 1) pg_stage_weights(wmem + fbase, nin, nout, wl, tid);  // nobody reads wl in the patches
            __syncthreads();
            for (int w = tid; w < nin * (T / 16); w += PG_THREADS) {
                const int eb = w / nin, i = w - eb * nin;
                pg_back_block<16>(wl + i, stride, d + 16 * eb, x + i * ES + 16 * eb, ES, nout);
            }
            __syncthreads();
        }
        __syncthreads();  // the tiles are free for the next tile's columns
    }
}

// a member's partials in partial order
__global__ void __launch_bounds__(256) cp_policy_grad_reduce_kernel(int64_t PF, int slices, const float* partial, float* grad) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= PF) return;
    float g = partial[f];
    for (int s = 1; s < slices; ++s) g = g + partial[(size_t)s * (size_t)PF + (size_t)f];
    grad[f] = g;
}

inline hipError_t launch_policy_gradient(const cpc::Pol& pol, const cps::PolicyGrad& pg, const PolGrad& a, float* grad,
                                         hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)pg.rows * pg.es + (size_t)pg.wfloats);
    if (lds > 64 * 1024) {  // above the default dynamic-LDS limit
        const hipError_t e = hipFuncSetAttribute((const void*)cp_policy_grad_kernel,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cp_policy_grad_kernel, dim3((unsigned)pg.slices * (unsigned)pg.P), dim3(PG_THREADS), lds, st, pol,
                       pg, a);
    const int64_t PF = (int64_t)pg.P * pol.floats;
    hipLaunchKernelGGL(cp_policy_grad_reduce_kernel, dim3((unsigned)((PF + 255) / 256)), dim3(256), 0, st, PF, pg.slices,
                       a.partial, grad);
    return hipSuccess;
}

}  // namespace cp
