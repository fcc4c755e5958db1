// policy_grad_plan — cp_policy_gradient's work split (cp_shapes.h: policy_grad_plan, policy_grad_member_tiles,
// policy_grad_tile and the LDS sizes) against a brute-force loop, for tests/test_policy_grad_cpu.py (host C++ only):
//   c++ -std=c++17 -o policy_grad_plan tests/policy_grad_plan.cpp && ./policy_grad_plan
// Every sample (k, i) of the window must lie in exactly one tile of exactly one slice, of the member
// ((off + i) / G) % P; a tile holds at most `tile` samples of one run; the LDS of every legal architecture fits a CU.
#include <cstdio>
#include <vector>

#include "../cartpoleplusplus_amd/csrc/cp_shapes.h"

static int check(const int32_t* width, int layers, int64_t off, int G, int P, int B, int K) {
    const cps::PolicyGrad p = cps::policy_grad_plan(width, layers, P, G, off, K, B);
    if (p.tile != 16 && p.tile != 32 && p.tile != 64) return 1;
    if (p.es < p.tile || p.es % 4 != 0 || p.slices < 1) return 2;
    if ((int64_t)p.slices * p.P > 2048 && p.slices != 1) return 3;
    std::vector<int> seen((size_t)K * B, 0);
    for (int m = 0; m < p.P; ++m) {
        const int64_t tiles = cps::policy_grad_member_tiles(p, m);
        const int64_t per = (tiles + p.slices - 1) / p.slices;
        int64_t served = 0;
        for (int s = 0; s < p.slices; ++s) {
            const int64_t lo = (int64_t)s * per, hi = lo + per < tiles ? lo + per : tiles;
            for (int64_t t = lo; t < hi; ++t, ++served) {
                const cps::PolicyGradTile x = cps::policy_grad_tile(p, m, t);
                if (x.n < 1 || x.n > p.tile || x.len < 1 || x.lo < 0 || x.lo + x.len > B) return 4;
                if (x.s0 < 0 || (int64_t)x.s0 + x.n > (int64_t)x.len * K) return 5;
                for (int c = 0; c < x.n; ++c) {
                    const int sidx = x.s0 + c, k = sidx / x.len, i = x.lo + sidx % x.len;
                    const int64_t want = P > 1 ? ((off + i) / G) % P : 0;
                    if (want != m) return 6;
                    ++seen[(size_t)k * B + i];
                }
            }
        }
        if (served != tiles) return 7;
    }
    for (int v : seen)
        if (v != 1) return 8;
    return 0;
}

int main() {
    const int32_t lrpg[4] = {42, 100, 50, 10}, tiny[4] = {14, 7, 5, 10}, one[2] = {14, 10};
    const int32_t wide[5] = {126, 128, 128, 128, 10}, wide3[5] = {42, 128, 128, 128, 10};
    const int64_t offs[] = {0, 1, 37, 64, 4096, (1ll << 32) + 5};
    const int Gs[] = {1, 2, 5, 64, 65, 130, 4096, 1 << 30};
    const int Ps[] = {0, 1, 2, 3, 7, 130, 65536};
    const int Bs[] = {1, 3, 64, 65, 130, 200};
    const int Ks[] = {1, 2, 7, 40};
    long cases = 0;
    for (int64_t off : offs)
        for (int G : Gs)
            for (int P : Ps)
                for (int B : Bs)
                    for (int K : Ks) {
                        const int rc = check(cases % 2 ? lrpg : tiny, 3, off, G, P, B, K);
                        if (rc) {
                            std::printf("FAIL %d off=%lld G=%d P=%d B=%d K=%d\n", rc, (long long)off, G, P, B, K);
                            return 1;
                        }
                        ++cases;
                    }
    if (check(one, 1, 37, 5, 3, 130, 7) || check(wide, 4, 0, 1, 2, 65, 3)) {
        std::printf("FAIL extra\n");
        return 1;
    }
    // LDS: lrpg's net leaves room for two blocks per CU at 64 samples; the widest legal policy fits one CU at 32
    const cps::PolicyGrad a = cps::policy_grad_plan(lrpg, 3, 1, 1, 0, 200, 65536);
    const cps::PolicyGrad b = cps::policy_grad_plan(wide, 4, 1, 1, 0, 200, 65536);
    const cps::PolicyGrad c = cps::policy_grad_plan(wide3, 4, 1, 1, 0, 200, 65536);
    const size_t la = cps::policy_grad_lds_bytes(lrpg, 3, a.tile, nullptr, nullptr);
    const size_t lb = cps::policy_grad_lds_bytes(wide, 4, b.tile, nullptr, nullptr);
    const size_t lc = cps::policy_grad_lds_bytes(wide3, 4, c.tile, nullptr, nullptr);
    if (a.tile != 64 || 2 * la > cps::kPolicyGradLdsMax || b.tile != 32 || lb > cps::kPolicyGradLdsMax ||
        lc > cps::kPolicyGradLdsMax || a.slices != 2048) {
        std::printf("FAIL lds %d %zu %d %zu %d %zu slices %d\n", a.tile, la, b.tile, lb, c.tile, lc, a.slices);
        return 1;
    }
    // the test suite's several-partials shape: K = 40, B = 130, P = 2, G = 1
    const cps::PolicyGrad d = cps::policy_grad_plan(tiny, 3, 2, 1, 0, 40, 130);
    if (d.slices < 2 || cps::policy_grad_scratch_bytes(d, 198) != (((int64_t)d.slices * 2 * 198 * 4 + 15) & ~15ll)) {
        std::printf("FAIL partials %d\n", d.slices);
        return 1;
    }
    std::printf("ok %ld cases, lds %zu %zu %zu, tiles %d %d %d\n", cases, la, lb, lc, a.tile, b.tile, c.tile);
    return 0;
}
