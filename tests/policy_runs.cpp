// policy_runs — the member path's work split (cp_shapes.h: policy_path, policy_runs, policy_chunk and the LDS
// sizes) against a brute-force loop, for tests/test_policy_population_cpu.py (host C++ only):
//   c++ -std=c++17 -o policy_runs tests/policy_runs.cpp && ./policy_runs
// Every local env must lie in exactly one chunk, whose member is ((off + i) / G) % P; chunks hold at most 64
// envs of one run; the env blocks the kernel computes (4, or 16 wide) stay inside the tile's env stride.
#include <cstdio>
#include <vector>

#include "../cartpoleplusplus_amd/csrc/cp_shapes.h"

static int check(int64_t off, int G, int P, int B) {
    const cps::PolicyRuns r = cps::policy_runs(off, G, B);
    const int ES = cps::policy_env_stride(G, B);
    std::vector<int> seen(B, 0);
    for (int blk = 0; blk < r.runs * r.chunks_per_run; ++blk) {
        const cps::PolicyChunk c = cps::policy_chunk(off, G, P, B, r, blk);
        if (c.n <= 0) continue;
        if (c.n > 64 || c.lo < 0 || c.lo + c.n > B) return 1;
        for (int i = c.lo; i < c.lo + c.n; ++i) {
            if (((off + i) / G) % P != c.member) return 2;
            ++seen[i];
        }
        int e0 = 0, top = 0;  // the kernel's env blocks
        for (; e0 + 4 < c.n; e0 += 16) top = e0 + 16;
        for (; e0 < c.n; e0 += 4) top = e0 + 4;
        if (top > ES || ES % 4 != 0) return 3;
    }
    for (int i = 0; i < B; ++i)
        if (seen[i] != 1) return 4;
    return 0;
}

int main() {
    const int64_t offs[] = {0, 1, 31, 32, 63, 64, 95, 4096, (1ll << 32) + 7, (1ll << 40) + 64};
    const int Gs[] = {1, 2, 5, 32, 63, 64, 65, 96, 128, 130, 1000, 4096};
    const int Ps[] = {2, 3, 7, 130, 65536};
    const int Bs[] = {1, 3, 33, 64, 65, 130, 200, 1025};
    long cases = 0;
    for (int64_t off : offs)
        for (int G : Gs)
            for (int P : Ps)
                for (int B : Bs) {
                    const int rc = check(off, G, P, B);
                    if (rc) {
                        std::printf("FAIL %d off=%lld G=%d P=%d B=%d\n", rc, (long long)off, G, P, B);
                        return 1;
                    }
                    ++cases;
                }
    // the path: population <= 1 shared; whole waves of one member only when G and the offset are multiples of 64
    if (cps::policy_path(0, 0, 5) != cps::POLICY_SHARED || cps::policy_path(1, 7, 0) != cps::POLICY_SHARED ||
        cps::policy_path(3, 64, 128) != cps::POLICY_WAVE || cps::policy_path(3, 4096, 0) != cps::POLICY_WAVE ||
        cps::policy_path(3, 64, 32) != cps::POLICY_MEMBER || cps::policy_path(3, 96, 0) != cps::POLICY_MEMBER ||
        cps::policy_path(2, 1, 0) != cps::POLICY_MEMBER) {
        std::printf("FAIL path\n");
        return 1;
    }
    // LDS: the widest architecture with 64-env chunks fits a CU's 160 KiB; lrpg's "100,50" at G = 1 is small
    const int32_t wide[5] = {128, 128, 128, 128, 10}, lrpg[4] = {42, 100, 50, 10};
    const size_t big = cps::policy_member_lds_bytes(wide, 4, 64, 65536), small = cps::policy_member_lds_bytes(lrpg, 3, 1, 65536);
    if (big > 160 * 1024 || small != sizeof(float) * (2 * 100 * 4 + 5152)) {
        std::printf("FAIL lds %zu %zu\n", big, small);
        return 1;
    }
    std::printf("ok %ld cases, lds %zu %zu\n", cases, big, small);
    return 0;
}
