// shape_table — prints what cp_shapes.h resolves and accepts, for tests/test_shapes_cpu.py (host C++ only):
//   c++ -std=c++17 -o shape_table tests/shape_table.cpp && ./shape_table
// First the resolver's table, one line per case: its number, the inputs, "->", the step and reset shapes.
// Then cp_set_kernel_shape's checks: per handle class and step request -2..6, one letter per reset request
// -2..6 (A accepted, R refused).
#include <cstdio>

#include "../cartpoleplusplus_amd/csrc/cp_shapes.h"

static const char* name(int shape) {
    static const char* const names[] = {"auto", "throughput", "latency", "wide", "wide8", "wide64", "list"};
    return shape >= CP_SHAPE_AUTO && shape <= CP_SHAPE_LIST ? names[shape + 1] : "?";
}

int main() {
    const int SAME = CP_AUTORESET_SAME_STEP, NEXT = CP_AUTORESET_NEXT_STEP, A = CP_SHAPE_AUTO;
    const unsigned PM = CP_MODEL_PERSISTENT, SLP = CP_MODEL_SLEEPING;
    // num_envs, f64, model_flags, autoreset, done_on_bounds, lqr_done, step_knob, reset_knob, step_req, reset_req
    const cps::ShapeInputs rows[] = {
        {1, false, 0, CP_AUTORESET_OFF, false, false, -1, -1, A, A},
        {1024, false, 0, SAME, false, false, -1, -1, A, A},
        {1025, false, 0, SAME, false, false, -1, -1, A, A},
        {4096, false, 0, SAME, false, false, -1, -1, A, A},
        {4097, false, 0, SAME, false, false, -1, -1, A, A},
        {8192, false, 0, SAME, false, false, -1, -1, A, A},
        {8193, false, 0, SAME, false, false, -1, -1, A, A},
        {32768, false, 0, SAME, false, false, -1, -1, A, A},
        {32769, false, 0, SAME, false, false, -1, -1, A, A},
        {65536, false, 0, SAME, true, false, -1, -1, A, A},
        {64, false, 0, SAME, true, false, -1, -1, A, A},
        {65536, false, 0, SAME, false, true, -1, -1, A, A},
        {65536, false, 0, SAME, false, false, -1, -1, A, A},  // LQR gains on, both done thresholds <= 0
        {4096, false, 0, NEXT, false, false, -1, -1, A, A},
        {65536, false, 0, NEXT, false, false, -1, -1, A, A},
        {65536, false, 0, NEXT, true, false, -1, -1, A, A},
        {64, true, 0, SAME, false, false, -1, -1, A, A},
        {65536, true, 0, SAME, false, false, -1, -1, A, A},
        {64, false, SLP, SAME, false, false, -1, -1, A, A},
        {65536, false, PM, SAME, true, false, -1, -1, A, A},
        {64, false, 0, SAME, false, false, 0, -1, A, A},
        {65536, false, 0, SAME, false, false, 1, -1, A, A},
        {64, false, 0, SAME, false, false, 1, -1, A, A},
        {64, false, 0, SAME, false, false, -1, 0, A, A},
        {65536, false, 0, SAME, true, false, -1, 0, A, A},
        {65536, false, 0, SAME, false, false, -1, 1, A, A},
        {65536, false, 0, NEXT, false, false, -1, 1, A, A},
        {64, true, 0, SAME, false, false, 0, -1, A, A},
        {8192, false, 0, SAME, false, false, -1, -1, CP_SHAPE_THROUGHPUT, CP_SHAPE_LIST},
        {64, false, 0, SAME, false, false, 1, -1, CP_SHAPE_THROUGHPUT, A},
        {65536, false, 0, SAME, false, false, -1, -1, A, CP_SHAPE_WIDE64},
    };
    int n = 0;
    for (const cps::ShapeInputs& r : rows) {
        const cps::Shapes s = cps::resolve_shapes(r);
        std::printf("%d envs=%d f64=%d flags=%u autoreset=%d bounds=%d lqr_done=%d knobs=%d,%d req=%s,%s -> %s %s\n", ++n,
                    r.num_envs, (int)r.f64, r.model_flags, r.autoreset, (int)r.done_on_bounds, (int)r.lqr_done,
                    r.step_knob, r.reset_knob, name(r.step_req), name(r.reset_req), name(s.step), name(s.reset));
    }
    const struct {
        const char* what;
        bool f64;
        unsigned flags;
    } classes[] = {{"f32", false, 0}, {"f64", true, 0}, {"persistent", false, PM}, {"sleeping", false, SLP}};
    for (const auto& c : classes) {
        for (int step = -2; step <= 6; ++step) {
            std::printf("check %s step=%d ", c.what, step);
            for (int reset = -2; reset <= 6; ++reset)
                std::putchar(cps::check_requests(c.f64, c.flags, step, reset) ? 'R' : 'A');
            std::putchar('\n');
        }
    }
    // the knobs' values, and the lanes per env of every shape
    std::printf("knob %d %d %d %d %d\n", cps::knob_value(nullptr), cps::knob_value(""), cps::knob_value("0"),
                cps::knob_value("1"), cps::knob_value("2"));
    std::printf("lanes");
    for (int shape = CP_SHAPE_THROUGHPUT; shape <= CP_SHAPE_LIST; ++shape) std::printf(" %d", cps::lanes_per_env(shape));
    std::putchar('\n');
    return 0;
}
