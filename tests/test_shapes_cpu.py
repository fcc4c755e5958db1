"""The kernel-shape resolver (cartpoleplusplus_amd/csrc/cp_shapes.h) pinned on the CPU: tests/shape_table.cpp, a
stand-alone host program, prints what it resolves for 31 cases and which cp_set_kernel_shape requests it accepts;
both are compared with tables written out here.  The resolver's rows were confirmed against the code they
replaced (choose_reset_shape in cp_kernels.hip before cp_shapes.h existed).  About a second: one host compile."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")

PM, SLP = 0x4, 0x8  # CP_MODEL_PERSISTENT, CP_MODEL_SLEEPING
OFF, SAME, NEXT = 0, 1, 2  # CP_AUTORESET_*

# (envs, the inputs that differ from the defaults D, step, reset); the knobs sk / rk: -1 unset
D = dict(f64=0, flags=0, autoreset=SAME, bounds=0, lqr_done=0, sk=-1, rk=-1, sreq="auto", rreq="auto")
ROWS = [
    (1, dict(autoreset=OFF), "wide", "wide64"),
    (1024, {}, "wide", "wide64"),
    (1025, {}, "wide", "wide"),
    (4096, {}, "wide", "wide"),
    (4097, {}, "wide8", "wide8"),
    (8192, {}, "wide8", "wide8"),
    (8193, {}, "latency", "latency"),
    (32768, {}, "latency", "latency"),
    (32769, {}, "throughput", "throughput"),
    (65536, dict(bounds=1), "throughput", "list"),
    (64, dict(bounds=1), "wide", "list"),
    (65536, dict(lqr_done=1), "throughput", "list"),
    (65536, {}, "throughput", "throughput"),  # LQR gains on, both done thresholds <= 0: lqr_done stays 0
    (4096, dict(autoreset=NEXT), "wide", "latency"),
    (65536, dict(autoreset=NEXT), "throughput", "throughput"),
    (65536, dict(autoreset=NEXT, bounds=1), "throughput", "list"),
    (64, dict(f64=1), "latency", "latency"),
    (65536, dict(f64=1), "latency", "latency"),
    (64, dict(flags=SLP), "latency", "latency"),
    (65536, dict(flags=PM, bounds=1), "latency", "latency"),
    (64, dict(sk=0), "throughput", "wide64"),
    (65536, dict(sk=1), "latency", "throughput"),
    (64, dict(sk=1), "wide", "wide64"),  # a knob of 1: the latency register budget, the layout still automatic
    (64, dict(rk=0), "wide", "throughput"),
    (65536, dict(rk=0, bounds=1), "throughput", "throughput"),
    (65536, dict(rk=1), "throughput", "latency"),
    (65536, dict(rk=1, autoreset=NEXT), "throughput", "latency"),
    (64, dict(sk=0, f64=1), "latency", "latency"),
    (8192, dict(sreq="throughput", rreq="list"), "throughput", "list"),
    (64, dict(sk=1, sreq="throughput"), "throughput", "wide64"),
    (65536, dict(rreq="wide64"), "throughput", "wide64"),
]


def _expected_rows():
    out = []
    for n, (envs, over, step, reset) in enumerate(ROWS, 1):
        r = dict(D, **over)
        out.append(f"{n} envs={envs} f64={r['f64']} flags={r['flags']} autoreset={r['autoreset']} bounds={r['bounds']} "
                   f"lqr_done={r['lqr_done']} knobs={r['sk']},{r['rk']} req={r['sreq']},{r['rreq']} -> {step} {reset}")
    return out


def _expected_checks():
    """cp_set_kernel_shape: values outside -1..5 are refused; so are wide64 (4) and list (5) as step requests;
    fp64, persistent and sleeping handles take auto (-1) and latency (1) only, on either kernel."""
    out = []
    for what in ("f32", "f64", "persistent", "sleeping"):
        for step in range(-2, 7):
            row = ""
            for reset in range(-2, 7):
                ok = -1 <= step <= 5 and -1 <= reset <= 5 and step not in (4, 5)
                if what != "f32":
                    ok = ok and step in (-1, 1) and reset in (-1, 1)
                row += "A" if ok else "R"
            out.append(f"check {what} step={step} {row}")
    return out


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_shape_table(tmp_path):
    exe = str(tmp_path / "shape_table")
    subprocess.run([CXX, "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "shape_table.cpp")],
                   check=True, capture_output=True, text=True, timeout=120)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines()
    assert len(ROWS) == 31
    want = _expected_rows() + _expected_checks() + ["knob -1 -1 0 1 -1", "lanes 2 2 16 8 64 2"]
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
