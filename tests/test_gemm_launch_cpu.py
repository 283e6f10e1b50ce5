"""CPU: what launch_gemm / launch_gemm_mx refuse, and the launch shape they derive for what they accept.

The refusals between a GemmArgs and a kernel keep a wrong launch from becoming a wrong result or a fault, and most of
them cannot be reached from the public ops (a_rpg, patch_p, out_f32, resid32, fin_stats, the 2^24 / 2^31 limits; win_ws is
reachable since vdr_op_linear_window, whose own checks come first: tests/test_sam_ops_cpu.py, tests/test_sam_ops_gpu.py);
the launch shape (tile counts, column-group width, non-temporal stores, LDS bytes, block size, persistent form) cannot be
seen in any output.  tests/gemm_launch_cases.cpp calls the launchers with dummy buffers on a machine without a GPU -- an
accepted launch ends in hipErrorInvalidDevice (101) after every check has run, a refused one in hipErrorInvalidValue (1)
-- and prints the shape of each accepted case; its output is compared line for line with
tests/ledger/gemm_launch_cases.txt.

The ledger is a RECORD of the library at the commit its first line names, never of the code under test:
    python tests/test_gemm_launch_cpu.py --record tests/ledger/gemm_launch_cases.txt --lib path/to/libvdr.so --commit <sha>
(--no-builder: that library predates build_gemm_launch and prints the `shape` lines itself, from one printf ahead of the
device check of its launchers -- how the committed ledger was recorded, from the parent of the commit that introduced the
launch builder.)  With a GPU present the program refuses to run (its accepted cases would launch on dummy buffers) and
the test skips.
"""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "vit-deep-radiomics_amd", "csrc")
LIB = os.path.join(ROOT, "vit-deep-radiomics_amd", "vdr", "libvdr.so")
LEDGER = os.path.join(HERE, "ledger", "gemm_launch_cases.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HAS_DEVICE = 77


def _run_cases(lib, workdir, builder=True):
    """Builds the case program against `lib` and runs it: (exit status, stdout)."""
    exe = os.path.join(str(workdir), "gemm_launch_cases")
    libdir = os.path.dirname(os.path.abspath(lib))
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "gemm_launch_cases.cpp"), "-o", exe,
           "-L", libdir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    if not builder:
        cmd.append("-DVDR_CASES_NO_BUILDER")
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_refusals_and_launch_shapes_match_the_ledger(tmp_path):
    rc, out = _run_cases(LIB, tmp_path)
    if rc == HAS_DEVICE:
        pytest.skip("a GPU is present: the accepted cases would launch on dummy buffers")
    assert rc == 0
    with open(LEDGER) as f:
        header, want = f.readline(), f.read().splitlines()
    assert header.startswith("# recorded at commit ") and len(header.split()[-1]) == 40
    got = out.splitlines()
    assert sum(line.startswith("case ") for line in want) > 400
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            case = next(line for line in reversed(want[:i + 1]) if line.startswith("case "))
            pytest.fail(f"{case}: got `{g.strip()}`, ledger `{w.strip()}`")
    assert len(got) == len(want)


if __name__ == "__main__":
    import argparse
    import tempfile
    ap = argparse.ArgumentParser(description="record the GEMM launch ledger from a build of libvdr.so")
    ap.add_argument("--record", required=True, metavar="LEDGER.txt")
    ap.add_argument("--lib", default=LIB, help="the libvdr.so to record from (default: the package's own)")
    ap.add_argument("--commit", required=True, help="the commit that library was built at (the ledger's header)")
    ap.add_argument("--no-builder", action="store_true", help="the library prints the shape lines itself")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        rc, out = _run_cases(a.lib, d, builder=not a.no_builder)
    if rc != 0:
        sys.exit(f"the case program exited with {rc}" + (" (a GPU is present)" if rc == HAS_DEVICE else ""))
    with open(a.record, "w") as f:
        f.write(f"# recorded at commit {a.commit}\n" + out)
