"""Host check of the lazy inverse of the wave-local transforms (learn-fhe_amd/csrc/arith.hpp: ArithDS<B>::gs_lazy, gs_diag_lazy,
gs_last_scaled_lazy / gs_last_plain_lazy and the compile-time schedule DsGsLazy<B>) against unsigned __int128, at 60, 55 and 54
bits: tests/ds_gs_lazy_host_test.cpp drives every step of every ring size's schedule with operands and twiddle words at the maxima
the schedule assumes and checks that no intermediate reaches 2^64, no difference goes negative, the outputs are x + y and
(x - y) w mod q below the schedule's bounds, and the last layer comes out canonical.  The static_asserts of arith.hpp are the proof;
this checks that the code follows it.  arith.hpp is a HIP header, so the program is built with the HIP compiler's host pass alone;
nothing here touches a GPU."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lazy_inverse_bounds_against_int128(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "ds_gs_lazy_host_test")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "ds_gs_lazy_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "passed" in out.stdout
