"""Host check of the lazy forward butterfly of the wave-local transforms (learn-fhe_amd/csrc/arith.hpp: ArithDS<B>::ct_lazy, mul_raw,
fold1 and the compile-time schedule DsLazy<B>) against unsigned __int128, at 60, 55 and 54 bits: tests/ds_lazy_host_test.cpp feeds
every layer of the schedule its largest admitted input and checks that no intermediate reaches 2^64 and that the outputs are
x + w y and x - w y mod q.  The static_asserts of arith.hpp are the proof; this checks that the code follows it.  arith.hpp is a HIP
header, so the program is built with the HIP compiler's host pass alone; nothing here touches a GPU."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lazy_butterfly_bounds_against_int128(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "ds_lazy_host_test")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "ds_lazy_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "passed" in out.stdout
