"""No-GPU check of the pruning and levelling core that the FHEW and the TFHE netlist compilers share (csrc/netlist_levels.hpp)."""
import os
import subprocess


def test_levelling_core_as_a_host_program(tmp_path):
    """tests/netlist_levels_host_test.cpp: about 200 random DAGs (at most 40 inputs and 200 two-input gates; fan-out, dead gates, outputs
    that name inputs) through the core against a restatement, and as FHEW gates and TFHE nodes through both compilers: the same levels,
    level_start, max_width, n_live and live-node order; a stand-alone program under AddressSanitizer and UBSan, run as its own process"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "netlist_levels_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(here, "netlist_levels_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "netlist_levels_host_test ok" in out.stdout, out.stdout + out.stderr
