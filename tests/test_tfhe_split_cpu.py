"""No-GPU checks of the split TFHE blind rotation: the library's new exports and the harness names, the values the lab switch TFHE_SPLIT
takes, and csrc/tfhe_split.hpp (role map, rule, workspace sizes) as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ("fhe_tfhe_blind_rotate_split", "fhe_tggsw_key_status")


def test_new_symbols_and_harness_names(fhe):
    lib = fhe.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert callable(getattr(fhe.TggswKey, "split", None)) and callable(getattr(fhe.TggswKey, "check", None))


def test_null_arguments_are_invalid(fhe):
    import ctypes as C
    lib, g = fhe.lib(), C.c_int(-1)
    assert lib.fhe_tfhe_blind_rotate_split(None, None, 1, C.byref(g)) == 1 and g.value == -1
    assert lib.fhe_tggsw_key_status(None, None, 0) == 1


def test_option_values(fhe):
    try:
        for v in (-1, 0, 2, 6):
            fhe.set_option("TFHE_SPLIT", v)
        for v in (1, 3, 4, 8, -2, 5, 7, 12):
            with pytest.raises(fhe.FheError) as e:
                fhe.set_option("TFHE_SPLIT", v)
            assert e.value.code == 1, v
        fhe.set_option("tfhe_split", 2)  # names in either case, like every switch
    finally:
        fhe.set_option("TFHE_SPLIT", -1)


def test_host_header_as_a_program(tmp_path):
    exe = str(tmp_path / "tfhe_split_host_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "tfhe_split_host_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "tfhe_split_host_test ok" in out.stdout, out.stdout + out.stderr
