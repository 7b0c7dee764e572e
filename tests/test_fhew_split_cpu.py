"""No-GPU checks of the split FHEW blind rotation's public surface: the header declares the option name, the query and the status
code, the library exports the query, and fhe_set_option validates the values of "BR_SPLIT"."""
import ctypes as C
import os
import re

from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "fhe_ring.h")).read()


def test_header_declares_option_query_and_status():
    text = header()
    assert '"BR_SPLIT"' in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fhe_blind_rotate_split\s*\(\s*const\s+fhe_bootstrap_key\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*int\s*\*\s*\w+\s*\)", code)
    # the status enum: the new code is the last one and takes the next free value; the earlier ones keep theirs
    enum = re.search(r"enum\s*\{(.*?)\}", code, flags=re.S).group(1)
    items = [(m.group(1), int(m.group(2))) for m in re.finditer(r"(FHE_\w+)\s*=\s*(\d+)", enum)]
    assert items[:8] == [("FHE_OK", 0), ("FHE_ERR_INVALID", 1), ("FHE_ERR_NOT_PRIME", 2), ("FHE_ERR_NO_ROOT", 3), ("FHE_ERR_MODULUS", 4),
                         ("FHE_ERR_HIP", 5), ("FHE_ERR_UNSUPPORTED", 6), ("FHE_ERR_NO_DEVICE", 7)]
    assert items[8:] == [("FHE_ERR_TIMEOUT", 8)]


def test_library_exports_the_query_and_names_the_status(fhe):
    lib = fhe.lib()
    assert hasattr(lib, "fhe_blind_rotate_split")
    g = C.c_int(-1)
    assert lib.fhe_blind_rotate_split(None, 1, C.byref(g)) == 1  # FHE_ERR_INVALID: no key
    from learn_fhe_amd import _lib
    assert _lib.STATUS[8] == "FHE_ERR_TIMEOUT"


def test_br_split_values(fhe):
    lib = fhe.lib()
    try:
        for v in (-1, 0, 2, 4, 8):
            assert lib.fhe_set_option(b"BR_SPLIT", v) == 0, v
        for v in (-2, 1, 3, 5, 6, 7, 9, 16, 64):
            assert lib.fhe_set_option(b"BR_SPLIT", v) == 1, v  # FHE_ERR_INVALID
        assert lib.fhe_set_option(b"BR_SPLITS", 2) == 1  # unknown names stay errors
    finally:
        assert lib.fhe_set_option(b"BR_SPLIT", -1) == 0
