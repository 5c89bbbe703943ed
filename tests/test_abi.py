"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/vc2hip.h declares; host-only helpers agree with the oracle.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vc2-reference_amd", "libvc2hip.so")


def _declared():
    hdr = open(os.path.join(ROOT, "include", "vc2hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(vc2hip_[a-z0-9_]+)\s*\(", hdr)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return C.CDLL(LIB)


def test_header_symbols_exported(lib):
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vc2hip.h but not exported"


def test_nothing_but_the_header_is_exported(lib):
    """the library is built with hidden visibility; `nm -D` must list the functions of
    include/vc2hip.h as its only defined text symbols (round 4 exported 73 internal C++ launchers beside them)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    text = sorted(l.split()[-1] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] in "TtWw")
    assert text == sorted(_declared()), sorted(set(text) ^ set(_declared()))


def test_release_library_reads_no_environment():
    """the switches between two correct paths are vc2hip_create_with_flags bits; getenv appears in the
    library's sources only inside -DVC2HIP_ABLATE / -DVC2HIP_STAMPS blocks (tools builds)."""
    import glob
    import re
    for f in sorted(glob.glob(os.path.join(ROOT, "vc2-reference_amd", "csrc", "*.h*"))):
        depth = []   # stack of (is_tools_block)
        for n, line in enumerate(open(f), 1):
            t = line.strip()
            if t.startswith("#if"):
                depth.append(bool(re.search(r"VC2HIP_ABLATE|VC2HIP_STAMPS", t)) and not t.startswith("#ifndef"))
            elif t.startswith("#else") and depth:
                depth[-1] = False if depth[-1] else depth[-1]
            elif t.startswith("#endif") and depth:
                depth.pop()
            elif "getenv(" in t and not t.startswith("//"):
                assert any(depth), f"{os.path.basename(f)}:{n}: getenv outside a tools-only block: {t[:100]}"


def test_the_callers_stream_constructor_with_flags_is_declared_and_bound():
    import vc2hip_py
    assert "vc2hip_create_on_stream_with_flags" in _declared()
    assert "vc2hip_create_on_stream_with_flags" in vc2hip_py.EXPORTS


def test_binding_covers_header():
    import vc2hip_py
    assert sorted(vc2hip_py.EXPORTS) == [n for n in _declared() if n in vc2hip_py.EXPORTS]
    missing = set(_declared()) - set(vc2hip_py.EXPORTS)
    assert not missing, missing


def test_host_helpers_match_oracle(lib, oracle):
    for size in (1, 15, 16, 17, 1080, 2160):
        for d in range(1, 6):
            assert lib.vc2hip_padded_size(size, d) == oracle.padded_size(size, d)
    for k in range(7):
        for d in range(1, 6):
            out = np.zeros(3 * d + 1, np.int32)
            lib.vc2hip_quant_matrix.argtypes = [C.c_int, C.c_int, np.ctypeslib.ndpointer(np.int32)]
            assert lib.vc2hip_quant_matrix(k, d, out) == 0
            assert out.tolist() == oracle.quant_matrix(k, d).tolist()
    for (ys, xs, total, scalar) in [(8, 4, 6000, 1), (135, 120, 8294400, 2), (3, 5, 1000, 3)]:
        out = np.zeros((ys, xs), np.int32)
        lib.vc2hip_slice_bytes.argtypes = [C.c_int] * 4 + [np.ctypeslib.ndpointer(np.int32)]
        lib.vc2hip_slice_bytes(ys, xs, total, scalar, out)
        assert np.array_equal(out, oracle.slice_bytes(ys, xs, total, scalar))
    assert lib.vc2hip_slice_size_is_valid(4, 2160, 2160, 1) == 135
    assert lib.vc2hip_slice_size_is_valid(4, 3840, 1920, 2) == 120
    assert lib.vc2hip_slice_size_is_valid(3, 80, 40, 1) == 0


def test_error_strings_are_the_reference_ones(lib):
    lib.vc2hip_error_string.restype = C.c_char_p
    assert lib.vc2hip_error_string(-2) == b"quantization index exceeds maximum implemented value."
    assert lib.vc2hip_error_string(-3) == b"Slice scalar is too small, consider using a larger slice scalar."
    assert lib.vc2hip_error_string(-4) == b"SliceIO, HQ CBR mode: Too many bytes for the slice"


def test_create_without_gpu_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert lib.vc2hip_create(0, C.byref(h)) != 0   # no silent CPU fallback
