"""The operand check the norm and dropout launchers share (csrc/kernels/rowwise.h) is plain host
code: rowwise_check_main.hip calls it directly -- no rows with null pointers, a single row's
stride, the 8,192-feature limit, the chunk-width rule, misaligned bases, overlapping operands --
built with the host side under AddressSanitizer and UBSan.  A host-only check: it needs hipcc but
no device, and stays off machines that have one."""
import os
import subprocess

import pytest

import nnmpi_amd  # noqa: F401
from nnmpi_amd import _build
from conftest import gpu_available

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not os.path.exists(_build.HIPCC), reason="hipcc not found")
@pytest.mark.skipif(gpu_available(), reason="host-side sanitizer run: not on a GPU machine")
def test_row_check_contract_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "rowwise_check")
    cmd = [_build.HIPCC, f"--offload-arch={_build.ARCH}", "--cuda-host-only", "-std=c++17", "-O1",
           "-g", "-I", _build.CSRC, "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(HERE, "rowwise_check_main.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "rowwise check: ok" in r.stdout
