"""The 7-byte fp64 values of the SELL delta layout (opts.sell_values; csrc/launch.hpp) on the host: a small C++ driver compiled against
launch.hpp checks that decode(encode(v)) gives back every bit of v for each value that qualifies (random normals over every exponent
range, +-0, denormals; unpacked from the three packed hi dwords as the kernel does), and that the qualification refuses exactly the sets
holding Inf / NaN or normals more than 7 binades apart."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_sell_values_encode_decode_and_qualification(tmp_path):
    exe = tmp_path / "codec"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "spmv-research_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sell_values_codec.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout
