"""The posterior predictive kernels (csrc/dc_ppc.hip.h) keep everything in registers and LDS: no scratch, at
most 64 KB of LDS per workgroup, and the VGPR bound of DESIGN.md section 13 (no GPU needed: read from the code
object's metadata in the built library, as tests/test_loglik_resources.py does)."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bpl-next_amd", "bpl", "libbplhip.so")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library or LLVM tools not present")
    d = tmp_path_factory.mktemp("co")
    fat, co = str(d / "fat.bin"), str(d / "gfx950.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", LIB], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {
            "vgpr": int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
            "scratch": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
            "lds": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)),
        }
    shutil.rmtree(d, ignore_errors=True)
    return out


def _ppc(kernels):
    return {k: v for k, v in kernels.items() if "dcppc" in k and "dc_ppc" in k}


def test_ppc_kernels_exist_without_scratch(kernels):
    mine = _ppc(kernels)
    assert len(mine) == 2, sorted(mine)   # the plain and the venue form
    for name, k in mine.items():
        assert k["scratch"] == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)


def test_ppc_vgprs(kernels):
    # up to 96 VGPRs keep 5 waves per SIMD (one 256-lane workgroup per replication)
    for name, k in _ppc(kernels).items():
        assert k["vgpr"] <= 96, (name, k)
