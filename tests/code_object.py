"""The gfx950 code object of the built library, for the test_*_resources.py files (no GPU needed): dumps the
fat binary, unbundles the gfx950 code object and parses each kernel's registers, scratch and LDS out of
the `llvm-readelf --notes` metadata."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bpl-next_amd", "bpl", "libbplhip.so")


def read_kernels(tmp_path_factory):
    """{mangled kernel name: {"vgpr", "scratch", "lds"}}; skips the calling test module when the library or
    the LLVM tools are not present.  The body of each module's `kernels` fixture."""
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
