import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "openvino-sam-6d_amd")
for _p in (ROOT, PKG, os.path.join(PKG, "pem"), os.path.join(PKG, "ism")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLD = os.path.join(ROOT, "tests", "golden")


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def kernel_resources(marker, name_regex=r"([a-z_]+_kernel)", disassemble=False):
    """The compiler's figures for the kernels of the library's gfx950 code objects that contain `marker` (bytes, or a tuple of them:
    any), read from the code objects' metadata notes: {kernel: (VGPRs, scratch bytes, spilled VGPRs)}, the kernel named by the
    group of `name_regex` matched behind the mangled name's length.  With disassemble=True -> (that dict, the set of global / flat
    atomic mnemonics in those code objects).  Skips the calling test where the LLVM tools are not installed."""
    import re
    import subprocess
    import tempfile

    import pytest
    from sam6d_hip import _lib
    from tests.test_abi import _gfx950_code_objects
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(readelf) or (disassemble and not os.path.exists(objdump)):
        pytest.skip("llvm-readelf / llvm-objdump not available")
    markers = (marker,) if isinstance(marker, bytes) else tuple(marker)
    found, atomics = {}, set()
    for blob in _gfx950_code_objects(_lib.LIB_PATH):
        if not any(m in blob for m in markers):
            continue
        with tempfile.NamedTemporaryFile(suffix=".elf") as fh:
            fh.write(blob)
            fh.flush()
            notes = subprocess.run([readelf, "--notes", fh.name], capture_output=True, text=True, check=True).stdout
            if disassemble:
                asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", fh.name], capture_output=True, text=True, check=True).stdout
                atomics |= set(re.findall(r"\b(global_atomic_\w+|flat_atomic_\w+)", asm))
        for entry in re.split(r"\n\s*- \.agpr_count", notes):
            name = re.search(r"\.name:\s+_Z\d+" + name_regex, entry)
            if name:
                found[name.group(1)] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))
                                             for key in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count"))
    return (found, atomics) if disassemble else found
