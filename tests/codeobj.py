"""The gfx950 code objects of the built libcgen_hip.so, for the tests that look at the shipped kernels without a GPU.

The library is unbundled once per process (llvm-objdump --offloading, into a temporary directory that is removed at exit) and the
kernel metadata is read once (llvm-readelf --notes).  Both functions skip the calling test when the llvm tools or the library are
missing; what a kernel may use is the calling test's business."""
import atexit
import functools
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

OBJDUMP, READELF = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
SO = os.path.join(ROOT, "causal-gen_amd", "libcgen_hip.so")


@functools.lru_cache(maxsize=None)
def _unbundle():
    d = tempfile.mkdtemp()
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    shutil.copy(SO, d)  # (llvm-objdump writes the bundles next to its input)
    subprocess.run([OBJDUMP, "--offloading", os.path.join(d, "libcgen_hip.so")], check=True, capture_output=True)
    return sorted(glob.glob(os.path.join(d, "*gfx950*")))


@functools.lru_cache(maxsize=None)
def _metadata():
    out = []
    for b in _unbundle():
        notes = subprocess.run([READELF, "--notes", b], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.wavefront_size", notes, re.S):
            name, body = m.group(1), m.group(2)
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
            sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", body)
            out.append((name, scratch, int(sp.group(1)) if sp else 0))
    return out


def bundle_paths():
    """Paths of the library's gfx950 code objects (ELF files a disassembler takes)."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(SO)):
        pytest.skip("llvm-objdump or the built library is missing")
    return list(_unbundle())


def kernels():
    """[(mangled kernel name, private_segment_fixed_size, vgpr_spill_count)] over every gfx950 kernel of the library; a kernel
    whose metadata has no spill count has 0."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF) and os.path.exists(SO)):
        pytest.skip("llvm tools or the built library are missing")
    return list(_metadata())
