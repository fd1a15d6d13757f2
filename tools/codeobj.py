"""The gfx950 code object inside a compiled csrc object, for the tools that read it (spills.py,
code_diff.py): the .hip_fatbin bundle of OBJ is unbundled into a temporary file, and the AMDGPU
metadata notes (llvm-readelf --notes) give each kernel's register, LDS, scratch and spill counts."""
import contextlib
import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = "gfx950"


@contextlib.contextmanager
def code_object(obj):
    """Path of OBJ's unbundled gfx950 code object (None: a host-only object), valid inside the block."""
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "f.bin"), os.path.join(td, "k.co")
        r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(td, "o")],
                           capture_output=True)
        if r.returncode:   # no device code in this object (host-only source)
            yield None
            return
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
                        f"--input={fb}", f"--output={co}", "--unbundle"], check=True, capture_output=True)
        yield co


def metadata(co):
    """One dict per kernel of the code object CO, from its metadata notes."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    out = []
    # a kernel's entry starts at "  - ." and holds its own keys at that depth (its arguments' deeper)
    for blk in re.split(r"^  - (?=\.)", notes.split("amdhsa.kernels:", 1)[-1], flags=re.M)[1:]:
        blk = re.split(r"^\S", "    " + blk, 1, flags=re.M)[0]   # up to the next top-level key
        def g(k):
            m = re.search(r"^    \." + k + r":\s+(\S+)", blk, flags=re.M)
            return m.group(1) if m else "0"
        if not g("symbol").endswith(".kd"):
            continue
        out.append({"name": g("name"), "vgpr": int(g("vgpr_count")), "agpr": int(g("agpr_count")),
                    "sgpr": int(g("sgpr_count")), "vspill": int(g("vgpr_spill_count")),
                    "sspill": int(g("sgpr_spill_count")), "scratch": int(g("private_segment_fixed_size")),
                    "lds": int(g("group_segment_fixed_size"))})
    return out


def kernels(obj):
    with code_object(obj) as co:
        return metadata(co) if co else []
