"""The library's gfx950 assembly for the ISA guards (tests/test_isa_*.py) and tools/isa_diff.py: engine.hip is compiled
once per process, with the flags every guard has always used, and parsed into per-kernel metadata and instruction lists."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only"]
META_KEYS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "sgpr_spill_count", "sgpr_count",
             "group_segment_fixed_size")
_ISA = []  # [text] or [exception]: the one compile of this process, failed or not


def engine_isa():
    """Assembly text of eoc_tfhe_amd/csrc/engine.hip; skips the calling test where there is no hipcc.  A failed compile is
    remembered too: every later caller gets the same error at once."""
    if not os.path.exists(HIPCC):
        import pytest
        pytest.skip("no hipcc")
    if not _ISA:
        try:
            with tempfile.TemporaryDirectory(prefix="eoc_isa_") as tmp:
                out = os.path.join(tmp, "engine.s")
                subprocess.run([HIPCC, *ISA_FLAGS, "-o", out, os.path.join(ROOT, "eoc_tfhe_amd", "csrc", "engine.hip")],
                               check=True, cwd=tmp)
                with open(out) as f:
                    _ISA.append(f.read())
        except (subprocess.CalledProcessError, OSError) as e:
            _ISA.append(e)
    if isinstance(_ISA[0], Exception):
        raise _ISA[0]
    return _ISA[0]


def multi_isa():
    """Assembly text of eoc_tfhe_amd/csrc/multi.hip, the library's second code object (one small kernel: not remembered)"""
    if not os.path.exists(HIPCC):
        import pytest
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory(prefix="eoc_isa_") as tmp:
        out = os.path.join(tmp, "multi.s")
        subprocess.run([HIPCC, *ISA_FLAGS, "-o", out, os.path.join(ROOT, "eoc_tfhe_amd", "csrc", "multi.hip")], check=True, cwd=tmp)
        with open(out) as f:
            return f.read()


def demangled(names):
    """the mangled names `names` demangled by c++filt (binutils), in order"""
    out = subprocess.run([shutil.which("c++filt") or "c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return out.stdout.splitlines()


def kernel_meta(text):
    """mangled kernel name -> the code object's metadata: registers, spills, scratch and LDS bytes"""
    meta = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in META_KEYS}
        meta[name]["agpr_count"] = int(re.match(r"\s*(\d+)", blk).group(1))
    return meta


# a branch target: .LBB<function's number in the code object>_<block index>
_BLOCK_LABEL = re.compile(r"(?<![\w.$])\.LBB\d+_(\d+)\b")


def kernel_bodies(text):
    """mangled kernel name -> its instructions, stripped, from the kernel's label to its .Lfunc_end: the whole function,
    not only what precedes the first s_endpgm (the blind-rotation kernels leave early once).  Comments, directives and
    labels are dropped.  Branch targets lose the function's number and keep the block index (.LBB17_4 -> .LBB_4): the
    number says where in the code object the kernel was emitted, not what it does.  Nothing else is touched."""
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.M | re.S):
        lines = (ln.strip() for ln in m.group(2).splitlines())
        bodies[m.group(1)] = [_BLOCK_LABEL.sub(r".LBB_\1", ln) for ln in lines if ln and not ln.startswith((";", "."))]
    return bodies
