"""What the CPU-side test files of the training ops share (test_{attn_bwd,linear_bwd,layer_train,mlp_train,conv_train}_cpu.py, and the
resource checks of test_abi_cpu.py, test_dedup_cpu.py, test_metrics_cpu.py): the compiler's resource report of a kernel file, the
never-dereferenced address and dtype codes of the argument-error tests, and the "exported, declared, one ABI number" check.  A plain
module: nothing here is a fixture."""
import ctypes as C
import os
import re
import subprocess

from brepgen_amd import _lib
from brepgen_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a 16-byte aligned address nobody dereferences: an argument check fails before anything touches the device
F32, F16, BF = _lib.BG_F32, _lib.BG_F16, _lib.BG_BF16
vp = C.c_void_p
RESOURCE_FLAG = "-Rpass-analysis=kernel-resource-usage"


def resource_usage(source, asm=False):
    """(names, scratch bytes per lane, VGPR spills, SGPR spills) of every kernel of csrc/`source`, one entry per kernel in the
    compiler's order, from hipcc's resource report with the build's flags; asm=True appends the device assembly text."""
    assert source in b.SOURCES, source
    out = ["-S", "--cuda-device-only", "-c", os.path.join(b.CSRC, source), "-o", "-"] if asm else ["-c", os.path.join(b.CSRC, source), "-o", os.devnull]
    r = subprocess.run([b._hipcc(), *b.FLAGS, *b.PER_FILE_FLAGS.get(source, []), RESOURCE_FLAG, *out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    cols = [[int(v) for v in re.findall(key + r": (\d+)", r.stderr)] for key in (r"ScratchSize \[bytes/lane\]", "VGPRs Spill", "SGPRs Spill")]
    assert all(len(c) == len(names) for c in cols), (len(names), [len(c) for c in cols])
    return (names, *cols, r.stdout) if asm else (names, *cols)


def explained(rc, code, word):
    """an entry refused its arguments with the negative `code` and a message that holds `word`"""
    msg = _lib.load().bg_last_error()
    assert rc == code and rc < 0, (rc, msg)
    assert word in msg, msg


def assert_exported(names, abi=7):
    """every name is exported by the library, bound in _lib and declared in the header (comments aside), and header, binding and
    library agree on the ABI number `abi`"""
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "brepgen_hip.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\b%s\s*\(" % n, code), n
    assert int(re.search(r"#define BG_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.bg_abi_version() == abi
