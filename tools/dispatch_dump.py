"""Dump the conv dispatch table (CPU only, no GPU): one line per (case, mode, pass) of every grid tests/test_cpu_dispatch.py
walks, with the kernel name, the pass's workspace bytes, the executed FLOPs and (forward, backward-data) the prepared weight
bytes.  Two builds dispatch alike when their dumps are equal:

    python tools/dispatch_dump.py --envs OUT_DIR                       # this tree's library
    MUNIT_HIP_LIB=/path/to/other/libmunit_hip.so python tools/dispatch_dump.py --envs OTHER_DIR
    diff -r OUT_DIR OTHER_DIR

--envs writes one file per environment: the default one, MUNIT_WINO_S2_MIN_BLOCKS=1 and every MUNIT_DEBUG_* switch the
library's sources name, each set alone (the library reads a switch once per process, so each dump is a child process).
Without --envs the dump of the current environment goes to stdout."""
import ctypes
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases():
    """[(op case, (compute, in_dtype, out_dtype), passes)], each once, in a fixed order."""
    from tests import test_cpu_dispatch as T
    out = [(c, T.F32_MODE, (0, 1, 2)) for c in list(T.production_cases()) + T.op_cases()]
    out += [(c, mode, (0, 1, 2)) for c, mode in T.bf16s_production_cases()]
    out += [(c, mode, passes) for c, mode, passes in T.bf16_op_cases()]
    out += [(c, T.F32_MODE, (p,)) for p, c in T.seg_production_cases()]
    return sorted(set((tuple(c), tuple(m), tuple(p)) for c, m, p in out))


def dump(out):
    from munit_amd import _lib
    from tests.test_cpu_dispatch import PASSES, _desc
    lib = _lib.load()
    ws = (lib.munit_conv2d_fwd_workspace_bytes, lib.munit_conv2d_dgrad_workspace_bytes, lib.munit_conv2d_wgrad_workspace_bytes)
    for case, mode, passes in cases():
        for p in passes:
            d = ctypes.byref(_desc(case, p, mode))
            prep = lib.munit_conv2d_prepared_weight_bytes(d, p) if p < 2 else "-"
            out.write("%s %s %s | %s | ws %d | flops %r | prep %s\n" % (
                case, mode, PASSES[p], lib.munit_conv2d_kernel_name(d, p).decode(), ws[p](d), lib.munit_conv2d_executed_flops(d, p), prep))


def switches():
    src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "munit_amd", "csrc", "*.hip"))))
    return sorted(set(re.findall(r'"(MUNIT_DEBUG_[A-Z0-9_]+)"', src)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--envs":
        os.makedirs(sys.argv[2], exist_ok=True)
        envs = [("default", {}), ("MUNIT_WINO_S2_MIN_BLOCKS=1", {"MUNIT_WINO_S2_MIN_BLOCKS": "1"})] + [(s, {s: "1"}) for s in switches()]
        for name, extra in envs:
            with open(os.path.join(sys.argv[2], name + ".txt"), "w") as f:
                subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **extra), stdout=f, check=True)
            print("wrote", name)
    else:
        dump(sys.stdout)
