"""Build the gfx950 HIP library (vpin_amd/lib/libvpin_hip.so) in-tree with hipcc.

hipcc cross-compiles for gfx950 without a GPU present, so this also runs in the CPU-only
build container.  The built .so is git-ignored but travels with the tree to the GPU box.
"""
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libvpin_hip.so")
ARCH = "gfx950"


def hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built (no CPU fallback exists)")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))


def deps():
    return sources() + [os.path.join(CSRC, "cli", "vpin_prove.cpp")] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "host", "*.h")) + [
        os.path.join(os.path.dirname(HERE), "include", "vpin_hip.h")]


def up_to_date():
    if not os.path.exists(LIB_PATH):
        return False
    t = os.path.getmtime(LIB_PATH)
    return all(os.path.getmtime(s) <= t for s in deps())


def build(force=False, verbose=False):
    if not force and up_to_date():
        build_devtest(verbose=verbose)
        build_hosttest(verbose=verbose)
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    objs = []
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    procs = []
    for src in sources():
        obj = os.path.join(obj_dir, os.path.basename(src) + ".o")
        objs.append(obj)
        newest_dep = max(os.path.getmtime(d) for d in deps() if not d.endswith((".hip", ".cpp")) or d == src)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= newest_dep:
            continue
        cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-c", src, "-o", obj,
               "-I", os.path.join(os.path.dirname(HERE), "include")] + os.environ.get("VPIN_HIPCC_FLAGS", "").split()
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-fopenmp", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    build_cli(verbose)
    build_devtest(force=True, verbose=verbose)
    build_hosttest(force=True, verbose=verbose)
    return LIB_PATH


def build_cli(verbose=False):
    """vpin_amd/bin/vpin_prove: the reference binary's CLI contract over the C ABI."""
    src = os.path.join(CSRC, "cli", "vpin_prove.cpp")
    out_dir = os.path.join(HERE, "bin")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "vpin_prove")
    cmd = [hipcc(), "-O2", "-std=c++17", "-pthread", src, "-o", out, "-L", LIB_DIR, "-lvpin_hip", "-Wl,-rpath,$ORIGIN/../lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


DEVTEST_SRC = os.path.join(os.path.dirname(HERE), "tests", "devarith", "devarith.hip")
DEVTEST_LIB = os.path.join(LIB_DIR, "libvpin_devtest.so")


def devtest_up_to_date():
    if not os.path.exists(DEVTEST_LIB):
        return False
    t = os.path.getmtime(DEVTEST_LIB)
    return all(os.path.getmtime(s) <= t for s in [DEVTEST_SRC] + glob.glob(os.path.join(CSRC, "*.h")))


def build_devtest(force=False, verbose=False, out=None, csrc=None):
    """vpin_amd/lib/libvpin_devtest.so: tests/devarith/devarith.hip, one kernel and one launcher per device function of the
    arithmetic headers, compiled with the product's flags.  Test-only and a library of its own: nothing of it is in
    libvpin_hip.so or include/vpin_hip.h; it refers to libvpin_hip.so for the host function make_fq_const alone.
    out / csrc: another output file and another copy of the headers (a mutated copy, to see that the tests notice)."""
    if out is None and csrc is None and not force and devtest_up_to_date():
        return DEVTEST_LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libvpin_hip.so comes first: the harness links to it for make_fq_const")
    os.makedirs(LIB_DIR, exist_ok=True)
    out = out or DEVTEST_LIB
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", DEVTEST_SRC, "-o", out,
           "-I", csrc or CSRC, "-L", LIB_DIR, "-lvpin_hip", "-Wl,-rpath,$ORIGIN"]
    cmd += os.environ.get("VPIN_HIPCC_FLAGS", "").split()
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


HOSTTEST_DIR = os.path.join(os.path.dirname(HERE), "tests", "hostarith")
HOSTTEST_SRC = os.path.join(HOSTTEST_DIR, "hostarith.cpp")
HOSTTEST_MAIN = os.path.join(HOSTTEST_DIR, "hostarith_main.cpp")
HOSTTEST_LIB = os.path.join(LIB_DIR, "libvpin_hosttest.so")
HOSTTEST_FLAGS = ["--offload-host-only", "-O3", "-std=c++17", "-fPIC", "-fopenmp"]  # the host pass with the product's flags


def hosttest_deps():
    return [HOSTTEST_SRC] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "host", "*.h"))


def build_hosttest(force=False, verbose=False, out=None, csrc=None):
    """vpin_amd/lib/libvpin_hosttest.so: tests/hostarith/hostarith.cpp, one extern "C" function per function of host/field.h,
    host/curve.h and the UniPoly / eq helpers of host/prover_common.h, compiled by hipcc's host pass with the product's flags.
    Test-only and a library of its own: nothing of it is in libvpin_hip.so or include/vpin_hip.h, and it refers to neither.
    out / csrc: another output file and another copy of csrc's headers (a mutated copy, to see that the tests notice)."""
    if out is None and csrc is None and not force and os.path.exists(HOSTTEST_LIB) and all(
            os.path.getmtime(s) <= os.path.getmtime(HOSTTEST_LIB) for s in hosttest_deps()):
        return HOSTTEST_LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    out = out or HOSTTEST_LIB
    cmd = [hipcc()] + HOSTTEST_FLAGS + ["-shared", HOSTTEST_SRC, "-o", out, "-I", csrc or CSRC]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_hosttest_program(out, sanitize="address,undefined", verbose=False):
    """the same harness as a program of its own (tests/hostarith/hostarith_main.cpp reads a vector file and prints the results),
    host code only, with the sanitizers compiled in: sanitized code is run as a child process, never loaded into python."""
    cmd = [hipcc()] + HOSTTEST_FLAGS + ["-g", "-fno-omit-frame-pointer", "-Xarch_host", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
                                        HOSTTEST_SRC, HOSTTEST_MAIN, "-o", out, "-I", CSRC]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
