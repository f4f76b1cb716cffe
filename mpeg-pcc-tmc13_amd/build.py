"""Build the gfx950 shared library IN-TREE with hipcc (cross-compiles without a
GPU).  The .so is git-ignored but travels to the GPU box with the snapshot."""
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB = os.path.join(PKG_DIR, "libgpcc_attr_mi355.so")
# the same library with the experiments' branches compiled in (csrc/raht_links.hpp: they cost the headline kernel
# 1.6 %, so the product leaves them out): what the GPU tier runs the opt-in paths on, through GPCC_LIB_PATH
LIB_EXPERIMENTS = os.path.join(PKG_DIR, "libgpcc_attr_mi355_experiments.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)
                  if f.endswith((".hip", ".hpp"))) + [os.path.join(ROOT, "include", "gpcc_attr_mi355.h")]


def needs_build(lib=LIB):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(s) > t for s in sources())


def build(force=False, verbose=False):
    """both libraries, compiled side by side; returns the product's"""
    running = []
    for lib, flags in ((LIB, []), (LIB_EXPERIMENTS, ["-DGPCC_EXPERIMENTS=1"])):
        if not force and not needs_build(lib):
            continue
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *flags,
               *os.environ.get("GPCC_EXTRA_FLAGS", "").split(),
               os.path.join(CSRC, "gpcc_attr_mi355.hip"), "-o", lib]
        if verbose:
            print(" ".join(cmd))
        running.append((cmd, subprocess.Popen(cmd)))
    for cmd, proc in running:
        if proc.wait():
            raise subprocess.CalledProcessError(proc.returncode, cmd)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
