"""Builds libsim3opt.so in-tree with hipcc for gfx950 (MI355X).

    python -m sim3opt_amd.build [--force]                       the product library (the Makefile's recipe)
    python -m sim3opt_amd.build --flags "-DFOO=1 ..." --out PATH   an experiment build, loaded with SIM3OPT_LIB=PATH

build() is the product whatever the environment holds: one flag list, the translation units of csrc/SOURCES.
An experiment build never writes the product library.  The .so is git-ignored.
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsim3opt.so")
# the one list of translation units, shared with the Makefile
SOURCES = open(os.path.join(CSRC, "SOURCES")).read().split()
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp")) + [
    os.path.join("..", "..", "include", "sim3opt.h"), os.path.join("..", "..", "include", "sim3opt_bench.h"), "SOURCES"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
         "-Wall", "-Wno-unused-result", "-pthread"]


def command(extra_flags=(), out=LIB):
    """argv of the one hipcc call.  Extra flags make an experiment build, which may not land on the product library."""
    extra_flags = list(extra_flags)
    if extra_flags and os.path.realpath(out) == os.path.realpath(LIB):
        raise ValueError(f"an experiment build ({' '.join(extra_flags)}) must not overwrite the product library {LIB}")
    return [HIPCC] + FLAGS + extra_flags + ["-o", out] + [os.path.join(CSRC, s) for s in SOURCES] + ["-ldl"]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    cmd = command()
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--force", action="store_true", help="rebuild the product library even if it is up to date")
    ap.add_argument("--flags", default="", help="extra compiler flags of an experiment build (needs --out)")
    ap.add_argument("--out", help="where an experiment build goes; never the product library")
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--flags" in argv[:-1]:  # (argparse takes a lone "-DFOO=1" after --flags for an option: hand it over as --flags=...)
        i = argv.index("--flags")
        argv[i:i + 2] = ["--flags=" + argv[i + 1]]
    a = ap.parse_args(argv)
    if a.out is None:
        if a.flags:
            ap.error("--flags needs --out: an experiment build does not replace the product library")
        print(build(force=a.force, verbose=True))
        return
    if os.path.realpath(a.out) == os.path.realpath(LIB):
        raise ValueError(f"--out {a.out} is the product library: build that with no --out")
    cmd = command(a.flags.split(), a.out)
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    print(a.out)


if __name__ == "__main__":
    main()
