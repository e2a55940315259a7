"""Builds the reference renderer's own sources CPU-only into oracle/_ref/ (TEST INFRASTRUCTURE).

The reference (Ben-Edwards44/Ray-Tracer) is CUDA + SFML.  SURVEY.md §8(c) / App. B found that its sources
compile and run on the CPU with a header of CUDA stand-ins, a stub of SFML and three edited lines.  This
module is that recipe, committed: it copies the reference's src/*.cu and models/ into oracle/_ref/ (which
git ignores), applies the edits to the copy, and compiles oracle/ref_recipe/driver.cpp - which includes the
copy - once per image size, the size being a compile-time constant of the reference.

Nothing of the reference is stored in this repository: the copy is made at build time from a checkout
whose place RT_REFERENCE_DIR names (default /root/reference, where SURVEY.md read it).  Where there is no
such checkout, build() returns None and leaves an existing oracle/_ref/ alone; the fixtures under
tests/golden/ref/ are what travels.
"""
import glob
import json
import os
import platform
import re
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
RECIPE = os.path.join(_HERE, "ref_recipe")
OUT = os.path.join(_HERE, "_ref")

# One program per image size.  64x48 is the fixtures' size: no multiple of the reference's 8x8 block in
# either direction, so its grid overshoot and bounds guard are exercised.  256x256 is the size of the three
# frame hashes SURVEY.md App. C.2 recorded.
SIZES = ((64, 48), (256, 256))

# main.cu needs clang++ (g++ 11 misparses two of its lines); -fno-builtin keeps tan/sin/cos/log
# run-time libm calls (a compile-time fold of tanf is correctly rounded and differs from glibc's by 1 ulp);
# -ffp-contract=off keeps a*b+c two roundings; -Wno-parentheses for the reference's chained comparison.
# -ftrivial-auto-var-init=zero makes the fields Material::create_emissive leaves unset the zeros this project
# defines; the three recorded 256x256 hashes reproduce with it
# (tests/test_reference_pin.py::test_recorded_hashes_from_the_reference_binary).
FLAGS = ["-std=c++17", "-O2", "-fno-builtin", "-ffp-contract=off", "-ftrivial-auto-var-init=zero",
         "-Wno-parentheses", "-Wno-error=parentheses", "-w", "-pthread"]

# The survey's three edits, as patterns over public names only.  Each must match exactly once in the whole copy.
EDITS = (
    # kernel<<<grid, block>>>(args  ->  cpu_launch(kernel, grid, block, args
    (r"(\w+)\s*<<<\s*([^<>]+?)\s*>>>\s*\(", r"cpu_launch(\1, \2, "),
    (r"\bconst\s+int\s+SCREEN_WIDTH\s*=\s*[^;]+;", "const int SCREEN_WIDTH = RT_REF_W;"),
    (r"\bconst\s+int\s+SCREEN_HEIGHT\s*=\s*[^;]+;", "const int SCREEN_HEIGHT = RT_REF_H;"),
)


def reference_dir():
    return os.environ.get("RT_REFERENCE_DIR", "/root/reference")


def binary(width, height):
    return os.path.join(OUT, "refdrv_%dx%d" % (width, height))


def available():
    """True when every program of SIZES has been built."""
    return all(os.path.exists(binary(w, h)) for w, h in SIZES)


def compiler():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no clang++ found (looked under $ROCM_PATH/llvm/bin and on PATH)")


def _copy_and_edit(ref):
    src = os.path.join(OUT, "src")
    for d in (src, os.path.join(OUT, "models")):
        if os.path.isdir(d):
            os.chmod(d, 0o755)
            shutil.rmtree(d)
    os.makedirs(src)
    files = sorted(glob.glob(os.path.join(ref, "src", "*.cu")))
    if not files:
        raise RuntimeError("no src/*.cu under %s" % ref)
    text = {}
    for f in files:
        with open(f, encoding="utf-8") as fh:
            text[os.path.basename(f)] = fh.read()
    for pattern, replacement in EDITS:
        hits = [(name, m) for name, t in text.items() for m in re.finditer(pattern, t)]
        if len(hits) != 1:
            raise RuntimeError("reference edit %r matches %d times (in %s), expected exactly once: the reference "
                               "has changed, adapt oracle/ref_build.py" % (pattern, len(hits), sorted({n for n, _ in hits})))
        name = hits[0][0]
        text[name] = re.sub(pattern, replacement, text[name])
    for name, t in text.items():
        with open(os.path.join(src, name), "w", encoding="utf-8") as fh:
            fh.write(t)
    os.makedirs(os.path.join(OUT, "models"))
    for f in sorted(glob.glob(os.path.join(ref, "models", "*"))):
        shutil.copyfile(f, os.path.join(OUT, "models", os.path.basename(f)))      # contents only, not the checkout's modes


def compile_command(width, height, out):
    return [compiler()] + FLAGS + ["-I", RECIPE, "-I", OUT, "-DRT_REF_W=%d" % width, "-DRT_REF_H=%d" % height,
                                   os.path.join(RECIPE, "driver.cpp"), "-o", out]


def build_sizes(sizes, out_dir, verbose=False):
    """The driver for each (width, height) of `sizes`, compiled side by side from the copy build() made, into `out_dir`.
    build() makes the programs of SIZES in oracle/_ref/; the fixture generator makes the camera-only sizes SURVEY.md
    App. A.12 recorded in a temporary directory of its own, so oracle/_ref/ holds what build() made and nothing else."""
    paths = [os.path.join(out_dir, os.path.basename(binary(w, h))) for w, h in sizes]
    procs = []
    for (w, h), path in zip(sizes, paths):
        cmd = compile_command(w, h, path)
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    return paths


def build(verbose=False):
    """Returns the build-info dict, or None where there is no reference checkout."""
    ref = reference_dir()
    sources = glob.glob(os.path.join(ref, "src", "*.cu"))
    if not sources or not all(os.access(f, os.R_OK) for f in sources):
        if verbose:
            print("oracle.ref_build: no readable reference checkout at %s; oracle/_ref left as it is" % ref)
        return None
    os.makedirs(OUT, exist_ok=True)
    _copy_and_edit(ref)
    cxx = compiler()
    for stale in glob.glob(os.path.join(OUT, "refdrv_*")):
        os.remove(stale)
    build_sizes(SIZES, OUT, verbose)
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.splitlines()[0].strip()
    info = {"compiler": version, "flags": FLAGS, "libc": " ".join(platform.libc_ver()),
            "sizes": ["%dx%d" % s for s in SIZES]}
    with open(os.path.join(OUT, "build_info.json"), "w") as fh:
        json.dump(info, fh, indent=1)
    return info


def build_info():
    with open(os.path.join(OUT, "build_info.json")) as fh:
        return json.load(fh)


if __name__ == "__main__":
    print(build(verbose=True))
