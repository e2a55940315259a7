"""Builds ray-tracer_amd/libraytracer_amd.so (HIP kernels + C ABI) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU; the built .so travels with the repo snapshot to the GPU
box.  -ffp-contract=off is mandatory: the reference's `a*b+c` are two roundings and a fused
multiply-add changes hit/miss decisions (hard part 1).
"""
import glob
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libraytracer_amd.so")
SOURCES = [os.path.join(HERE, "csrc", f) for f in ("rt_kernel.hip", "rt_capi.cpp", "rt_pipeline_capi.cpp", "rt_multi_capi.cpp", "rt_query_capi.cpp", "rt_occlusion_capi.cpp", "rt_ao_capi.cpp", "rt_nearest_capi.cpp", "rt_sweep_capi.cpp", "rt_multihit_capi.cpp", "rt_overlap_capi.cpp", "rt_tritri_capi.cpp", "rt_winding_capi.cpp", "rt_denoise_capi.cpp", "rt_adaptive_capi.cpp", "rt_views_capi.cpp", "rt_sky_capi.cpp", "rt_update_capi.cpp", "rt_host.cpp")]
# every header there is: a new one cannot be forgotten, and needs_build() then serves no stale library after an edit
HEADERS = sorted(glob.glob(os.path.join(HERE, "csrc", "*.h"))) + [os.path.join(ROOT, "include", "rt_amd.h")]
# text a header includes more than once (the wave loop both render kernels run): watched like the headers
INCLUDED = sorted(glob.glob(os.path.join(HERE, "csrc", "*.inc")))
# -fno-slp-vectorize: the SLP vectorizer pairs the scalar f32 adds / multiplies of the vector math into v_pk_*_f32, which
# are not faster on gfx950 and need register pairs: 128 instead of ~90 VGPRs and ~10 % more time (same-box A/B, round 2).
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared", "-std=c++17",
         "-Wall", "-Wno-unused-result", "-I" + os.path.join(ROOT, "include")]


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP extension cannot be built")
    return exe


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(p) > t for p in SOURCES + HEADERS + INCLUDED)


def build_variant(name, extra_flags):
    """development builds (e.g. -DRT_STATS) next to the product library; never loaded by default"""
    out = os.path.join(HERE, "libraytracer_amd_%s.so" % name)
    subprocess.check_call([hipcc()] + FLAGS + list(extra_flags) + SOURCES + ["-o", out])
    return out


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    cmd = [hipcc()] + FLAGS + SOURCES + ["-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


EXAMPLE = os.path.join(HERE, "host", "example_main")
QUERY_EXAMPLE = os.path.join(HERE, "host", "example_query")
DENOISE_EXAMPLE = os.path.join(HERE, "host", "example_denoise")
ADAPTIVE_EXAMPLE = os.path.join(HERE, "host", "example_adaptive")
VIEWS_EXAMPLE = os.path.join(HERE, "host", "example_views")
ANIMATE_EXAMPLE = os.path.join(HERE, "host", "example_animate")
SKY_EXAMPLE = os.path.join(HERE, "host", "example_sky")
NEAREST_EXAMPLE = os.path.join(HERE, "host", "example_nearest")
XRAY_EXAMPLE = os.path.join(HERE, "host", "example_xray")
SDF_EXAMPLE = os.path.join(HERE, "host", "example_sdf")
SWEEP_EXAMPLE = os.path.join(HERE, "host", "example_sweep")
VOXELIZE_EXAMPLE = os.path.join(HERE, "host", "example_voxelize")
SLICE_EXAMPLE = os.path.join(HERE, "host", "example_slice")


def _build_host_program(source, exe):
    build()
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", os.path.join(HERE, "host", source), "-o", exe,
           "-L" + HERE, "-lraytracer_amd", "-Wl,-rpath," + HERE, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    subprocess.check_call(cmd)
    return exe


def build_example():
    """The C++ host-side mirror (host/raytracer.hpp) compiled into a small program with g++."""
    return _build_host_program("example_main.cpp", EXAMPLE)


def build_query_example():
    """The mirror's ray queries and first-hit planes (host/example_query.cpp): what the centre pixel sees, the depth plane as a PGM."""
    return _build_host_program("example_query.cpp", QUERY_EXAMPLE)


def build_denoise_example():
    """The mirror's denoiser (host/example_denoise.cpp): the reference's monkey_test_scene (scene 0) at a few samples per pixel, noisy and denoised side by side as a PNG."""
    return _build_host_program("example_denoise.cpp", DENOISE_EXAMPLE)


def build_adaptive_example():
    """The mirror's adaptive sampling (host/example_adaptive.cpp): the monkey scene sampled to a noise target, the frame and the map of where the samples went as PNGs."""
    return _build_host_program("example_adaptive.cpp", ADAPTIVE_EXAMPLE)


def build_views_example():
    """The mirror's camera sequences (host/example_views.cpp): an orbit of the monkey scene as numbered PNGs from one launch, and one depth-of-field frame."""
    return _build_host_program("example_views.cpp", VIEWS_EXAMPLE)


def build_animate_example():
    """The mirror's time-varying geometry (host/example_animate.cpp): the monkey bent step by step through Renderer::update_mesh, a PNG per step."""
    return _build_host_program("example_animate.cpp", ANIMATE_EXAMPLE)


def build_sky_example():
    """The mirror's environment lighting (host/example_sky.cpp): the monkey under a procedural gradient-and-sun cube map, as a PNG."""
    return _build_host_program("example_sky.cpp", SKY_EXAMPLE)


def build_nearest_example():
    """The mirror's nearest-surface queries (host/example_nearest.cpp): a slice of the monkey's distance field as a PGM."""
    return _build_host_program("example_nearest.cpp", NEAREST_EXAMPLE)


def build_xray_example():
    """The mirror's multi-hit queries (host/example_xray.cpp): the number of surfaces along every primary ray of the monkey view as a PGM."""
    return _build_host_program("example_xray.cpp", XRAY_EXAMPLE)


def build_sdf_example():
    """The mirror's winding-number queries (host/example_sdf.cpp): a slice of the monkey's signed distance field as a PGM."""
    return _build_host_program("example_sdf.cpp", SDF_EXAMPLE)


def build_sweep_example():
    """The mirror's sphere-cast queries (host/example_sweep.cpp): a ball dropped straight down on a grid over the monkey, its rest heights as a PGM."""
    return _build_host_program("example_sweep.cpp", SWEEP_EXAMPLE)


def build_voxelize_example():
    """The mirror's box-overlap queries (host/example_voxelize.cpp): the monkey voxelised, one slice as a PGM, the surface and solid cells counted."""
    return _build_host_program("example_voxelize.cpp", VOXELIZE_EXAMPLE)


def build_slice_example():
    """The mirror's triangle-overlap queries (host/example_slice.cpp): a cross-section of the monkey, its outline rasterised from the segments into a PGM."""
    return _build_host_program("example_slice.cpp", SLICE_EXAMPLE)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
