"""The seam between rt_kernel.hip and the host translation units - the kernel launchers and rt_kernel_blocks_per_cu, C linkage - is declared
in ray-tracer_amd/csrc/rt_launch.h and nowhere else, so that the compilers check every definition, caller and stub against the one
declaration.  Textual, CPU only: no other file under csrc/ holds a prototype of one; every declared name is defined once in the kernel
headers (beside the refusing fallbacks of rt_ray_kernels.h) and once in tests/sanitize/launcher_stubs.h; no program under tests/sanitize/
defines one itself."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracer_amd", "csrc")
SANITIZE = os.path.join(ROOT, "tests", "sanitize")
NAME = r"\b(rt_launch_\w+|rt_kernel_blocks_per_cu)\s*\("
# a return type, the name at nesting depth 0, its parameter list (no parentheses inside: none of the launchers takes a function), then ...
HEAD = r"^[ \t]*(?:extern\s+\"C\"\s+)?(?:static\s+|inline\s+)*(?:hipError_t|int)\s+" + NAME + r"[^()]*\)\s*"
PROTOTYPE = re.compile(HEAD + r";", re.M)           # ... a semicolon: a declaration
DEFINITION = re.compile(HEAD + r"\{", re.M)         # ... a body: a definition


def _text(path):
    with open(path) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)


def _names(pattern, path):
    return [m.group(1) for m in pattern.finditer(_text(path))]


HEADER = os.path.join(CSRC, "rt_launch.h")
DECLARED = _names(PROTOTYPE, HEADER)


def test_the_header_declares_each_function_once_inside_one_extern_c_block():
    text = _text(HEADER)
    assert len(DECLARED) == len(set(DECLARED)) and {"rt_kernel_blocks_per_cu", "rt_launch_render"} <= set(DECLARED), DECLARED
    assert len(re.findall(r'extern\s+"C"', text)) == 1 and _names(DEFINITION, HEADER) == []
    block = text[text.index('extern "C"'):text.rindex("}")]
    assert [m.group(1) for m in PROTOTYPE.finditer(block)] == DECLARED
    assert not re.search(r"#\s*include\s*<hip/hip_runtime\.h>", text)       # a host header (test_headers_compile.py: through g++)


def test_no_other_file_of_the_library_declares_a_launcher():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) != "rt_launch.h" and _names(PROTOTYPE, path):
            found[os.path.basename(path)] = _names(PROTOTYPE, path)
    assert found == {}, found


def test_every_launcher_is_defined_once_in_the_kernel_headers():
    defined = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) != "rt_ray_kernels.h":
            defined += _names(DEFINITION, path)
    assert sorted(defined) == sorted(DECLARED), sorted(set(defined) ^ set(DECLARED))
    # the development builds' fallbacks: ray-kernel launchers that the header declares, and behind its include
    ray = _text(os.path.join(CSRC, "rt_ray_kernels.h"))
    fallbacks = [m.group(1) for m in DEFINITION.finditer(ray)]
    assert sorted(fallbacks) == ["rt_launch_ao", "rt_launch_multihit", "rt_launch_multihit_uv", "rt_launch_occlusion", "rt_launch_overlap", "rt_launch_query",
                                 "rt_launch_tritri"], fallbacks
    assert ray.index('#include "rt_launch.h"') < DEFINITION.search(ray).start()


def test_every_file_that_defines_a_launcher_includes_the_header():
    for path in sorted(glob.glob(os.path.join(CSRC, "*")) + [os.path.join(SANITIZE, "launcher_stubs.h")]):
        if _names(DEFINITION, path):
            assert re.search(r'#\s*include\s*"rt_launch\.h"', _text(path)), path


def test_the_stubs_define_every_launcher_once_and_no_program_defines_one():
    assert sorted(_names(DEFINITION, os.path.join(SANITIZE, "launcher_stubs.h"))) == sorted(DECLARED)
    programs = sorted(glob.glob(os.path.join(SANITIZE, "*.cpp")))
    assert len(programs) >= 6, programs
    for path in programs:
        assert _names(DEFINITION, path) == [] and _names(PROTOTYPE, path) == [], path


def test_the_patterns_find_what_they_are_for():
    """the forms the parent commits had, which must not come back unseen: a prototype in a caller, a stub in a program, and the launchers that
    were declared in their family's header and fell back at the foot of their kernel header"""
    old = ('extern "C" hipError_t rt_launch_exhaustive(unsigned long long *out4, hipStream_t stream);\n'
           'extern "C" hipError_t rt_launch_blend_tiles(const float *partial, long long plane_floats,\n'
           '                                            const uint32_t *tile_list, hipStream_t stream);\n'
           'extern "C" int rt_kernel_blocks_per_cu(rt_shape, size_t) { return 1; }\n'
           'extern "C" hipError_t rt_launch_ao(const rt_ao_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }\n'
           'extern "C" {\n'
           'hipError_t rt_launch_nearest(const rt_nearest_args *args, rt_shape shape, int front, int num_cus, size_t lds_bytes, hipStream_t stream);\n'
           '}\n'
           '#else\n'
           'extern "C" hipError_t rt_launch_multihit(const rt_multihit_args *, rt_shape, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }\n'
           '#endif\n'
           '    if (e == hipSuccess) e = rt_launch_exhaustive(d, nullptr);\n'
           '    RT_HIP(ctx, rt_launch_rgba8(d_rgb, width * height, d_rgba, (hipStream_t)hip_stream), "launching rgba8 kernel");\n')
    assert [m.group(1) for m in PROTOTYPE.finditer(old)] == ["rt_launch_exhaustive", "rt_launch_blend_tiles", "rt_launch_nearest"]
    assert [m.group(1) for m in DEFINITION.finditer(old)] == ["rt_kernel_blocks_per_cu", "rt_launch_ao", "rt_launch_multihit"]
