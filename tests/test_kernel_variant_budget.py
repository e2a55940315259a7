"""The register / scratch budget of rt_traits_kernel, the render kernel's variant for scenes of known traits (rt_render_kernel.h), read from the
code object inside the shipped library like tests/test_kernel_budget.py reads rt_render_kernel's, and held to the limits that test holds the
generic kernel of the same shape to - or tighter: the variant exists to issue fewer instructions, and a spill it adds would be paid in the
sections it was written to shorten.  CPU test: nothing runs on a GPU."""
import os
import re

import pytest

from test_kernel_budget import LLVM, kernel_notes

SHAPES_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ray-tracer_amd", "csrc", "rt_device_scene.h")


def shape_of(name):
    m = re.search(r"ILi(\d+)ELb([01])ELi([012])E", name)
    return int(m.group(1)), m.group(2) == "1", int(m.group(3))


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_traits_kernel_register_budget(rt, tmp_path):
    notes = kernel_notes(rt, tmp_path)
    traits = {shape_of(n): v for n, v in notes.items() if "rt_traits_kernel" in n}
    generic = {shape_of(n): v for n, v in notes.items() if "rt_render_kernel" in n}
    # one per shape whose class has a trait set (rt_variant_traits, rt_device_scene.h): the scene-in-LDS shapes, four without and four with a mesh
    assert sorted(traits) == sorted(s for s in generic if s[2] == 1), sorted(traits)
    report = []
    for (nt, mesh, mode), v in sorted(traits.items()):
        g = generic[(nt, mesh, mode)]
        report.append("NT=%4d mesh=%d mode=%d: %s (generic: %d VGPRs, %d SGPR spills)" % (nt, mesh, mode, v, g["vgpr_count"], g["sgpr_spill_count"]))
        assert v["agpr_count"] == 0, v
        # no VGPR spill, no scratch instruction and no private segment in ANY shape: tighter than the generic kernels without a mesh, which
        # keep up to 8 values of the once-per-pixel code in scratch
        assert v["vgpr_spill_count"] == 0 and v["scratch_insts"] == 0 and v["private_segment_fixed_size"] == 0, ((nt, mesh, mode), v)
        # the occupancy limits of the shape, as for the generic kernel: <= 80 VGPRs for six waves per SIMD without a mesh, <= 96 for five with
        # one, <= 128 for the 1024-thread workgroup's four
        assert v["vgpr_count"] <= (128 if nt == 1024 else (96 if mesh else 80)), ((nt, mesh, mode), v)
        # ... and never more registers than the generic kernel of the shape
        assert v["vgpr_count"] <= g["vgpr_count"], ((nt, mesh, mode), v, g)
        # SGPR spills go to VGPR lanes; the same bound as the generic LDS shapes
        assert v["sgpr_spill_count"] <= 80, ((nt, mesh, mode), v)
    print("\n".join(report))
