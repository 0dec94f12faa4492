"""The flagship kernel's static resources, read from the built library's own code object metadata
(tools/kernel_resources.py: the NT_AMDGPU_METADATA note's counts — no instruction is inspected):

* wf_finish_bvh<false, 4> stays within 128 VGPRs (4 waves per SIMD), spills no more vector registers than
  before RT_COLD_ARGS (12) and no more scalar registers than RT_COLD_ARGS left it with;
* the kernels that read their WfState and camera arguments in place (wf_state.h wf_cold_state,
  wf_cold_camera) find them where the header says: the argument table's offsets are the header's
  WF_KERNARG_* values, for every instantiation of wf_finish_bvh and wf_long.
"""
import os
import sys

import pytest

import rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

VGPR_SPILL_BEFORE = 12  # wf_finish_bvh<false, 4> before RT_COLD_ARGS (200 SGPR spills, 44 B of scratch per lane)
# wf_finish_bvh<false, 4> of this tree as built by build.py's flags (python tools/kernel_resources.py; also
# profiles/fin_trip/resources.txt); before RT_COLD_ARGS: 200
SGPR_SPILL_ACHIEVED = 79
# wf_state.h: WF_KERNARG_FRAME, WF_KERNARG_CAMERA, WF_KERNARG_STATE and the arguments' sizes (its static_assert)
KERNARG = [[0, 248], [248, 112], [360, 56], [416, 344]]


@pytest.fixture(scope="module")
def kernels():
    rt.lib()  # the library must exist
    return kernel_resources.kernels(rt.LIB_PATH)


def test_finisher_registers_and_spills(kernels):
    name, k = kernel_resources.find(rt.LIB_PATH, *kernel_resources.FIN_DEFAULT)
    print(name, k)
    assert k["vgpr_count"] <= 128, k
    assert k["vgpr_spill_count"] <= VGPR_SPILL_BEFORE, k
    assert k["sgpr_spill_count"] <= SGPR_SPILL_ACHIEVED, k


def test_in_place_arguments_are_where_the_header_says(kernels):
    names = [n for n in kernels if n.startswith("_Z13wf_finish_bvh") or n.startswith("_Z7wf_long")]
    assert len(names) >= 5, sorted(kernels)  # wf_finish_bvh<false|true, 4>, <false, 1>, wf_long<false|true>
    for n in names:
        assert kernels[n]["args"][:4] == KERNARG, (n, kernels[n]["args"])
