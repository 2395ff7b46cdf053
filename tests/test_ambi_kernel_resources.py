"""AmbiParamsKernel (csrc/source_ambi_kernels.hip) from the compiler's own metadata, built with the Makefile's flags: a 64-lane
workgroup per source whose chain lives in registers and whose matrices live in LDS: no spill, no scratch (the first-order block
and the per-pass line tables are selected by comparisons or unrolled, never indexed); LDS is the rotation, the mix matrix and the
panned coefficients, reported and only bounded by 8 KB."""
import os
import shutil

import pytest

import test_kernel_resources as kr

pytestmark = pytest.mark.skipif(not (os.path.exists(kr.HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_ambi_params_kernel_does_not_spill(tmp_path):
    meta, text = kr.full_metadata(tmp_path, "source_ambi_kernels.hip")
    (name, m), = [(n, m) for n, m in meta.items() if "AmbiParamsKernel" in n]
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert m.get("sgpr_spill_count", 0) == 0, (name, m)
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 64, (name, m)
    assert (2 * 25 * 25 + 25) * 4 <= m["group_segment_fixed_size"] < 8192, (name, m)
    print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    for other, om in meta.items():                          # every kernel of the file
        assert om["vgpr_spill_count"] == 0 and om["private_segment_fixed_size"] == 0 and om.get("sgpr_spill_count", 0) == 0, (other, om)
        assert om["wavefront_size"] == 64, (other, om)
