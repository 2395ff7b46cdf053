"""SourceParamsKernel (csrc/source_kernels.hip) from the compiler's own metadata, built with the Makefile's flags (hipcc
cross-compiles for gfx950 without a GPU): a wavefront per source record whose scalar chain lives in registers -- no spill, no
scratch (a run-time index into the per-send arrays puts the whole result struct there: it happened while the kernel was
written), no LDS -- and whose fp32 divisions are the correctly rounded expansions mStep and the resampler's scale index
depend on (csrc/dev_source.hpp, "Exactness")."""
import os
import shutil

import pytest

import test_kernel_resources as kr

pytestmark = pytest.mark.skipif(not (os.path.exists(kr.HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_source_params_kernel_does_not_spill(tmp_path):
    meta, text = kr.full_metadata(tmp_path, "source_kernels.hip")
    (name, m), = [(n, m) for n, m in meta.items() if "SourceParamsKernel" in n]
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert m.get("sgpr_spill_count", 0) == 0 and m["group_segment_fixed_size"] == 0, (name, m)
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 128, (name, m)            # (four wavefronts per SIMD and more)
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 64, (name, m)
    # every division of the scalar chain and of the filter designs in full: scale, reciprocal estimate, refinement, fix-up
    body = text[text.index(name + ":"):]
    assert body.count("v_div_fixup_f32") >= 25 and body.count("v_div_fixup_f32") == body.count("v_div_fmas_f32"), body.count("v_div_fixup_f32")
    assert body.count("v_div_scale_f32") == 2 * body.count("v_div_fixup_f32")
