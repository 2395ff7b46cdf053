"""ChannelParamsKernel (csrc/source_channel_kernels.hip) from the compiler's own metadata, built with the Makefile's flags: a
wavefront per channel voice whose chain -- SourceParamsKernel's plus the channel's map entry and warp -- lives in registers: no
spill, no scratch (the channel map is selected by comparisons, never indexed), no LDS; and whose fp32 divisions are the
correctly rounded expansions mStep depends on (csrc/dev_source.hpp, "Exactness")."""
import os
import shutil

import pytest

import test_kernel_resources as kr

pytestmark = pytest.mark.skipif(not (os.path.exists(kr.HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_channel_params_kernel_does_not_spill(tmp_path):
    meta, text = kr.full_metadata(tmp_path, "source_channel_kernels.hip")
    (name, m), = [(n, m) for n, m in meta.items() if "ChannelParamsKernel" in n]
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert m.get("sgpr_spill_count", 0) == 0 and m["group_segment_fixed_size"] == 0, (name, m)
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 128, (name, m)            # (four wavefronts per SIMD and more)
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 64, (name, m)
    body = text[text.index(name + ":"):]
    assert body.count("v_div_fixup_f32") >= 25 and body.count("v_div_fixup_f32") == body.count("v_div_fmas_f32"), body.count("v_div_fixup_f32")
    assert body.count("v_div_scale_f32") == 2 * body.count("v_div_fixup_f32")
    print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")}, body.count("v_div_fixup_f32"))
