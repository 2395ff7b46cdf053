"""SourceNfcKernel (csrc/source_nfc_kernels.hip) from the compiler's own metadata, built with the Makefile's flags: a wavefront
per source that keeps of SourceAttenuation only the chain up to the distance, in registers -- no spill, no scratch, no LDS --
and whose fp32 divisions (the w0, the sections' coefficients, normalize()'s) are all the correctly rounded expansion: every
v_div_fixup_f32 has its v_div_fmas_f32 (csrc/dev_source.hpp, "Exactness")."""
import os
import shutil

import pytest

import test_kernel_resources as kr

pytestmark = pytest.mark.skipif(not (os.path.exists(kr.HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_source_nfc_kernel_does_not_spill(tmp_path):
    meta, text = kr.full_metadata(tmp_path, "source_nfc_kernels.hip")
    (name, m), = [(n, m) for n, m in meta.items() if "SourceNfcKernel" in n]
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert m.get("sgpr_spill_count", 0) == 0 and m["group_segment_fixed_size"] == 0, (name, m)
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 128, (name, m)
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 64, (name, m)
    body = text[text.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert body.count("v_div_fixup_f32") >= 1 and body.count("v_div_fixup_f32") == body.count("v_div_fmas_f32"), body.count("v_div_fixup_f32")
    print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")}, body.count("v_div_fixup_f32"))
