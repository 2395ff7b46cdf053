"""The merge of a device context's attached contexts (csrc/bus_merge_kernels.hip), from the compiler's metadata as
tests/test_limiter_resources.py reads it.  BusMergeKernel runs on the device context's post stream beside the next update's
voice kernel, like the post-process kernels: no LDS, no scratch, no spills, and at most 32 VGPRs -- a wavefront of it then
finds room on a SIMD beside four wavefronts of the voice-per-wavefront HRTF kernel (4 x 112 + 32 <= 512 registers per lane)."""
import os
import shutil

import pytest

from test_limiter_resources import HIPCC, ROOT, metadata      # (the same hipcc invocation)

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_bus_merge_kernel_needs_no_lds_no_scratch_and_32_registers(tmp_path):
    assert "csrc/bus_merge_kernels.hip" in open(os.path.join(ROOT, "openal-soft_amd", "Makefile")).read()
    meta = metadata(tmp_path, "bus_merge_kernels.hip")
    assert len(meta) == 1 and "BusMergeKernel" in next(iter(meta)), sorted(meta)      # exactly the merge kernel
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] + m.get("agpr_count", 0) <= 32, (name, m)
