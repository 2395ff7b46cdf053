"""The TSME encoder's kernels (csrc/tsme_kernels.hip), from the compiler's metadata as tests/test_limiter_resources.py reads
it: no spills, no scratch, and at most 32 KB of LDS.  Like the UHJ encoder's they run on the post stream beside the next
update's voice kernel, one workgroup each: within 32 KB a workgroup finds room on a CU whose other workgroups are voice
workgroups (160 KB per CU), whichever voice kernel runs.  The largest, FIR-512, stages the W/X history and four delay lines
with the update behind them: (639 + 1024) + 4 (384 + 1024) floats = 29180 bytes."""
import os
import shutil

import pytest

from test_limiter_resources import HIPCC, ROOT, metadata      # (the same hipcc invocation)

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_tsme_kernels_do_not_spill(tmp_path):
    assert "csrc/tsme_kernels.hip" in open(os.path.join(ROOT, "openal-soft_amd", "Makefile")).read()
    meta = metadata(tmp_path, "tsme_kernels.hip")
    names = sorted(meta)
    assert len(names) == 3 and any("TsmeIirKernel" in n for n in names) and sum("TsmeFirKernel" in n for n in names) == 2, names
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 32 * 1024, (name, m)
    fir512 = next(m for n, m in meta.items() if "Lj512" in n)
    assert fir512["group_segment_fixed_size"] == 29180, fir512
