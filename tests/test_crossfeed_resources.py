"""The bs2b crossfeed's kernels (csrc/crossfeed_kernels.hip), from the compiler's metadata as tests/test_limiter_resources.py
reads it: no spills, no scratch, and at most 32 KB of LDS (the two staged lines and the four chains' outputs: 24 KB).  They run
on the post stream beside the next update's voice kernel, one workgroup each."""
import os
import shutil

import pytest

from test_limiter_resources import HIPCC, ROOT, metadata      # (the same hipcc invocation)

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_crossfeed_kernels_do_not_spill(tmp_path):
    assert "csrc/crossfeed_kernels.hip" in open(os.path.join(ROOT, "openal-soft_amd", "Makefile")).read()
    meta = metadata(tmp_path, "crossfeed_kernels.hip")
    names = sorted(meta)
    assert len(names) == 2 and any("CrossfeedSplitKernel" in n for n in names) and any("CrossfeedKernel" in n for n in names), names
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 32 * 1024, (name, m)
