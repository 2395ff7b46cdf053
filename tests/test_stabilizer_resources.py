"""The front stabilizer's and the distance compensation's kernels (csrc/stabilizer_kernels.hip), from the compiler's metadata as
tests/test_limiter_resources.py reads it: no spills, no scratch, at most 32 KB of static LDS.  They run on the post stream beside
the next update's voice kernel, the stabilizer as one workgroup."""
import os
import shutil

import pytest

from test_limiter_resources import HIPCC, ROOT, metadata      # (the same hipcc invocation)

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_stabilizer_kernels_do_not_spill(tmp_path):
    mk = open(os.path.join(ROOT, "openal-soft_amd", "Makefile")).read()
    assert "csrc/stabilizer_kernels.hip" in mk and "host/stabilizer_params.cpp" in mk
    meta = metadata(tmp_path, "stabilizer_kernels.hip")
    names = sorted(meta)
    assert len(names) == 3, names
    for want in ("StabilizerSplitKernel", "StabilizerKernel", "DistanceCompKernel"):
        assert any(want in n for n in names), (want, names)
    for name, m in meta.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] <= 32 * 1024, (name, m)
    main = next(m for n, m in meta.items() if "16StabilizerKernel" in n)
    assert 0 < main["group_segment_fixed_size"]                 # the tiles are staged in LDS
    assert main["vgpr_count"] + main.get("agpr_count", 0) <= 128, main
