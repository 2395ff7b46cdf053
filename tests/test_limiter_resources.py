"""The output limiter kernel's budgets (csrc/limiter_kernels.hip), from the compiler's metadata as
tests/test_kernel_resources.py reads it: no spills, and one workgroup fits on a CU beside the resident
voice kernel (OALGPU_CTX_RESIDENT).  The limiter runs behind the resident post-process while the voice
workgroups stay on their CUs, and the next update's reduction waits for it: if it found no room, nothing
would move again."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openal-soft_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def makefile_flags():
    text = open(os.path.join(ROOT, "openal-soft_amd", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", text, re.M).group(1).split()
    hip = re.search(r"^HIPFLAGS := (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(CXXFLAGS)", " ".join(cxx)).split()
    per_file = {m.group(1): m.group(2).split() for m in re.finditer(r"^FLAGS_(\w+)\s*:= (.*)$", text, re.M)}
    return hip, per_file


def metadata(tmp_path, source):
    hip, per_file = makefile_flags()
    out = tmp_path / (source + ".s")
    subprocess.run([HIPCC, *hip, *per_file.get(source[:-4], []), "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                    "-o", str(out), os.path.join(CSRC, source)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = {}
    for block in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", block))
        if "name" in fields:
            meta[fields["name"]] = {k: int(v) for k, v in fields.items() if v.isdigit()}
    return meta


def granule(n, g=8):
    return (n + g - 1) // g * g


def test_limiter_kernel_does_not_spill_and_fits_beside_the_resident_voice_kernel(tmp_path):
    assert "csrc/limiter_kernels.hip" in open(os.path.join(ROOT, "openal-soft_amd", "Makefile")).read()
    lim = metadata(tmp_path, "limiter_kernels.hip")
    (name, m), = [(n, m) for n, m in lim.items() if "LimiterKernel" in n]
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    # one wavefront per SIMD (256 threads), beside four wavefronts of the resident voice-per-wavefront kernel (512 registers per lane)
    voice = metadata(tmp_path, "voice_wave16.hip")
    k16r = next(v for n, v in voice.items() if "VoiceWave16KernelILb0ELi16ELb0ELb1E" in n)
    assert 4 * granule(k16r["vgpr_count"] + k16r.get("agpr_count", 0)) + granule(m["vgpr_count"] + m.get("agpr_count", 0)) <= 512, (k16r, m)
    # LDS: 160 KB per CU in granules of 1280 bytes
    assert granule(k16r["group_segment_fixed_size"], 1280) + granule(m["group_segment_fixed_size"], 1280) <= 160 * 1024, (k16r, m)
