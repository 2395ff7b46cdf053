"""The buffer table's lifetime rules (openal-soft_amd/host/buffer_table.cpp: release flag, reference counts, queue links, views,
the voice slot's hold) are plain C++ without a HIP header, so they are tested without a GPU: tests/host/buffer_table_main.cpp, a
stand-alone program, is compiled together with the unit under the address and undefined-behaviour sanitizers and run.  What it
asserts: see its head comment."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # (the compiler tests/test_kernel_resources.py uses)
FLAGS = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_buffer_table_rules_under_sanitizers(tmp_path):
    exe = tmp_path / "buffer_table_main"
    sources = [os.path.join(ROOT, "tests", "host", "buffer_table_main.cpp"),
               os.path.join(ROOT, "openal-soft_amd", "host", "buffer_table.cpp")]
    subprocess.run([HIPCC, *FLAGS, "-x", "c++", *sources, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffer table: ok" in run.stdout
