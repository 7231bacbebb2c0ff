"""Host-side checks of the sliced hand-over (no GPU): the option is documented, a null context is rejected, and the
slice arithmetic (nemo_amd/csrc/stage_host.h: slice bounds from the node count, the pair capacity and the slice count)
passes its stand-alone check program under the host sanitizers: more slices than words, a capacity of zero, a capacity
no multiple of the slice count, and the ranges tiling [0, n) exactly once."""
import os
import shutil
import subprocess

import pytest

from nemo_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_list_documents_the_option():
    hdr = open(E.HEADER).read()
    opts = hdr[hdr.index("Tuning / test knobs"):hdr.index("int nemo_set_option")]
    assert '"stage_slices"' in opts and "1..8, default 2" in opts
    assert '"stage_slice_ratio"' in opts and "1..8, default 4" in opts
    assert '"stage_pair_slices"' in opts and "1..8, default 1" in opts
    src = open(os.path.join(ROOT, "nemo_amd", "csrc", "stage_host.h")).read()
    for d in ("NEMO_STAGE_SLICES_MAX 8u", "NEMO_STAGE_SLICES_DEFAULT 2u", "NEMO_STAGE_RATIO_DEFAULT 4u",
              "NEMO_STAGE_PAIR_SLICES_DEFAULT 1u"):
        assert "#define " + d in src, d


def test_null_context_is_rejected_without_a_device():
    assert E.lib().nemo_set_option(None, b"stage_slices", 2) == 1  # NEMO_ERR_INVALID


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "stage_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/stage_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "stage_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "stage_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/stage_host_check.cpp")
    exe = str(tmp_path / "stage_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "stage_host_check", f"STAGE_CHECK={exe}"],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("stage_host_check OK")
