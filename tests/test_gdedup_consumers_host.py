"""The duplicate-graph consumers, the parts that need no GPU: the option list documents proto_dedup and pull_dedup,
the fetch contract says that graphs of identical content share a region, and the host check program (run classes,
the pull's slot map) passes."""
import os
import shutil
import subprocess

import pytest

from nemo_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_list_documents_the_options():
    hdr = open(E.HEADER).read()
    opts = hdr[hdr.index("Tuning / test knobs"):hdr.index("int nemo_set_option")]
    for name in ('"proto_dedup"', '"pull_dedup"', '"replicate_lazy"'):
        assert name in opts
    contract = hdr[hdr.index("Every slot at once"):hdr.index("int nemo_fetch_pulled_all")]
    assert "identical content" in contract and "pull_dedup" in contract


def test_null_context_is_rejected_without_a_device():
    for name in (b"proto_dedup", b"pull_dedup", b"replicate_lazy"):
        assert E.lib().nemo_set_option(None, name, 0) == 1  # NEMO_ERR_INVALID


def test_host_check_program_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "gdedup_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tools", "gdedup_host_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.rstrip().endswith("gdedup_host_check OK") and "duplicate runs" in out
