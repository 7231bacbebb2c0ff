"""Duplicate graphs, the parts that need no GPU: the option list documents graph_dedup and dedup_hash_bits, a null
context is rejected, and the host check program of gdedup_host.h is committed."""
import os

from nemo_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_list_documents_the_options():
    hdr = open(E.HEADER).read()
    opts = hdr[hdr.index("Tuning / test knobs"):hdr.index("int nemo_set_option")]
    assert '"graph_dedup"' in opts and "1 (default)" in opts
    assert '"dedup_hash_bits"' in opts and "0..128" in opts and "default 128" in opts


def test_null_context_is_rejected_without_a_device():
    assert E.lib().nemo_set_option(None, b"graph_dedup", 0) == 1  # NEMO_ERR_INVALID


def test_host_check_program_is_committed():
    src = open(os.path.join(ROOT, "tools", "gdedup_host_check.cpp")).read()
    assert "int main()" in src and '#include "../nemo_amd/csrc/gdedup_host.h"' in src
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "gdedup_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
