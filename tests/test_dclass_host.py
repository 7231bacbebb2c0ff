"""Failure classes, the parts that need no GPU: the C ABI declares and the library exports the three entry
points and the struct, the option list documents class_hash_bits, the Go drop-in calls each entry point with
the header's arity, and graphing.failure_class_order groups and orders a hand-made class_of."""
import ctypes
import os
import re

from nemo_amd import engine as E
from nemo_amd import graphing as GR
from tests.test_go_binding import GO, go_calls, header_decls

NEW = {"nemo_diff_classes": 1, "nemo_fetch_diff_classes": 5, "nemo_fetch_diff_support": 3}


def test_header_declares_the_entry_points_and_the_struct():
    funcs, _, types, fields = header_decls()
    for name, arity in NEW.items():
        assert funcs.get(name) == arity, name
    assert "nemo_diff_class" in types
    assert fields["nemo_diff_class"] == {"rep", "size", "nodes"}
    hdr = open(E.HEADER).read()
    # the calls say what they replace: nothing in the reference; they summarise CreateNaiveDiffProv's output
    assert re.search(r"Replaces nothing in the reference.*?differential-provenance\.go:18-146", hdr, flags=re.S)


def test_library_exports_them_and_abi_version_stays_1():
    L = E.lib()
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
        assert name in E.header_symbols()
    assert L.nemo_abi_version() == 1
    assert "#define NEMOHIP_ABI_VERSION 1\n" in open(E.HEADER).read()

    class CClass(ctypes.Structure):
        _fields_ = [("rep", ctypes.c_uint32), ("size", ctypes.c_uint32), ("nodes", ctypes.c_uint32)]

    assert ctypes.sizeof(CClass) == 12  # Engine.diff_classes reads the classes as rows of three u32


def test_null_context_is_rejected_without_a_device():
    L = E.lib()
    assert L.nemo_diff_classes(None) == 1  # NEMO_ERR_INVALID
    assert L.nemo_fetch_diff_classes(None, None, None, 0, None) == 1
    assert L.nemo_fetch_diff_support(None, None, 0) == 1


def test_option_list_documents_class_hash_bits():
    hdr = open(E.HEADER).read()
    opts = hdr[hdr.index("Tuning / test knobs"):hdr.index("int nemo_set_option")]
    assert '"class_hash_bits"' in opts and "0..128" in opts and "default 128" in opts


def test_go_file_calls_each_entry_point_with_the_headers_arity():
    src = open(GO).read()
    assert re.search(r"func \(n \*Neo4J\) FailureClasses\(", src)
    calls = go_calls(src)
    for name, arity in NEW.items():
        got = [a for n, a in calls if n == name]
        assert got and all(a == arity for a in got), (name, got)
    assert "C.nemo_diff_class" in src


def test_failure_class_order_groups_and_orders():
    failed = [11, 12, 13, 14, 15, 16, 12]
    class_of = [0, 1, 0, 2, 1, 3, 1]
    classes = [(0, 2, 7), (1, 3, 9), (3, 1, 0), (5, 1, 4)]  # (rep, size, nodes), by smallest entry
    got = GR.failure_class_order(failed, class_of, classes)
    # largest first; the two singletons in order of their representatives; duplicates once per entry
    assert got == [(1, 12, [12, 15, 12]), (0, 11, [11, 13]), (2, 14, [14]), (3, 16, [16])]
    assert GR.failure_class_order([], [], []) == []
    # ties between larger classes too: by representative entry, not by iteration
    assert [k for k, _, _ in GR.failure_class_order([9, 3, 9, 3], [0, 1, 0, 1], [(0, 2, 1), (1, 2, 1)])] == [0, 1]


def test_host_check_program_is_committed():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "tools", "dclass_host_check.cpp")).read()
    assert "int main()" in src and '#include "../nemo_amd/csrc/dclass_host.h"' in src
